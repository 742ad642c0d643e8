"""What "bit for bit" means in this suite: one definition for torch tensors (on either device) and numpy arrays."""
import numpy as np
import torch

_TORCH_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NUMPY_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(x):
    """The elements of ``x`` as integers of their width: of a tensor on its device, of anything else as a numpy array."""
    if torch.is_tensor(x):
        return x.detach().contiguous().view(_TORCH_INT[x.element_size()])
    a = np.asarray(x)
    return np.ascontiguousarray(a).view(_NUMPY_UINT[a.dtype.itemsize]).reshape(a.shape)


def same_bits(a, b):
    """True only for equal shape, equal dtype and equal bit patterns: +0.0 is not -0.0, and a NaN equals only a NaN of
    the same payload.  Both tensors (compared on the host when their devices differ) or both numpy arrays; a comparison
    across dtypes states its ``.view(...)`` at the call."""
    if torch.is_tensor(a) != torch.is_tensor(b):
        raise TypeError("same_bits: a tensor against an array; convert one of them at the call")
    if not torch.is_tensor(a):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
