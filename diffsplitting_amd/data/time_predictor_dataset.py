"""``data/time_predictor_dataset.py`` of the reference on the device: what the TimePredictor is fed.

``compute_input_normalization_dict`` (:6-21) is ``n + 1`` numpy passes over the whole frame set in the reference; here
it is one HIP launch (``dsx_mix_range``, include/dsx.h) over the frames resident in HBM, bitwise equal to numpy's float64
result.  ``TimePredictorDataset`` (:24-89) returns ``(inp, t)`` items whose mixing and min-max normalisation run in the
fused tile kernel (``dsx_tiles_gather_mix``, channel 1); ``batch`` cuts a whole batch of them, every item with its own
drawn ``t``, in one launch (``dsx_tiles_gather_mix_items``).

Refused loudly (training-time only): ``gaussian_noise_std_factor``, ``enable_transforms``, ``uncorrelated_channels``.
"""
import ctypes as C
import inspect

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib
from .split_dataset import DataLocation, SplitDataset, compute_normalization_dict  # noqa: F401  (the reference's imports)


def _frames(x, device):
    """One channel's frames -> a contiguous float32 tensor on the device (numpy arrays and lists are uploaded)."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    return x.to(device=device, dtype=torch.float32).contiguous()


def compute_input_normalization_dict(data_dict, n_timesteps, mean_target, std_target, device="cuda"):
    """:6-21.  ``{t_int: [min, max]}`` (numpy float64) for t_int in 0..n_timesteps: the range, over every pixel of every
    frame, of ``t*ch0 + (1-t)*ch1`` with t = t_int / n_timesteps on the normalised channels, in float64 as numpy
    computes it (bitwise, for frames float32 holds exactly: integer-valued microscope frames).  ``data_dict``: the
    ``_data_dict`` of the engine's datasets (device tensors), or numpy arrays / lists of frames, which are uploaded."""
    mean = np.asarray(mean_target, dtype=np.float64).squeeze().reshape(-1)
    std = np.asarray(std_target, dtype=np.float64).squeeze().reshape(-1)
    if mean.size != 2 or std.size != 2:
        raise DsxError("mean_target and std_target must hold one value per channel (two channels)")
    if not (np.isfinite(mean).all() and np.isfinite(std).all()) or (std == 0).any():
        raise DsxError("mean_target / std_target must be finite with non-zero std")
    n = int(n_timesteps)
    if not 1 <= n <= 1024:
        raise DsxError(f"n_timesteps = {n_timesteps}, must be in 1..1024")
    _lib.require_gpu()
    dev = data_dict[0].device if torch.is_tensor(data_dict[0]) and data_dict[0].is_cuda else torch.device(device)
    f0, f1 = _frames(data_dict[0], dev), _frames(data_dict[1], dev)
    if f0.shape != f1.shape or f0.numel() == 0:
        raise DsxError(f"the two channels must hold the same, non-empty frames (got {tuple(f0.shape)}, {tuple(f1.shape)})")
    pixels = f0.numel()
    rows = check(lib.dsx_mix_range_blocks(pixels, n))
    part = torch.empty((rows, n + 1, 2), dtype=torch.float64, device=dev)
    out = np.empty((n + 1, 2), dtype=np.float64)
    norm = (C.c_double * 4)(mean[0], std[0], mean[1], std[1])
    check(lib.dsx_mix_range(f0, f1, pixels, norm, n, part, out.ctypes.data_as(C.POINTER(C.c_double)), None))
    return {t_int: [out[t_int, 0], out[t_int, 1]] for t_int in range(n + 1)}


class TimePredictorDataset(SplitDataset):
    """:24-89.  ``__getitem__`` -> ``(inp (1, p, p) float32, t)``: t drawn by ``sample_t``, inp = t*patch1 +
    (1-t)*patch2 on the normalised patches, min-max-normalised with row t_int of ``input_normalization_dict``.

    The item is the float32 chain of include/dsx.h (dsx_tiles_gather_mix, channel 1).  That is the reference's own
    arithmetic under numpy 1.x (its environment); under numpy 2 ``img - np.float64(...)`` promotes and the reference's
    normalisation step runs in float64 -- the engine returns the float32 chain in both cases."""
    _COLOUR_REFUSAL = "the TimePredictor's mixed inputs (dsx_mix_range, dsx_tiles_gather_mix) take two grey channels"

    def __init__(self, *args, **kwargs):
        kwargs.pop("step_size", None)                                # accepted and unused, as in the reference (:26-29)
        if kwargs.pop("gaussian_noise_std_factor", None) is not None:
            raise DsxError("gaussian_noise_std_factor is training-time augmentation: out of scope")
        bound = inspect.signature(SplitDataset.__init__).bind(self, *args, **kwargs)
        if bound.arguments.get("uncorrelated_channels", False):
            raise DsxError("uncorrelated_channels draws a second random frame per item: training-time only")
        super().__init__(*args, **kwargs)
        self._num_timesteps = 100
        self.input_normalization_dict = compute_input_normalization_dict(self._data_dict, self._num_timesteps,
                                                                         self._mean_target, self._std_target)

    def sample_t(self):                                              # :42-44
        t_int = np.random.randint(0, self._num_timesteps)
        return t_int / self._num_timesteps, t_int

    def min_max_normalize(self, img, t_int):                         # :46-48 (host arrays, as the reference's)
        t_min, t_max = self.input_normalization_dict[t_int]
        return 2 * (img - t_min) / (t_max - t_min) - 1

    def __getitem__(self, index):                                    # :50-89
        loc = self._get_location(index)
        t, t_int = self.sample_t()
        lo, hi = self.input_normalization_dict[t_int]
        out = self.mixed_tiles_at([loc], t, (lo, hi, lo, hi), want=("cls",))
        return out["cls"][0, 1:2].cpu().numpy(), t

    def batch(self, indices, t_ints=None):
        """The items of ``indices`` as one batch -> ``(inp (B, 1, p, p) float32 on the device, t (B,) float64 numpy)``,
        cut by ONE launch (dsx_tiles_gather_mix_items: every item its own t and its own table row).  Item k is bitwise
        ``self[indices[k]]`` for the same draw.

        ``t_ints`` None: location and ``sample_t()`` per index, in index order -- the ``np.random`` call sequence of
        ``[self[i] for i in indices]``, so a seeded run draws the same values.  ``t_ints`` given: no random number is
        consumed for t; each value must be an integer in 0..num_timesteps-1."""
        self._grey_only("batch")
        _lib.require_gpu()
        indices = [int(i) for i in indices]
        n = self._num_timesteps
        if t_ints is not None:
            given = list(t_ints)
            if len(given) != len(indices):
                raise DsxError(f"t_ints holds {len(given)} values for {len(indices)} indices")
            for k, v in enumerate(given):
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < n:
                    raise DsxError(f"t_ints[{k}] = {v!r}: an integer in 0..{n - 1}")
        locs, ts, rows = [], [], []
        for k, index in enumerate(indices):
            locs.append(self._get_location(index))
            t, t_int = self.sample_t() if t_ints is None else (int(given[k]) / n, int(given[k]))
            ts.append(t)
            rows.append(t_int)
        b, p, dev = len(indices), self._patch_size, self._dev[0].device
        t = np.array(ts, dtype=np.float64).reshape(b)
        cls = torch.empty((b, 2, p, p), dtype=torch.float32, device=dev)
        if b:
            loc = np.ascontiguousarray(np.asarray(locs, dtype=np.int64).reshape(b, 3))
            lohi = np.array([self.input_normalization_dict[r] * 2 for r in rows], dtype=np.float64).reshape(b, 4)
            i64 = lambda v: (C.c_int64 * 3)(*[int(x) for x in v])
            pd = C.POINTER(C.c_double)
            check(lib.dsx_tiles_gather_mix_items(
                self._dev[0], self._dev[1], i64(self._data_shape), i64((1, p, p)),
                loc.ctypes.data_as(C.POINTER(C.c_int64)), b, self._norm4(), t.ctypes.data_as(pd), lohi.ctypes.data_as(pd),
                None, None, cls, None))
        return cls[:, 1:2].contiguous(), t
