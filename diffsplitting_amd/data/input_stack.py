"""An INPUT-ONLY stack as a tiled-prediction dataset: one (N,H,W) acquisition in which the two structures are already
superimposed -- no ground truth, nothing to build the network input from.  ``InputStackTiledPred`` mirrors the members
of ``SplitDatasetTiledPred`` (split_dataset.py) that the prediction path uses: ``plan``, ``tile_manager``, ``__len__``,
``tiles(ids) -> {'input': (b,1,p,p)}``, ``__getitem__`` (numpy), ``get_normalization_dict()``, ``_target_channel_idx``.

The normalisation comes from elsewhere (``data/normalization.py``: the training set's dict as a file).  uint8 / uint16
stacks are uploaded and STAY resident in their file width -- no fp32 copy of the stack exists -- and a batch of normalised
tiles is one launch of dsx_tileplan_gather_input, which widens, clips and normalises while it cuts.  On a stack that
holds w0 * ch0 + w1 * ch1 of a two-channel set the tiles are that set's 'input' bit for bit."""
import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib
from .tiling import TilePlan, as_sequence
from .tiling_manager import TileIndexManager, TilingMode

_PIX = {np.dtype(np.uint8): _lib.PIX_U8, np.dtype(np.uint16): _lib.PIX_U16, np.dtype(np.float32): _lib.PIX_F32}
ITEMS_PER_CALL = 65535                                              # dsx_tileplan_gather_input's limit


def read_stack(frames):
    """``frames``: an (N,H,W) array or a ``.tif`` / ``.npy`` path -> the contiguous (N,H,W) host array in its own
    pixel type (uint8 / uint16 / float32); every refusal that concerns the file, before anything touches the device."""
    name = None
    if isinstance(frames, (str, bytes)) or hasattr(frames, "__fspath__"):
        from .split_dataset import _read
        name = str(frames)
        frames = _read(name)
    what = f"{name}: " if name else ""
    a = np.asarray(frames)
    if a.ndim == 4 and a.shape[-1] == 2:
        raise DsxError(f"{what}the stack holds {a.shape}: two ground-truth channels (N,H,W,2), not one superimposed "
                       "acquisition (N,H,W); give such a file to --frames (SplitDatasetTiledPred) instead")
    if a.ndim != 3 or a.size == 0:
        raise DsxError(f"{what}an input-only stack is (N,H,W), got {a.shape}")
    if a.dtype not in _PIX:
        raise DsxError(f"{what}pixel type {a.dtype}: an input-only stack holds uint8, uint16 or float32 pixels")
    return np.ascontiguousarray(a)


class InputStackTiledPred:
    def __init__(self, frames, patch_size, normalization_dict, grid_size=None, target_channel_idx=None,
                 input_clip=None, device="cuda"):
        host = read_stack(frames)
        for k in ("mean_input", "std_input", "mean_target", "std_target"):
            if normalization_dict is None or k not in normalization_dict:
                raise DsxError(f"InputStackTiledPred: the normalisation dict must provide {k!r} (an input-only stack has "
                               "no channels to compute it from: data/normalization.py)")
        self._nd = dict(normalization_dict)
        self._mean_inp, self._std_inp = float(self._nd["mean_input"]), float(self._nd["std_input"])
        if not (np.isfinite(self._mean_inp) and np.isfinite(self._std_inp) and self._std_inp > 0):
            raise DsxError(f"InputStackTiledPred: mean_input = {self._mean_inp}, std_input = {self._std_inp}: finite, with "
                           "a positive std")
        if input_clip is not None and not (np.isfinite(input_clip) and input_clip >= 0):
            raise DsxError(f"InputStackTiledPred: input_clip = {input_clip}: a finite, non-negative count (None: no clip)")
        self._input_clip = None if input_clip is None else float(input_clip)
        self._target_channel_idx = target_channel_idx
        self._patch_size = int(patch_size)
        if grid_size is None:
            grid_size = self._patch_size // 2                       # as SplitDatasetTiledPred
        self._frameN, H, W = host.shape
        self._data_shape = tuple(host.shape)
        self._pix = _PIX[host.dtype]
        self.dtype = host.dtype
        patch_shape, grid_shape = (1, self._patch_size, self._patch_size), (1, int(grid_size), int(grid_size))
        self.tile_manager = TileIndexManager(self._data_shape, grid_shape, patch_shape, TilingMode.ShiftBoundary)
        self.plan = TilePlan(self._data_shape, grid_shape, patch_shape)
        _ = self.plan.handle                                        # a tiling that leaves the frames is refused here
        if torch.device(device).type == "cuda":
            _lib.require_gpu()
        # the stack in its file width: torch has no uint16 arithmetic, the bytes are all the kernel needs
        self._dev = torch.as_tensor(host.view(np.uint8) if host.dtype != np.float32 else host).to(torch.device(device))

    def __len__(self):
        return self.tile_manager.total_grid_count()

    def patch_location(self, index):
        return self.tile_manager.get_patch_location_from_dataset_idx(index)

    def get_normalization_dict(self):
        return dict(self._nd)

    @property
    def device(self):
        """The device the stack is resident on."""
        return self._dev.device

    def resident_bytes(self):
        """Device bytes the stack occupies (its file width: half of an fp32 copy for uint16, a quarter for uint8)."""
        return self._dev.numel() * self._dev.element_size()

    def acquisition(self):
        """What the data-consistency check (core/consistency.py) needs of the stack: ``(the resident bytes, their pixel
        type _lib.PIX_*, the (N,H,W) shape, input_clip or None)``.  Nothing is copied."""
        return self._dev, self._pix, self._data_shape, self._input_clip

    def _gather_seq(self, seq, out):
        first, stride, count = seq
        for k0 in range(0, count, ITEMS_PER_CALL):
            n = min(ITEMS_PER_CALL, count - k0)
            check(lib.dsx_tileplan_gather_input(self.plan.handle, self._dev, self._pix, first + k0 * stride, stride, n,
                                                self._mean_inp, self._std_inp,
                                                -1.0 if self._input_clip is None else self._input_clip, out[k0:], None))

    def tiles(self, indices):
        """Tile ids -> ``{'input': (b,1,p,p)}`` on the device.  A rank's shard or a batch of it is an arithmetic id
        sequence: one launch; any other list takes one launch per tile."""
        _lib.require_gpu()
        ids = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.plan.total):
            raise DsxError(f"tile id out of range (0..{self.plan.total - 1})")
        p = self._patch_size
        out = torch.empty((ids.size, 1, p, p), dtype=torch.float32, device=self._dev.device)
        seq = as_sequence(ids)
        if seq is not None:
            self._gather_seq(seq, out)
        else:
            for k, i in enumerate(ids):
                self._gather_seq((int(i), 1, 1), out[k:])
        return {"input": out}

    def __getitem__(self, index):
        return {"input": self.tiles([int(index)])["input"][0].cpu().numpy()}
