"""``data/split_dataset.py`` of the reference with the frames resident in HBM (§8f N2): same constructor arguments
and item format as ``SplitDataset`` (:93-278), normalisation statistics as ``compute_normalization_dict`` (:29-74)
computed on the device, and — what the tiled-prediction path actually wants — whole BATCHES of normalised tiles
cut by one HIP launch (``tiles(ids)`` -> dsx_tiles_gather_norm) instead of one host crop + host->device copy per
tile through a DataLoader(batch_size = 1) (data/__init__.py:16-18).

Not available here (and refused loudly): ``enable_transforms`` (albumentations).  ``.tif`` stacks are read by the
library's own reader (data/tiff.py: uncompressed TIFF / BigTIFF); uint8 / uint16 stacks go to the device in their file
width and are clipped and widened there (dsx_frames_to_f32).  ``data_type='cifar10'`` reads its pickle batches with
data/cifar10.py; its frames carry colour planes, (N, Cc, H, W) per class with Cc in 1..8 (also accepted through
``DataLocation(arrays=...)``), the items are {'input': (Cc, p, p), 'target': (2 Cc, p, p)} and a batch of them is one
launch of dsx_tiles_gather_norm_planes.  Grey (N, H, W) frames take the calls they always took.
Parity: the Hagen arithmetic of ``__getitem__`` is bit-exact against a numpy restatement of :237-278; the quantile of
``compute_normalization_dict`` is numpy's published linear-interpolation definition (checked against
``numpy.quantile``).  With empty stand-ins for albumentations / skimage the reference module imports, and its own
``SplitDataset('cifar10', ...)`` wrote tests/golden/cifar_items.npz (tools/gen_cifar_golden.py): loader, normalisation
dict and items are pinned bit for bit by the reference's code.  The Hagen items have no such fixture (beyond the
reference's known-answer test, tests/test_tiling_setup.py: identity normalisation, stitch(tiles(arange)) == arange).
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib
from .tiling import TilePlan, _i64x3
from .tiling_manager import TileIndexManager, TilingMode


@dataclass
class DataLocation:                                                 # split_dataset.py:10-18
    channelwise_fpath: Tuple[str] = ()
    fpath: str = ""
    directory: str = ""
    arrays: tuple = field(default=())                               # extension: (ch0, ch1) arrays already in memory

    def __post_init__(self):
        assert self.channelwise_fpath or self.fpath or self.directory or len(self.arrays), "no data location given"


def _read(path):
    if str(path).endswith(".npy"):
        return np.load(path, allow_pickle=False)
    if str(path).endswith((".tif", ".tiff")):
        from .tiff import imread
        return imread(path)
    raise DsxError(f"unsupported frame file {path} (.npy, .tif)")


MAX_PLANES = 8                                                      # colour planes per stack: half of VAL_MAX_CHANNELS
UPPER_CLIP = 1993.0                                                 # the reference's hard-coded upper clip (:80-82)
_NARROW = (np.dtype(np.uint8), np.dtype(np.uint16))                 # uploaded as they are, widened on the device


def _load(data_type, dataloc):
    """-> ({0: frames of channel 0 (N,H,W), 1: frames of channel 1}, clip).  ``clip`` is the upper clip that is still
    to be applied -- by dsx_frames_to_f32, on the device -- to channelwise uint8 / uint16 stacks, which keep their
    dtype; None when the frames are final.  'cifar10': (n_i, 3, 32, 32) uint8 per class, labels 1 and 7 (:20-22)."""
    if len(dataloc.arrays):
        return {0: np.asarray(dataloc.arrays[0]), 1: np.asarray(dataloc.arrays[1])}, None
    if data_type == "cifar10":
        if not dataloc.directory:
            raise DsxError("data_type 'cifar10' reads a directory of batch files: DataLocation(directory=...) or arrays")
        from .cifar10 import load_train_val_data
        data = load_train_val_data(dataloc.directory, [1, 7])
        return {0: data[0], 1: data[1]}, None
    if dataloc.fpath:
        data = _read(dataloc.fpath)                                 # (N,H,W,2), :85-91: no clip
        if data.ndim != 4 or data.shape[-1] < 2:
            raise DsxError(f"{dataloc.fpath}: (N,H,W,2) frames expected, got {data.shape}")
        return {0: data[..., 0], 1: data[..., 1]}, None
    assert len(dataloc.channelwise_fpath) == 2, "Only two channelwise fpaths are supported"
    raw = [_read(f) for f in dataloc.channelwise_fpath]
    is_tif = all(str(f).endswith((".tif", ".tiff")) for f in dataloc.channelwise_fpath)
    if is_tif and all(r.dtype in _NARROW for r in raw):               # .npy: float32 on the host, as ever
        return {0: raw[0], 1: raw[1]}, UPPER_CLIP
    ch0 = np.array(raw[0], dtype=np.float32, copy=True)
    ch1 = np.array(raw[1], dtype=np.float32, copy=True)
    ch0[ch0 > UPPER_CLIP] = UPPER_CLIP
    ch1[ch1 > UPPER_CLIP] = UPPER_CLIP
    return {0: ch0, 1: ch1}, None


def load_data(data_type, dataloc):
    """:20-27,76-91 -> {0: frames of channel 0 (N,H,W), 1: frames of channel 1}, on the host, the channelwise clip
    applied."""
    data, clip = _load(data_type, dataloc)
    if clip is not None:
        data = {c: np.minimum(v, v.dtype.type(clip)) for c, v in data.items()}
    return data


def frames_to_device(frames, dev, clip=None):
    """(N,H,W) or (N,Cc,H,W) host frames -> contiguous fp32 CUDA tensor.  uint8 / uint16 frames are uploaded in their own
    width and widened (and clipped at ``clip``) by dsx_frames_to_f32; the values equal the host conversion
    ``np.minimum(frames, clip).astype(np.float32)`` bit for bit (every uint16 is an fp32)."""
    frames = np.asarray(frames)
    if frames.dtype not in _NARROW or frames.size == 0 or torch.device(dev).type != "cuda":
        if clip is not None:
            frames = np.minimum(frames, clip)
        return torch.as_tensor(np.ascontiguousarray(frames, dtype=np.float32)).to(dev)
    _lib.require_gpu()
    src = torch.as_tensor(np.ascontiguousarray(frames).view(np.uint8)).to(dev)      # raw bytes: torch has no uint16 math
    dst = torch.empty(frames.shape, dtype=torch.float32, device=dev)
    check(lib.dsx_frames_to_f32(src, _lib.PIX_U16 if frames.dtype == np.uint16 else _lib.PIX_U8, frames.size,
                                -1.0 if clip is None else float(clip), dst, None))
    torch.cuda.current_stream(dst.device).synchronize()             # `src` is released on return
    return dst


def quantile_device(x, q):
    """numpy.quantile(x.astype(float64), q) (default linear interpolation) of a flat CUDA / CPU tensor: the two
    neighbouring order statistics come from a sort on the tensor's device, numpy interpolates between them.  This is
    what the reference computes on its integer-typed .tif frames (numpy promotes them to float64); for float32 input
    numpy 2.x would interpolate in float32 instead — the float64 value is used here in every case."""
    v = torch.sort(x.reshape(-1)).values
    pos = (v.numel() - 1) * float(q)
    lo = int(np.floor(pos))
    hi = min(lo + 1, v.numel() - 1)
    pair = torch.stack([v[lo], v[hi]]).to(torch.float64).cpu().numpy()
    return np.quantile(pair, pos - lo)              # np.float64, as numpy.quantile returns it (a "strong" scalar: the
                                                    # normalisation arithmetic that uses it runs in float64)


def order_stats_device(a, b, w0, w1, ranks):
    """The ``ranks``-th smallest (0-based) of (double)a, or of (double)a*w0 + (double)b*w1 with ``b``, over flat fp32
    CUDA tensors -> np.float64 array: dsx_order_stats, a radix select (no sort, no per-element temporary)."""
    _lib.require_gpu()
    a = a.reshape(-1).contiguous()
    b = None if b is None else b.reshape(-1).contiguous()
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    out = np.empty(ranks.size, dtype=np.float64)
    ws = torch.empty(int(lib.dsx_order_stats_workspace_bytes(a.numel(), ranks.size)), dtype=torch.uint8, device=a.device)
    check(lib.dsx_order_stats(a, b, a.numel(), float(w0), float(w1), ranks.ctypes.data_as(C.POINTER(C.c_int64)),
                              ranks.size, out.ctypes.data_as(C.POINTER(C.c_double)), ws, None))
    return out


def quantile_select(a, b, w0, w1, q):
    """``quantile_device`` of the key of ``order_stats_device`` without the sort: the two neighbouring order statistics
    by radix select, the same interpolation expression."""
    n = a.numel()
    pos = (n - 1) * float(q)
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    return np.quantile(order_stats_device(a, b, w0, w1, [lo, hi]), pos - lo)


def compute_normalization_dict(data_dict, channel_weights, q_val=1.0, uint8_data=False):
    """:29-74.  ``data_dict`` values may be numpy arrays or torch tensors.  fp32 CUDA tensors take the radix select
    (dsx_order_stats); CPU tensors and other dtypes the sort of ``quantile_device``: the same values.
    Departure from the reference: the key of ``input_max`` is always float64 (channel * weight + channel * weight, each
    operation rounded once); where the reference's uint16 sum would wrap (unclipped ``fpath`` data with integer
    weights) it does not wrap here."""
    if uint8_data:
        tar_max = 255
        inp_max = tar_max * np.sum(channel_weights)
        img_shape = data_dict[0][0].shape
        nC = 1 if len(img_shape) == 2 else img_shape[0]
        return {"mean_input": inp_max / 2, "std_input": inp_max / 2,
                "mean_target": np.array([tar_max / 2] * nC + [tar_max / 2] * nC),
                "std_target": np.array([tar_max / 2] * nC + [tar_max / 2] * nC),
                "target0_max": tar_max, "target1_max": tar_max, "input_max": inp_max}
    t1 = torch.as_tensor(data_dict[0]).reshape(-1)
    t2 = torch.as_tensor(data_dict[1]).reshape(-1)
    if t1.is_cuda and t2.is_cuda and t1.dtype == t2.dtype == torch.float32 and t1.numel() == t2.numel():
        w0, w1 = float(channel_weights[0]), float(channel_weights[1])
        tar1_max = quantile_select(t1, None, 1.0, 0.0, q_val)
        tar2_max = quantile_select(t2, None, 1.0, 0.0, q_val)
        inp_max = quantile_select(t1, t2, w0, w1, q_val)
        return {"mean_input": inp_max / 2, "std_input": inp_max / 2,
                "mean_target": np.array([tar1_max / 2, tar2_max / 2]), "std_target": np.array([tar1_max / 2, tar2_max / 2]),
                "target0_max": tar1_max, "target1_max": tar2_max, "input_max": inp_max}
    tar1_max = quantile_device(t1, q_val)
    tar2_max = quantile_device(t2, q_val)
    inp_max = quantile_device(t1.to(torch.float64) * channel_weights[0] + t2.to(torch.float64) * channel_weights[1], q_val)
    return {"mean_input": inp_max / 2, "std_input": inp_max / 2,
            "mean_target": np.array([tar1_max / 2, tar2_max / 2]), "std_target": np.array([tar1_max / 2, tar2_max / 2]),
            "target0_max": tar1_max, "target1_max": tar2_max, "input_max": inp_max}


def table_rows(table, mixing_t):
    """(lo0, hi0, lo1, hi1): the rows of the range table ``{t_int: [min, max]}`` (n + 1 rows) that normalise the two
    mix channels at ``mixing_t`` -- row int((1 - t) * n) for indi1's input, int(t * n) for indi2's (normalize_indi1/2,
    notebooks/EvaluateJointIndiIterative.ipynb cell 40).  Python's ``int`` truncates (int(0.29 * 100) == 28): kept."""
    if table is None:
        return None
    n = len(table) - 1
    r0, r1 = int((1 - mixing_t) * n), int(mixing_t * n)
    if not (0 <= r0 <= n and 0 <= r1 <= n):
        raise DsxError(f"mixing_t = {mixing_t} selects rows {r0}, {r1} outside the table (0..{n})")
    return (table[r0][0], table[r0][1], table[r1][0], table[r1][1])


class SplitDataset:
    """Constructor arguments of the reference (:94-103).  Frames live on the GPU as two fp32 tensors, (N,H,W) or, with
    colour planes, (N,Cc,H,W)."""
    _COLOUR_REFUSAL = None                                          # subclasses that are grey-only say why

    def __init__(self, data_type, data_location, patch_size, target_channel_idx=None, random_patching=False,
                 enable_transforms=False, max_qval=0.98, normalization_dict=None, uncorrelated_channels=False,
                 channel_weights=None, input_from_normalized_target=False, upper_clip=False, device="cuda"):
        assert data_type in ["cifar10", "Hagen"], "data_type must be one of ['cifar10','Hagen']"
        if enable_transforms:
            raise DsxError("enable_transforms needs albumentations (training-time augmentation): out of scope")
        self._patch_size = patch_size
        self._data_location = data_location
        self._channel_weights = channel_weights if channel_weights is not None else [1, 1]
        self._input_from_normalized_target = input_from_normalized_target
        data, clip = _load(data_type, data_location)
        self._planes = self._check_frames(data)                     # None: grey (N,H,W) frames
        self._frameN = min(len(data[0]), len(data[1]))
        self._target_channel_idx = target_channel_idx
        self._random_patching = random_patching
        self._uncorrelated_channels = uncorrelated_channels
        self._max_qval = max_qval
        self._transform = None
        dev = torch.device(device)
        self._dev = [frames_to_device(data[c][:self._frameN], dev, clip) for c in (0, 1)]
        if normalization_dict is None:
            normalization_dict = compute_normalization_dict({0: self._dev[0], 1: self._dev[1]}, self._channel_weights,
                                                            q_val=self._max_qval, uint8_data=data_type == "cifar10")
        if upper_clip:                                              # :147-150
            self._dev[0] = self._dev[0].clamp(0, float(normalization_dict["target0_max"]))
            self._dev[1] = self._dev[1].clamp(0, float(normalization_dict["target1_max"]))
        for k in ("mean_input", "std_input", "mean_target", "std_target"):
            assert k in normalization_dict, f"{k} must be provided"
        self._mean_inp = normalization_dict["mean_input"]
        self._std_inp = normalization_dict["std_input"]
        self._mean_target = np.asarray(normalization_dict["mean_target"]).reshape(-1, 1, 1)
        self._std_target = np.asarray(normalization_dict["std_target"]).reshape(-1, 1, 1)
        self._target0_max = normalization_dict.get("target0_max")
        self._target1_max = normalization_dict.get("target1_max")
        self._input_max = normalization_dict.get("input_max")
        self._data_shape = tuple(self._dev[0].shape)
        if self._planes and not self._mean_target.size == self._std_target.size == 2 * self._planes:
            raise DsxError(f"frames with {self._planes} colour planes need {2 * self._planes} mean_target / std_target "
                           f"values (one per target plane), got {self._mean_target.size} / {self._std_target.size}")

    def _check_frames(self, data):
        """The colour-plane count Cc of (N,Cc,H,W) frames, None for (N,H,W) ones; every refusal that concerns the
        frames' shape, on the host arrays (nothing is on the device yet)."""
        a, b = data[0], data[1]
        if a.ndim != b.ndim or a.shape[1:] != b.shape[1:] or a.ndim not in (3, 4):
            raise DsxError(f"the two channels must hold (N,H,W) or (N,Cc,H,W) frames of one shape, got {a.shape} and {b.shape}")
        if a.ndim == 3:
            return None
        planes = a.shape[1]
        if not 1 <= planes <= MAX_PLANES:
            raise DsxError(f"(N,Cc,H,W) frames with Cc = {planes} colour planes: 1..{MAX_PLANES}")
        if self._COLOUR_REFUSAL:
            raise DsxError(f"{type(self).__name__} on frames with colour planes {a.shape}: {self._COLOUR_REFUSAL}")
        if self._input_from_normalized_target and planes > 1:
            raise DsxError("input_from_normalized_target with colour planes: the reference mixes target[0:1] and "
                           "target[1:2], which are planes 0 and 1 of the FIRST image once an image has more than one "
                           "plane -- a grey-data assumption (joint_indi); no configuration pairs it with colour data")
        return planes

    def get_normalization_dict(self):                               # :185-194
        return {"mean_input": self._mean_inp, "std_input": self._std_inp, "mean_target": self._mean_target,
                "std_target": self._std_target, "target0_max": self._target0_max, "target1_max": self._target1_max,
                "input_max": self._input_max}

    @property
    def device(self):
        """The one device both channels' frames are resident on."""
        return self._dev[0].device

    def normalize_inp(self, inp):                                   # :195-197
        return ((inp - self._mean_inp) / self._std_inp).astype(np.float32)

    def normalize_target(self, target):                             # :199-201
        return ((target - self._mean_target) / self._std_target).astype(np.float32)

    def patch_count_per_frame(self):                                # :203-206
        h, w = self._data_shape[-2:]
        return (h // self._patch_size) * (w // self._patch_size)

    def __len__(self):
        return self._frameN * self.patch_count_per_frame()

    def frame_idx(self, index):
        return index // self.patch_count_per_frame()

    def patch_location(self, index):                                # :215-225
        frame_idx = self.frame_idx(index)
        index = index % self.patch_count_per_frame()
        h, w = self._data_shape[-2:]
        h_idx = index // (h // self._patch_size)
        w_idx = index % (w // self._patch_size)
        return frame_idx, h_idx * self._patch_size, w_idx * self._patch_size

    def _get_location(self, index):                                 # :228-236
        if self._random_patching:
            frame_idx = np.random.randint(0, self._frameN)
            h, w = self._data_shape[-2:]
            h_idx = np.random.randint(0, h - self._patch_size) if h > self._patch_size else 0
            w_idx = np.random.randint(0, w - self._patch_size) if w > self._patch_size else 0
            return frame_idx, h_idx, w_idx
        return self.patch_location(index)

    # ---- the device path: a batch of normalised tiles in one launch ------------------------------------
    def _norm6(self):
        mt, st = self._mean_target.reshape(-1), self._std_target.reshape(-1)
        return (C.c_double * 6)(float(self._mean_inp), float(self._std_inp), float(mt[0]), float(st[0]), float(mt[-1]), float(st[-1]))

    def tiles_at(self, locations):
        """``locations``: (b, 3) integer (frame, y, x) top-left corners -> {'input': (b,1,p,p), 'target': (b,2,p,p)}
        CUDA tensors, normalised exactly as ``__getitem__`` does, in one HIP launch."""
        _lib.require_gpu()
        loc = np.ascontiguousarray(np.asarray(locations, dtype=np.int64).reshape(-1, 3))
        if self._planes and not self._input_from_normalized_target:
            return self._plane_tiles_at(loc)
        b, p = loc.shape[0], self._patch_size
        dev = self._dev[0].device
        tin = torch.empty((b, 1, p, p), dtype=torch.float32, device=dev)
        ttar = torch.empty((b, 2, p, p), dtype=torch.float32, device=dev)
        shape3 = (self._data_shape[0],) + self._data_shape[-2:]      # (N,1,H,W) frames are (N,H,W) frames
        check(lib.dsx_tiles_gather_norm(self._dev[0], self._dev[1], _i64x3(shape3), _i64x3((1, p, p)),
                                        loc.ctypes.data_as(C.POINTER(C.c_int64)), None, b,
                                        float(self._channel_weights[0]), float(self._channel_weights[1]), self._norm6(),
                                        1 if self._input_from_normalized_target else 0, tin, ttar, None))
        if self._target_channel_idx is not None:
            ttar = ttar[:, self._target_channel_idx:self._target_channel_idx + 1].contiguous()
        return {"input": tin, "target": ttar}

    PLANE_ITEMS_PER_CALL = 65535                                    # dsx_tiles_gather_norm_planes' limit

    def _plane_tiles_at(self, loc):
        """``tiles_at`` for (N,Cc,H,W) frames -> {'input': (b,Cc,p,p), 'target': (b,2Cc,p,p)}: one launch of
        dsx_tiles_gather_norm_planes per 65535 items."""
        b, p, cc = loc.shape[0], self._patch_size, self._planes
        dev = self._dev[0].device
        tin = torch.empty((b, cc, p, p), dtype=torch.float32, device=dev)
        ttar = torch.empty((b, 2 * cc, p, p), dtype=torch.float32, device=dev)
        pd = C.POINTER(C.c_double)
        mt = np.ascontiguousarray(self._mean_target.reshape(-1), dtype=np.float64)
        st = np.ascontiguousarray(self._std_target.reshape(-1), dtype=np.float64)
        shape, patch = (C.c_int64 * 4)(*[int(x) for x in self._data_shape]), (C.c_int64 * 2)(p, p)
        for i0 in range(0, b, self.PLANE_ITEMS_PER_CALL):
            part = np.ascontiguousarray(loc[i0:i0 + self.PLANE_ITEMS_PER_CALL])
            check(lib.dsx_tiles_gather_norm_planes(
                self._dev[0], self._dev[1], shape, patch, part.ctypes.data_as(C.POINTER(C.c_int64)), None, part.shape[0],
                float(self._channel_weights[0]), float(self._channel_weights[1]), float(self._mean_inp),
                float(self._std_inp), mt.ctypes.data_as(pd), st.ctypes.data_as(pd), tin[i0:], ttar[i0:], None))
        if self._target_channel_idx is not None:
            ttar = ttar[:, self._target_channel_idx:self._target_channel_idx + 1].contiguous()
        return {"input": tin, "target": ttar}

    def tiles(self, indices):
        """Dataset indices -> the batch of their items on the device."""
        if self._uncorrelated_channels:
            raise DsxError("uncorrelated_channels draws a second random frame per item: training-time only")
        return self.tiles_at([self._get_location(int(i)) for i in indices])

    # ---- mixed inputs of the TimePredictor evaluation (dsx_tiles_gather_mix) -----------------------------
    @property
    def _data_dict(self):
        """{0: frames of channel 0, 1: frames of channel 1} as the reference's attribute of this name (:126), here the
        device tensors: what ``compute_input_normalization_dict(val_set._data_dict, ...)`` is given."""
        return {0: self._dev[0], 1: self._dev[1]}

    def _norm4(self):
        mt, st = self._mean_target.reshape(-1), self._std_target.reshape(-1)
        return (C.c_double * 4)(float(mt[0]), float(st[0]), float(mt[-1]), float(st[-1]))

    def _grey_only(self, what):
        if self._planes:
            raise DsxError(f"{what} on frames with colour planes {self._data_shape}: the mixed-input kernels "
                           "(dsx_tiles_gather_mix) take two grey channels")

    def _mixed_new(self, count, lohi, want):
        p, dev = self._patch_size, self._dev[0].device
        want = tuple(want) if want is not None else ("target", "mix") + (("cls",) if lohi is not None else ())
        if "cls" in want and lohi is None:
            raise DsxError("the classifier view ('cls') needs the range table")
        out = {k: torch.empty((count, 2, p, p), dtype=torch.float32, device=dev) for k in ("target", "mix", "cls") if k in want}
        if not out:
            raise DsxError("mixed_tiles: nothing asked for (want = target, mix, cls)")
        return out, (C.c_double * 4)(*[float(v) for v in lohi]) if "cls" in out else None

    def mixed_tiles_at(self, locations, mixing_t, lohi=None, want=None):
        """``locations``: (b, 3) (frame, y, x) corners -> {'target', 'mix', 'cls'} (b, 2, p, p) CUDA tensors in one HIP
        launch (op list: include/dsx.h, dsx_tiles_gather_mix).  ``lohi`` = (lo0, hi0, lo1, hi1), the (min, max) rows of
        the range table that normalise the two mix channels for the classifier; without it there is no 'cls'."""
        self._grey_only("mixed_tiles_at")
        _lib.require_gpu()
        loc = np.ascontiguousarray(np.asarray(locations, dtype=np.int64).reshape(-1, 3))
        b, p = loc.shape[0], self._patch_size
        out, lh = self._mixed_new(b, lohi, want)
        check(lib.dsx_tiles_gather_mix(self._dev[0], self._dev[1], _i64x3(self._data_shape), _i64x3((1, p, p)),
                                       loc.ctypes.data_as(C.POINTER(C.c_int64)), None, b, self._norm4(), float(mixing_t), lh,
                                       out.get("target"), out.get("mix"), out.get("cls"), None))
        return out

    def mixed_tiles(self, indices, mixing_t, table=None, want=None):
        """Dataset indices -> the mixed inputs of their tiles at mixing weight ``mixing_t`` (get_inputs,
        notebooks/EvaluateJointIndiIterative.ipynb cell 40): 'target' (as ``tiles``), 'mix' (channel 0 =
        t0*(1-t) + t1*t for indi1, channel 1 = t1*(1-t) + t0*t for indi2) and, with ``table`` (what
        ``compute_input_normalization_dict`` returns), 'cls': the two mix channels min-max-normalised for the
        classifier with the rows int((1-t)*n) and int(t*n) (normalize_indi1/2; ``int`` truncates, as there)."""
        self._grey_only("mixed_tiles")
        if self._uncorrelated_channels:
            raise DsxError("uncorrelated_channels draws a second random frame per item: training-time only")
        return self.mixed_tiles_at([self._get_location(int(i)) for i in indices], mixing_t, table_rows(table, mixing_t), want)

    def __getitem__(self, index):                                   # :237-278 (numpy, as the reference returns it)
        out = self.tiles([index])
        item = {k: v[0].cpu().numpy() for k, v in out.items()}
        return item


class SplitDatasetTiledPred(SplitDataset):
    """data/split_dataset_tiledpred.py:9-32: the dataset whose index is a tile of the ShiftBoundary tiling."""
    _COLOUR_REFUSAL = "the tile plan (TilePlan, TileIndexManager) is three-dimensional, (N,H,W); colour items are not tiled"

    def __init__(self, *args, **kwargs):
        grid_size = kwargs.pop("grid_size", None)
        super().__init__(*args, **kwargs)
        if grid_size is None:
            grid_size = self._patch_size // 2
        _, H, W = self._data_shape
        patch_shape, grid_shape = (1, self._patch_size, self._patch_size), (1, grid_size, grid_size)
        self.tile_manager = TileIndexManager((self._frameN, H, W), grid_shape, patch_shape, TilingMode.ShiftBoundary)
        self.plan = TilePlan((self._frameN, H, W), grid_shape, patch_shape)

    def __len__(self):
        return self.tile_manager.total_grid_count()

    def patch_location(self, index):
        return self.tile_manager.get_patch_location_from_dataset_idx(index)

    def _gather_norm_seq(self, plan, seq):
        """One launch of the fused crop + normalisation over the tiles ``first + k * stride`` of ``plan`` (its device
        tables are indexed by tile id: nothing is uploaded per call)."""
        _lib.require_gpu()
        first, stride, count = seq
        ph, pw = plan.patch_shape[1:]
        dev = self._dev[0].device
        tin = torch.empty((count, 1, ph, pw), dtype=torch.float32, device=dev)
        ttar = torch.empty((count, 2, ph, pw), dtype=torch.float32, device=dev)
        if count:
            check(lib.dsx_tileplan_gather_norm(plan.handle, self._dev[0], self._dev[1], first, stride, count,
                                               float(self._channel_weights[0]), float(self._channel_weights[1]),
                                               self._norm6(), 1 if self._input_from_normalized_target else 0,
                                               tin, ttar, None))
        if self._target_channel_idx is not None:
            ttar = ttar[:, self._target_channel_idx:self._target_channel_idx + 1].contiguous()
        return {"input": tin, "target": ttar}

    def tiles(self, indices):
        """Dataset indices (= tile ids) -> the batch of their items on the device.  A rank's shard or a batch of it is an
        arithmetic id sequence and goes through the plan's device tables; other index lists through ``tiles_at``."""
        from .tiling import as_sequence
        seq = as_sequence(indices)
        if seq is None or self._random_patching or self._uncorrelated_channels:
            return super().tiles(indices)
        return self._gather_norm_seq(self.plan, seq)

    def mixed_tiles(self, indices, mixing_t, table=None, want=None):
        """As ``SplitDataset.mixed_tiles`` for tile ids; an arithmetic id sequence goes through the plan's device
        tables (dsx_tileplan_gather_mix: nothing is uploaded per call), other index lists through ``mixed_tiles_at``."""
        from .tiling import as_sequence
        seq = as_sequence(indices)
        if seq is None or self._random_patching or self._uncorrelated_channels:
            return super().mixed_tiles(indices, mixing_t, table, want)
        _lib.require_gpu()
        first, stride, count = seq
        out, lh = self._mixed_new(count, table_rows(table, mixing_t), want)
        if count:
            check(lib.dsx_tileplan_gather_mix(self.plan.handle, self._dev[0], self._dev[1], first, stride, count,
                                              self._norm4(), float(mixing_t), lh, out.get("target"), out.get("mix"),
                                              out.get("cls"), None))
        return out

    def normalized_target_frames(self):
        """The normalised target channels of every frame, (N, H, W, C) on the device: the ground truth the stitched
        prediction is scored against.  Every rank holds the frames, so this needs no tiles and no collective: the same
        fused kernel with one whole-frame tile per frame."""
        _, H, W = self._data_shape
        whole = TilePlan((self._frameN, H, W), (1, H, W), (1, H, W))
        tar = self._gather_norm_seq(whole, (0, 1, self._frameN))["target"]          # (N, C, H, W)
        return tar.permute(0, 2, 3, 1).contiguous()
