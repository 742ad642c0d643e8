"""Tile planning, device-side tile gather and stitch (C ABI: dsx_tile_plan,
dsx_tile_regions, dsx_tiles_gather, dsx_stitch)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib
from ..core.psnr import range_invariant_psnr_from_sums

TRIM, PAD, SHIFT = _lib.TILING_TRIM, _lib.TILING_PAD, _lib.TILING_SHIFT
PSNR_MAX_CHANNELS = 4      # kPsnrMaxC (csrc/dsx_kernels.h): channels of a paste or blend that takes the PSNR sums


def _i64x3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def as_sequence(ids):
    """(first, stride, count) if ``ids`` is an arithmetic sequence with a positive stride (a rank's shard or a batch of
    it), else None."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size == 0:
        return 0, 1, 0
    if ids.size == 1:
        return int(ids[0]), 1, 1
    d = int(ids[1] - ids[0])
    if d < 1 or np.any(np.diff(ids) != d):
        return None
    return int(ids[0]), d, int(ids.size)


def _per_sequence(ids, call, out):
    """``call(first, stride, count, dst)`` over the id list ``ids``, rows of ``out`` in its order: an arithmetic sequence
    in launches of at most 65535 tiles (a grid dimension), any other list one tile per launch.  -> ``out``"""
    seq = as_sequence(ids)
    if seq is not None:
        for k0 in range(0, seq[2], 65535):
            call(seq[0] + k0 * seq[1], seq[1], min(65535, seq[2] - k0), out[k0:])
    else:
        for k, i in enumerate(ids):
            call(int(i), 1, 1, out[k:])
    return out


WINDOWS = ("triangle", "hann")


def window(name, n):
    """The 1-D blend window ``name`` over ``n`` pixels, float32, every value > 0.  ``"triangle"``: min(i + 1, n - i),
    integers, so the products of two of them are exact in fp32 up to n = 512.  ``"hann"``: sin^2(pi (i + 1/2) / n),
    computed in float64 and rounded to fp32 once."""
    n = int(n)
    if n < 1:
        raise DsxError(f"window: n = {n}, must be at least 1")
    i = np.arange(n, dtype=np.float64)
    if name == "triangle":
        return np.minimum(i + 1, n - i).astype(np.float32)
    if name == "hann":
        return (np.sin(np.pi * (i + 0.5) / n) ** 2).astype(np.float32)
    raise DsxError(f"window: {name!r} is not a window; one of {', '.join(WINDOWS)}")


def _rms_pair(sum_var, count):
    """sqrt(2 * sum_var / count): the RMS difference over all pairs of contributors; NaN where the count is 0"""
    return torch.where(count > 0, torch.sqrt(2.0 * sum_var / count.to(torch.float64)),
                       torch.full_like(sum_var, float("nan")))


def disagreement_from_partials(part):
    """The rows of ``dsx_tileplan_disagreement``, (N, blocks, C, 8) float64, folded over the workgroups the way
    ``TilePlan.psnr_from_partials`` folds its rows -> ``count`` (N,C,2) int64, ``sum_var`` (N,C,2), ``min_var`` and
    ``max_var`` (N,C), ``rms_pair`` (N,C,2); index 0 of the pairs is the overlap (two or more contributors), 1 the band."""
    s = part[..., :4].sum(dim=1)                                     # fixed order: reproducible
    count = s[..., 0::2].round().to(torch.int64)
    sum_var = s[..., 1::2].contiguous()
    return dict(count=count, sum_var=sum_var, min_var=part[..., 4].amin(dim=1), max_var=part[..., 5].amax(dim=1),
                rms_pair=_rms_pair(sum_var, count))


def fold_disagreement(a, b):
    """The scores of two measurements of one plan (two posterior samples) as one: counts and sums added, ``a`` first,
    min / max folded, ``rms_pair`` from the totals; maps and rows are not carried.  ``a`` None: ``b``'s scores."""
    if a is None:
        return {k: b[k] for k in ("count", "sum_var", "min_var", "max_var", "rms_pair")}
    count, sum_var = a["count"] + b["count"], a["sum_var"] + b["sum_var"]
    return dict(count=count, sum_var=sum_var, min_var=torch.minimum(a["min_var"], b["min_var"]),
                max_var=torch.maximum(a["max_var"], b["max_var"]), rms_pair=_rms_pair(sum_var, count))


class TilePlan:
    """All tiles of data (N,H,W) for a (1,g,g) grid and (1,p,p) patches —
    what ``SplitDatasetTiledPred.__init__`` sets up (split_dataset_tiledpred.py:9-24).
    Host-only integer math in the library; works without a GPU.

    The device methods go through a ``dsx_tileplan`` handle: the patch starts and valid regions of every tile are
    uploaded once, calls name their tiles as an arithmetic id sequence (``ids`` of a shard or batch), nothing is
    allocated, copied or synchronised per call.  Arbitrary id lists fall back to the per-call upload forms."""

    def __init__(self, data_shape, grid_shape, patch_shape, mode=SHIFT):
        if not (len(data_shape) == len(grid_shape) == len(patch_shape) == 3):
            raise DsxError("TilePlan handles 3-D data (N,H,W)")
        self.data_shape = tuple(int(v) for v in data_shape)
        self.grid_shape = tuple(int(v) for v in grid_shape)
        self.patch_shape = tuple(int(v) for v in patch_shape)
        self.mode = mode
        ds, gs, ps = _i64x3(data_shape), _i64x3(grid_shape), _i64x3(patch_shape)
        n = check(lib.dsx_tile_plan(ds, gs, ps, mode, None, None, 0))
        self.total = int(n)
        self.grid_start = np.zeros((self.total, 3), dtype=np.int64)
        self.patch_start = np.zeros((self.total, 3), dtype=np.int64)
        self.regions = np.zeros((self.total, 8), dtype=np.int32)
        if self.total:
            check(lib.dsx_tile_plan(ds, gs, ps, mode, self.grid_start.ctypes.data_as(C.POINTER(C.c_int64)),
                                    self.patch_start.ctypes.data_as(C.POINTER(C.c_int64)), self.total))
            check(lib.dsx_tile_regions(ds, gs, ps, mode, self.regions.ctypes.data_as(C.POINTER(C.c_int32)),
                                       self.total))
        self._h = None
        self._layouts = {}
        # the regions every paste uses: the valid regions, clipped where a later tile overwrites (a ragged extent's
        # shifted last tile), so that all tiles can be pasted at once with the sequential loop's result
        self.valid_regions = self.regions
        try:
            clipped = np.zeros((self.total, 8), dtype=np.int32)
            if self.total:
                check(lib.dsx_tileplan_regions(self.handle, clipped.ctypes.data_as(C.POINTER(C.c_int32)), self.total))
            self.regions = clipped
        except DsxError:
            pass                                     # tiling modes whose tiles leave the frames have no device plan

    # ---- the device-resident plan ------------------------------------------------------------------------
    @property
    def handle(self):
        if self._h is None:
            h = C.c_void_p()
            check(lib.dsx_tileplan_create(_i64x3(self.data_shape), _i64x3(self.grid_shape), _i64x3(self.patch_shape),
                                          self.mode, C.byref(h)))
            self._h = h
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                lib.dsx_tileplan_destroy(h)
            except Exception:
                pass

    def _ids(self, tile_ids):
        ids = np.arange(self.total, dtype=np.int64) if tile_ids is None else \
            np.ascontiguousarray(np.asarray(tile_ids, dtype=np.int64).reshape(-1))
        if ids.size and (ids.min() < 0 or ids.max() >= self.total):
            raise DsxError("tile id out of range")
        return ids

    def gather(self, frames, tile_ids=None):
        """frames: (N,H,W) fp32 CUDA tensor -> (count, ph, pw) tiles (all tiles by default)."""
        _lib.require_gpu()
        if not frames.is_cuda or frames.dtype != torch.float32 or tuple(frames.shape) != self.data_shape:
            raise DsxError(f"frames must be a float32 CUDA tensor of shape {self.data_shape}")
        frames = frames.contiguous()
        ids = self._ids(tile_ids)
        out = torch.empty((len(ids), self.patch_shape[1], self.patch_shape[2]), dtype=torch.float32,
                          device=frames.device)
        seq = as_sequence(ids)
        if len(ids) and seq is not None:
            check(lib.dsx_tileplan_gather(self.handle, frames, seq[0], seq[1], seq[2], out, None))
        elif len(ids):
            check(lib.dsx_tiles_gather(frames, _i64x3(self.data_shape), _i64x3(self.patch_shape),
                                       self.patch_start.ctypes.data_as(C.POINTER(C.c_int64)),
                                       ids.ctypes.data_as(C.POINTER(C.c_int64)), len(ids), out, None))
        return out

    def randn_field(self, tile_ids, C_state, seed, draw=0, id_base=0, device="cuda"):
        """Frame-keyed noise (``dsx_tileplan_randn``): (count, C, ph, pw) normals, tile ``k`` cut at (n, y0, x0) holding
        the crop ``[:, y0:y0 + ph, x0:x0 + pw]`` of ``engine.randn_samples((1, C, H, W), seed, [id_base + n], draw)`` --
        a function of (seed, frame, draw, channel, y, x) in frame coordinates, so tiles of one frame share the bits of
        their overlap.  An arithmetic id sequence takes one launch, any other list one launch per tile."""
        _lib.require_gpu()
        ids = self._ids(tile_ids)
        Cn = int(C_state)
        if Cn < 1:
            raise DsxError(f"randn_field: C = {Cn}, must be at least 1")
        draw, id_base = self._field_draw("randn_field", draw, id_base)
        out = torch.empty((len(ids), Cn, self.patch_shape[1], self.patch_shape[2]), dtype=torch.float32, device=device)
        seed64 = C.c_uint64(int(seed) & (2 ** 64 - 1))
        call = lambda first, stride, count, dst: check(lib.dsx_tileplan_randn(
            self.handle, Cn, first, stride, count, seed64, C.c_uint64(id_base), C.c_uint32(draw), dst, None))
        return _per_sequence(ids, call, out)

    def _field_draw(self, what, draw, id_base):
        """-> (draw, id_base) as ints, both in the range of the noise fields of this plan's frames."""
        draw, id_base = int(draw), int(id_base)
        if not 0 <= draw < _lib.STREAM_DRAW_LIMIT:
            raise DsxError(f"{what}: draw ordinal {draw} out of range (0 <= draw < 2^24)")
        if not 0 <= id_base <= _lib.STREAM_ID_LIMIT - self.data_shape[0]:
            raise DsxError(f"{what}: id_base = {id_base} with {self.data_shape[0]} frames: every field id must be "
                           "below 2^40")
        return draw, id_base

    def _check_tiles(self, tiles):
        if not tiles.is_cuda or tiles.dtype != torch.float32 or tiles.dim() != 4:
            raise DsxError("tiles must be a (count,C,ph,pw) float32 CUDA tensor")
        if tuple(tiles.shape[2:]) != self.patch_shape[1:]:
            raise DsxError("tile size does not match the plan")
        return tiles.contiguous()

    def stitch(self, tiles, tile_ids=None, canvas=None):
        """tiles: (count, C, ph, pw) fp32 CUDA -> canvas (N,H,W,C), zero-initialised
        unless an existing canvas is passed (every batch / rank pastes its share)."""
        _lib.require_gpu()
        tiles = self._check_tiles(tiles)
        ids = self._ids(tile_ids)
        if len(ids) != tiles.shape[0]:
            raise DsxError("one tile id per tile")
        Cn = tiles.shape[1]
        if canvas is None:
            canvas = torch.zeros(self.data_shape + (Cn,), dtype=torch.float32, device=tiles.device)
        seq = as_sequence(ids)
        if len(ids) and seq is not None:
            check(lib.dsx_tileplan_stitch(self.handle, tiles, Cn, seq[0], seq[1], seq[2], canvas, None, None, None))
        elif len(ids):
            reg = np.ascontiguousarray(self.regions[ids])
            check(lib.dsx_stitch(tiles, len(ids), Cn, self.patch_shape[1], self.patch_shape[2],
                                 reg.ctypes.data_as(C.POINTER(C.c_int32)), canvas, _i64x3(self.data_shape), None))
        return canvas

    # ---- RangeInvariantPsnr sums accumulated while pasting ---------------------------------------------------
    def psnr_blocks(self):
        return int(lib.dsx_stitch_psnr_blocks(self.patch_shape[1], self.patch_shape[2]))

    def new_psnr_partials(self, Cn, device):
        """Partial-sum rows of every tile of the plan, [total][blocks][C][8] float64 (filled batch by batch)."""
        return torch.zeros((self.total, self.psnr_blocks(), Cn, 8), dtype=torch.float64, device=device)

    def _check_gt(self, gt, Cn):
        gt = gt.to(torch.float32).contiguous()
        if tuple(gt.shape) != self.data_shape + (Cn,) or not gt.is_cuda:
            raise DsxError(f"gt must be a CUDA tensor of shape {self.data_shape + (Cn,)}")
        if Cn > PSNR_MAX_CHANNELS:
            raise DsxError(f"the fused PSNR sums handle at most {PSNR_MAX_CHANNELS} channels")
        return gt

    def stitch_psnr_into(self, tiles, tile_ids, canvas, gt, partials):
        """Paste the tiles ``tile_ids`` (an arithmetic id sequence) into ``canvas`` and write their PSNR partial sums
        to the rows ``partials[tile_ids]``: a batch of a longer run, no (total, C, ph, pw) buffer needed."""
        _lib.require_gpu()
        tiles = self._check_tiles(tiles)
        seq = as_sequence(self._ids(tile_ids))
        if seq is None or seq[2] != tiles.shape[0]:
            raise DsxError("stitch_psnr_into needs one id per tile, ids in arithmetic sequence")
        if seq[2] == 0:
            return
        Cn = tiles.shape[1]
        gt = self._check_gt(gt, Cn)
        rows = torch.empty((seq[2],) + tuple(partials.shape[1:]), dtype=torch.float64, device=tiles.device)
        check(lib.dsx_tileplan_stitch(self.handle, tiles, Cn, seq[0], seq[1], seq[2], canvas, gt, rows, None))
        partials[seq[0]:seq[0] + (seq[2] - 1) * seq[1] + 1:seq[1]] = rows

    def psnr_from_partials(self, partials):
        """(N, C) RangeInvariantPsnr (core/psnr.py:70-82) from the partial-sum rows of all tiles."""
        N = self.data_shape[0]                                      # tile ids are frame-major (tiling_manager.py:145-154)
        Cn = partials.shape[2]
        # rows of a paste, [total][blocks][C][8] (frame-major tiles), or of a blend, [N][blocks][C][8]
        p = partials.view(N, -1, Cn, 8)
        s = p[..., :5].sum(dim=1)                                    # fixed order: reproducible
        gmin, gmax = p[..., 5].amin(dim=1), p[..., 6].amax(dim=1)
        return range_invariant_psnr_from_sums(s[..., 0], s[..., 1], s[..., 2], s[..., 3], s[..., 4], gmin, gmax,
                                              float(self.data_shape[1] * self.data_shape[2]))

    def stitch_with_psnr(self, tiles, gt):
        """Stitch ALL tiles (count == total, id order) and compute RangeInvariantPsnr (core/psnr.py:70-82) of every
        (frame, channel) against ``gt`` (N,H,W,C fp32 CUDA) from sums accumulated while pasting: no second pass
        over the canvas.  Returns (canvas (N,H,W,C), psnr (N,C) float64 on the device)."""
        _lib.require_gpu()
        if tiles.shape[0] != self.total:
            raise DsxError("stitch_with_psnr needs every tile of the plan")
        Cn = tiles.shape[1]
        canvas = torch.zeros(self.data_shape + (Cn,), dtype=torch.float32, device=tiles.device)
        part = self.new_psnr_partials(Cn, tiles.device)
        self.stitch_psnr_into(tiles, np.arange(self.total), canvas, gt, part)
        return canvas, self.psnr_from_partials(part)

    # ---- cropped exchange for multi-GPU tiled prediction (tile_stitcher.py:38-56 before the collective) ----
    def pack_layout(self, world):
        """Host only: (pixel offset of every tile inside its rank's packed run [total], pixels of every rank's run
        [world]) for the sharding ``id % world``; multiply by C for elements."""
        world = int(world)
        if world not in self._layouts:
            off = np.zeros(self.total, dtype=np.int64)
            rp = np.zeros(world, dtype=np.int64)
            check(lib.dsx_tileplan_pack_layout(self.handle, world, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                               rp.ctypes.data_as(C.POINTER(C.c_int64))))
            self._layouts[world] = (off, rp)
        return self._layouts[world]

    def rank_stride(self, world, Cn):
        """Elements of one rank's slot in the exchange buffer: the longest run (equal counts, as RCCL wants)."""
        return int(self.pack_layout(world)[1].max()) * int(Cn) if self.total else 0

    def pack(self, tiles, world, first, flat_rank):
        """Valid regions of the predicted tiles ``first, first + world, ...`` (tiles.shape[0] of them) -> their places
        in ``flat_rank``, the packed run of rank ``first % world`` (a 1-D fp32 CUDA tensor of rank_stride elements)."""
        _lib.require_gpu()
        tiles = self._check_tiles(tiles)
        Cn = tiles.shape[1]
        if flat_rank.dtype != torch.float32 or not flat_rank.is_cuda or not flat_rank.is_contiguous() or \
                flat_rank.numel() < int(self.pack_layout(world)[1][int(first) % int(world)]) * Cn:
            raise DsxError("flat_rank must be a contiguous float32 CUDA tensor that holds this rank's run")
        check(lib.dsx_tileplan_pack(self.handle, tiles, Cn, int(world), int(first), int(tiles.shape[0]), flat_rank, None))

    def paste_packed(self, flat_all, Cn, world, gt=None):
        """Every tile of the plan from the gathered exchange buffer (world, rank_stride) -> canvas (N,H,W,C); with
        ``gt`` also the (N, C) RangeInvariantPsnr.  Returns canvas or (canvas, psnr)."""
        _lib.require_gpu()
        flat_all = flat_all.contiguous()
        stride = flat_all.numel() // int(world)
        if flat_all.dtype != torch.float32 or not flat_all.is_cuda or stride < self.rank_stride(world, Cn):
            raise DsxError("flat_all must be a float32 CUDA tensor of world * rank_stride elements")
        canvas = torch.zeros(self.data_shape + (Cn,), dtype=torch.float32, device=flat_all.device)
        part = None
        if gt is not None:
            gt = self._check_gt(gt, Cn)
            part = self.new_psnr_partials(Cn, flat_all.device)
        check(lib.dsx_tileplan_paste_packed(self.handle, flat_all, int(Cn), int(world), stride, canvas, gt, part, None))
        return canvas if gt is None else (canvas, self.psnr_from_partials(part))

    # ---- blended stitching: the overlap-add of all tiles (dsx_tileplan_blend) ---------------------------------------
    def contributors(self):
        """Host only: (rows (H, 2), cols (W, 2)) int32 -- per canvas row (first tile row, count), per canvas column
        (first tile column, count).  Tile (iy, ix) of frame n has id (n * ny + iy) * nx + ix."""
        rows = np.zeros((self.data_shape[1], 2), dtype=np.int32)
        cols = np.zeros((self.data_shape[2], 2), dtype=np.int32)
        check(lib.dsx_tileplan_contributors(self.handle, rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                            cols.ctypes.data_as(C.POINTER(C.c_int32))))
        return rows, cols

    def set_window(self, win):
        """The separable blend window of the plan: a name of ``WINDOWS`` or a pair ``(wy (ph,), wx (pw,))`` of arrays,
        every value finite and > 0.  Host only; goes to the device once, at the next ``blend``."""
        if isinstance(win, str):
            wy, wx = window(win, self.patch_shape[1]), window(win, self.patch_shape[2])
        else:
            wy, wx = (np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)) for w in win)
        if wy.size != self.patch_shape[1] or wx.size != self.patch_shape[2]:
            raise DsxError(f"set_window: the window must have {self.patch_shape[1]} and {self.patch_shape[2]} values, "
                           f"got {wy.size} and {wx.size}")
        check(lib.dsx_tileplan_set_window(self.handle, wy, wx))
        self._window = (wy, wx)

    def blend_blocks(self):
        return int(lib.dsx_tileplan_blend_blocks(self.handle))

    def blend_rank_stride(self, world, Cn):
        """Elements of one rank's slot of WHOLE tiles in the exchange buffer of a blend: rank 0's, the longest."""
        return -(-self.total // int(world)) * int(Cn) * self.patch_shape[1] * self.patch_shape[2]

    def _whole_tiles(self, what, tiles, world, Cn):
        """Every tile of the plan as ``blend`` and ``blend_step`` take them -> (tiles, Cn, slot stride).  One rank:
        a (total, C, ph, pw) tensor, stride 0.  Several: the gathered exchange buffer of ``world`` equal slots of at
        least ``blend_rank_stride`` elements, with its channel count ``Cn``."""
        if world == 1:
            tiles = self._check_tiles(tiles)
            if tiles.shape[0] != self.total:
                raise DsxError(f"{what} needs every tile of the plan")
            return tiles, int(tiles.shape[1]), 0
        tiles = tiles.contiguous()
        if Cn is None or tiles.dtype != torch.float32 or not tiles.is_cuda:
            raise DsxError(f"{what}: a gathered buffer is a float32 CUDA tensor and needs its channel count Cn")
        Cn, stride = int(Cn), tiles.numel() // world
        if stride < self.blend_rank_stride(world, Cn):
            raise DsxError(f"{what}: the gathered buffer must hold world slots of blend_rank_stride elements")
        return tiles, Cn, stride

    def blend(self, tiles, world=1, gt=None, canvas=None, Cn=None):
        """Every tile of the plan, overlap-added under the plan's window (``set_window`` first) -> canvas (N,H,W,C);
        with ``gt`` also the (N, C) RangeInvariantPsnr: (canvas, psnr).  ``world == 1``: ``tiles`` (total, C, ph, pw).
        ``world > 1``: the gathered exchange buffer of ``world`` equal slots, rank q's holding its whole tiles q,
        q + world, ... back to back, with ``Cn`` channels.  The result depends on the tiles alone, not on the layout.
        The partial-sum rows of the last call, (N, blend_blocks, C, 8) float64 or None, stay in ``last_blend_partials``."""
        _lib.require_gpu()
        world = int(world)
        tiles, Cn, stride = self._whole_tiles("blend", tiles, world, Cn)
        if canvas is None:
            canvas = torch.empty(self.data_shape + (Cn,), dtype=torch.float32, device=tiles.device)
        part = None
        if gt is not None:
            gt = self._check_gt(gt, Cn)
            part = torch.zeros((self.data_shape[0], self.blend_blocks(), Cn, 8), dtype=torch.float64, device=tiles.device)
        check(lib.dsx_tileplan_blend(self.handle, tiles, Cn, world, stride, canvas, gt, part, None))
        self.last_blend_partials = part
        return canvas if gt is None else (canvas, self.psnr_from_partials(part))

    def blend_step(self, x0_tiles, state, c_x0, c_xt, sigma, seed, draw, id_base=0, world=1, Cn=None):
        """One reverse step of the frame state with the blend of the tiles as its x0 (``dsx_tileplan_blend_step``):
        ``state`` (N,H,W,C) fp32 CUDA, contiguous, is updated IN PLACE and returned --
        ``X = c_x0 * blend(x0_tiles) + c_xt * X (+ Z * sigma where sigma != 0)``, every operation rounded on its own,
        ``Z`` the noise field (seed, id_base + n, draw) of frame n: ``engine.randn_samples((N, C, H, W), seed,
        [id_base + n], draw)`` in (N,H,W,C) order, generated inside the kernel.  ``x0_tiles``, ``world`` and ``Cn`` as
        in ``blend``; the state must not alias the tiles."""
        _lib.require_gpu()
        world = int(world)
        x0_tiles, Cn, stride = self._whole_tiles("blend_step", x0_tiles, world, Cn)
        if not torch.is_tensor(state) or not state.is_cuda or state.dtype != torch.float32 or \
                not state.is_contiguous() or tuple(state.shape) != self.data_shape + (Cn,):
            raise DsxError(f"blend_step: the state must be a contiguous float32 CUDA tensor of shape "
                           f"{self.data_shape + (Cn,)} (it is updated in place)")
        draw, id_base = self._field_draw("blend_step", draw, id_base)
        check(lib.dsx_tileplan_blend_step(self.handle, x0_tiles, Cn, world, stride, state, float(c_x0), float(c_xt),
                                          float(sigma), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(id_base),
                                          C.c_uint32(draw), None))
        return state

    # ---- tile disagreement: how far the tiles that predicted a pixel differ (dsx_tileplan_disagreement) -------------
    def crop_lines(self, band=8):
        """Host only: (rows (H,), cols (W,)) uint8 -- 1 where the canvas row / column is NEAR A CROP LINE: some line L,
        the first row / column owned by another tile row / column of ``regions`` than the one before it, has
        ``L - band <= v < L + band``."""
        rows = np.zeros(self.data_shape[1], dtype=np.uint8)
        cols = np.zeros(self.data_shape[2], dtype=np.uint8)
        check(lib.dsx_tileplan_crop_lines(self.handle, int(band), rows, cols))
        return rows, cols

    def disagreement(self, tiles, world=1, Cn=None, band=8, want_map=True, out=None):
        """How far the tiles that cover a canvas pixel differ (contract: include/dsx.h, dsx_tileplan_disagreement):
        per pixel and channel the unbiased variance ``var`` among its contributors, in ascending tile id, Welford in
        double.  ``tiles``, ``world`` and ``Cn`` as in ``blend`` (no window is needed); C <= 4.  ``want_map``: also
        ``s = float32(sqrt(var))`` per pixel, written into ``out`` (a contiguous float32 CUDA tensor of (N,H,W,C)) if one
        is given.  -> dict:

        ``map`` (N,H,W,C) float32 or None; ``count`` (N,C,2) int64: pixels with two or more contributors, and those of
        them IN THE BAND (their row or column near a crop line, ``crop_lines(band)``); ``sum_var`` (N,C,2) float64 over
        the same two sets; ``min_var``, ``max_var`` (N,C) over the first; ``rms_pair`` (N,C,2) =
        ``sqrt(2 * sum_var / count)``, the RMS difference over all pairs of contributors, NaN where the count is 0;
        ``partials`` (N, blend_blocks, C, 8) float64, the kernel's rows.  Everything on the device."""
        _lib.require_gpu()
        world, band = int(world), int(band)
        tiles, Cn, stride = self._whole_tiles("disagreement", tiles, world, Cn)
        if not 1 <= Cn <= PSNR_MAX_CHANNELS:
            raise DsxError(f"disagreement: C = {Cn}, must be in 1..{PSNR_MAX_CHANNELS}")
        shape = self.data_shape + (Cn,)
        if out is not None and not want_map:
            raise DsxError("disagreement: out= is the map; it needs want_map=True")
        if out is not None and (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or
                                not out.is_contiguous() or tuple(out.shape) != shape):
            raise DsxError(f"disagreement: out must be a contiguous float32 CUDA tensor of shape {shape}")
        smap = out if out is not None else \
            torch.empty(shape, dtype=torch.float32, device=tiles.device) if want_map else None
        part = torch.empty((self.data_shape[0], self.blend_blocks(), Cn, 8), dtype=torch.float64, device=tiles.device)
        check(lib.dsx_tileplan_disagreement(self.handle, tiles, Cn, world, stride, band, smap, part, None))
        return dict(disagreement_from_partials(part), map=smap, partials=part)

    def gather_canvas(self, canvas, tile_ids=None):
        """The tiles ``tile_ids`` cut out of a multi-channel frame state ``canvas`` (N,H,W,C) fp32 CUDA -> (count, C, ph,
        pw), bit for bit the slices.  An arithmetic id sequence takes one launch, any other list one launch per tile."""
        _lib.require_gpu()
        if not canvas.is_cuda or canvas.dtype != torch.float32 or canvas.dim() != 4 or \
                tuple(canvas.shape[:3]) != self.data_shape:
            raise DsxError(f"gather_canvas: canvas must be a float32 CUDA tensor of shape {self.data_shape + ('C',)}")
        canvas = canvas.contiguous()
        ids = self._ids(tile_ids)
        Cn = int(canvas.shape[3])
        out = torch.empty((len(ids), Cn, self.patch_shape[1], self.patch_shape[2]), dtype=torch.float32,
                          device=canvas.device)
        call = lambda first, stride, count, dst: check(lib.dsx_tileplan_gather_canvas(
            self.handle, canvas, Cn, first, stride, count, dst, None))
        return _per_sequence(ids, call, out)
