"""The blend contract of include/dsx.h (dsx_tileplan_blend) restated in numpy float32: one numpy operation per rounding,
the contributors of a pixel in ascending tile id.  Also the brute-force contributor tables, and the float64 form."""
import numpy as np

from diffsplitting_amd.data import tiling


def window_pair(plan, name):
    return tiling.window(name, plan.patch_shape[1]), tiling.window(name, plan.patch_shape[2])


def blend_ref(plan, tiles, wy, wx, dtype=np.float32):
    """tiles (total, C, ph, pw) -> canvas (N, H, W, C).  Tile after tile in id order, every pixel's running
    num = num + w * v and den = den + w rounded per operation in ``dtype``; a pixel with one contributor keeps its
    value, any other gets num / den."""
    tiles = np.asarray(tiles, dtype=dtype)
    N, H, W = plan.data_shape
    total, Cn, ph, pw = tiles.shape
    assert total == plan.total and (ph, pw) == plan.patch_shape[1:]
    w = (np.asarray(wy, dtype=dtype)[:, None] * np.asarray(wx, dtype=dtype)[None, :]).astype(dtype)   # one rounding
    num = np.zeros((N, Cn, H, W), dtype=dtype)
    den = np.zeros((N, H, W), dtype=dtype)
    cnt = np.zeros((N, H, W), dtype=np.int64)
    only = np.zeros((N, Cn, H, W), dtype=dtype)
    for t in range(total):
        n, y0, x0 = (int(v) for v in plan.patch_start[t])
        wv = (w[None] * tiles[t]).astype(dtype)
        num[n, :, y0:y0 + ph, x0:x0 + pw] = (num[n, :, y0:y0 + ph, x0:x0 + pw] + wv).astype(dtype)
        den[n, y0:y0 + ph, x0:x0 + pw] = (den[n, y0:y0 + ph, x0:x0 + pw] + w).astype(dtype)
        cnt[n, y0:y0 + ph, x0:x0 + pw] += 1
        only[n, :, y0:y0 + ph, x0:x0 + pw] = tiles[t]
    assert cnt.min() >= 1, "the plan does not cover its frames"
    out = np.where((cnt == 1)[:, None], only, (num / den[:, None]).astype(dtype))
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def cut_tiles(plan, canvas):
    """canvas (N, H, W, C) -> (total, C, ph, pw): what TilePlan.gather_canvas returns for all tiles."""
    ph, pw = plan.patch_shape[1:]
    return np.stack([np.ascontiguousarray(canvas[n, y0:y0 + ph, x0:x0 + pw].transpose(2, 0, 1))
                     for n, y0, x0 in plan.patch_start])


def contributors_brute(plan):
    """(rows (H, 2), cols (W, 2)) from plan.patch_start alone: per coordinate the tile rows / columns that cover it."""
    N, H, W = plan.data_shape
    ph, pw = plan.patch_shape[1:]
    per = plan.total // N
    ys = sorted({int(s[1]) for s in plan.patch_start[:per]})
    xs = sorted({int(s[2]) for s in plan.patch_start[:per]})
    assert len(ys) * len(xs) == per
    for t in range(plan.total):                                         # id = (n * ny + iy) * nx + ix
        n, r = divmod(t, per)
        assert tuple(plan.patch_start[t]) == (n, ys[r // len(xs)], xs[r % len(xs)])

    def axis(starts, ext, D):
        tab = np.zeros((D, 2), dtype=np.int32)
        for v in range(D):
            ks = [k for k, s in enumerate(starts) if s <= v < s + ext]
            assert ks and ks == list(range(ks[0], ks[-1] + 1))
            tab[v] = ks[0], len(ks)
        return tab
    return axis(ys, ph, H), axis(xs, pw, W)


def slots(plan, tiles, world):
    """tiles (total, C, ph, pw) -> the gathered exchange buffer (world, stride) of whole tiles, rank q's slot holding
    its tiles q, q + world, ... back to back; unused tails are NaN."""
    per_tile = int(np.prod(tiles.shape[1:]))
    stride = -(-plan.total // world) * per_tile
    buf = np.full((world, stride), np.nan, dtype=np.float32)
    for q in range(world):
        own = tiles[q::world].reshape(-1)
        buf[q, :own.size] = own
    return buf
