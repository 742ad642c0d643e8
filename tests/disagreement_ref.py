"""The tile-disagreement contract of include/dsx.h (dsx_tileplan_disagreement) restated in numpy float64: one numpy
operation per rounding, the contributors of a pixel in ascending tile id; crop lines and band masks by brute force from
``plan.regions``; the totals as exactly rounded sums (``math.fsum``), with the bound the device's sums must meet.

Per canvas pixel and channel, over its contributors v_1 .. v_k (Welford, as dsx_moments_update / _finish):

    mean = v_1; M2 = 0;   d = v - mean;  mean = mean + d / (r + 1);  M2 = M2 + d * (v - mean)
    var = k > 1 ? M2 / (k - 1) : 0        s = float32(sqrt(var))

The device computes every var with these operations in this order, so the terms of its sums are the float64 values this
file holds, bit for bit: the sums differ only by the order of the additions and their roundings.

Bound on |device - this| for a sum of m terms, u = 2^-53, all terms non-negative, T = their exact sum:

    m terms added in ANY order (threads, the wave butterfly, the four waves, the workgroup rows, every one of them an
    addition of partial sums):                  gamma_(m-1) = (m - 1) u / (1 - (m - 1) u)  of T
                                                (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4))
    this file's one rounding of T (fsum):       u

    |device - this| <= ((m - 1) + 1) u T + (m - 1)^2 u^2 T / (1 - (m - 1) u)  <=  (m + 1) u T      while m < 6.7e7:

the second-order term stays below the one spare u.  Non-negative terms cannot cancel, so the bound is relative to the
sum itself.  Zeros that a thread without a pixel adds change nothing.  Counts are integers and must be equal.

``mistaken`` holds the typical mistakes the contract must reject."""
import math

import numpy as np

U = 2.0 ** -53
SCORES = ("count", "sum_var", "min_var", "max_var")


def owner_canvas(plan):
    """(H, W) int: the tile of frame 0 whose clipped paste region holds the pixel; the regions partition the frame"""
    N, H, W = plan.data_shape
    own = np.full((H, W), -1, dtype=np.int64)
    for t in range(plan.total // N):
        n, y, x, h, w = (int(v) for v in plan.regions[t][:5])
        assert n == 0 and (own[y:y + h, x:x + w] == -1).all()
        own[y:y + h, x:x + w] = t
    assert own.min() >= 0
    return own


def crop_lines(plan):
    """(rows, cols): the crop lines -- rows y >= 1 (columns x >= 1) that another tile row (column) owns than y - 1 (x - 1)"""
    own = owner_canvas(plan)
    rows = [y for y in range(1, own.shape[0]) if (own[y] != own[y - 1]).any()]
    cols = [x for x in range(1, own.shape[1]) if (own[:, x] != own[:, x - 1]).any()]
    # the partition is a product of row ranges and column ranges: a line crosses the whole frame
    assert all((own[y] != own[y - 1]).all() for y in rows) and all((own[:, x] != own[:, x - 1]).all() for x in cols)
    return rows, cols


def near_masks(plan, band, lo=0, hi=0):
    """(rows (H,), cols (W,)) uint8: 1 where some line L has L - band <= v < L + band.  (lo, hi) shift the two ends: the
    mistakes."""
    N, H, W = plan.data_shape
    out = []
    for lines, D in zip(crop_lines(plan), (H, W)):
        m = np.zeros(D, dtype=np.uint8)
        for v in range(D):
            m[v] = any(L - band + lo <= v < L + band + hi for L in lines)
        out.append(m)
    return out


def variance(plan, tiles, weights=None, ddof=1, owner_only=False):
    """tiles (total, C, ph, pw) -> (var (N, H, W, C) float64, k (N, H, W) int): tile after tile in id order, every pixel's
    recurrence one numpy operation per rounding.  ``weights`` (ph, pw): the window-weighted variance (a mistake)."""
    tiles = np.asarray(tiles)
    assert tiles.dtype == np.float32
    N, H, W = plan.data_shape
    total, Cn, ph, pw = tiles.shape
    assert total == plan.total and (ph, pw) == plan.patch_shape[1:]
    mean, m2 = np.zeros((N, Cn, H, W)), np.zeros((N, Cn, H, W))
    k = np.zeros((N, H, W), dtype=np.int64)
    wsum = np.zeros((N, H, W))
    for t in range(total):
        n, y0, x0 = (int(v) for v in plan.patch_start[t])
        sl = (n, slice(None), slice(y0, y0 + ph), slice(x0, x0 + pw))
        kk = (n,) + sl[2:]
        if owner_only:
            _, y, x, h, w, ry, rx, _ = (int(v) for v in plan.regions[t])
            mean[n, :, y:y + h, x:x + w] = tiles[t][:, ry:ry + h, rx:rx + w]
            k[n, y:y + h, x:x + w] += 1
            continue
        v = tiles[t].astype(np.float64)
        first = (k[kk] == 0)[None]
        d = v - mean[sl]
        if weights is None:
            m1 = mean[sl] + d / (k[kk] + 1)[None].astype(np.float64)
            m2n = m2[sl] + d * (v - m1)
        else:                                                         # West's weighted update
            wsum[kk] = wsum[kk] + weights
            m1 = mean[sl] + d * (weights / wsum[kk])[None]
            m2n = m2[sl] + weights[None] * d * (v - m1)
        mean[sl] = np.where(first, v, m1)
        m2[sl] = np.where(first, 0.0, m2n)
        k[kk] += 1
    assert k.min() >= 1, "the plan does not cover its frames"
    if weights is None:
        den = np.maximum(k - ddof, 1).astype(np.float64)
    else:
        den = wsum * np.maximum(k - ddof, 1) / k
    var = np.where((k > 1)[:, None], m2 / den[:, None], 0.0)
    return np.ascontiguousarray(var.transpose(0, 2, 3, 1)), k


def scores(var, k, rows, cols, least=2):
    """-> dict of count (N,C,2) int64, sum_var (N,C,2), min_var, max_var (N,C), rms_pair (N,C,2) and the bound on the
    sums, over the pixels with k >= ``least`` and over those of them in the band"""
    N, H, W, Cn = var.shape
    over = k >= least
    band = over & ((rows[:, None] != 0) | (cols[None, :] != 0))[None]
    out = dict(count=np.zeros((N, Cn, 2), dtype=np.int64), sum_var=np.zeros((N, Cn, 2)), bound=np.zeros((N, Cn, 2)),
               min_var=np.full((N, Cn), np.inf), max_var=np.full((N, Cn), -np.inf))
    for n in range(N):
        for c in range(Cn):
            for j, sel in enumerate((over[n], band[n])):
                terms = var[n, :, :, c][sel]
                out["count"][n, c, j] = terms.size
                out["sum_var"][n, c, j] = math.fsum(terms.tolist())
                out["bound"][n, c, j] = (terms.size + 1) * U * out["sum_var"][n, c, j]
            if over[n].any():
                out["min_var"][n, c] = var[n, :, :, c][over[n]].min()
                out["max_var"][n, c] = var[n, :, :, c][over[n]].max()
    with np.errstate(invalid="ignore", divide="ignore"):
        out["rms_pair"] = np.where(out["count"] > 0, np.sqrt(2.0 * out["sum_var"] / out["count"]), np.nan)
    return out


def disagreement_ref(plan, tiles, band=8):
    """The contract: -> (map (N,H,W,C) float32, scores)"""
    var, k = variance(plan, tiles)
    rows, cols = near_masks(plan, band)
    return np.sqrt(var).astype(np.float32), scores(var, k, rows, cols)


MISTAKES = ("ddof0", "count_k1", "band_late", "band_short", "window", "owner_only")


def mistaken(plan, tiles, band, kind, window=None):
    """(map, scores) of a typical mistake: the biased variance, k = 1 pixels counted, a band one pixel off at either end,
    the variance weighted by the blend window, the contributors of the crop-pasted owner only"""
    kw, mk, least = {}, {}, 2
    if kind == "ddof0":
        kw = dict(ddof=0)
    elif kind == "count_k1":
        least = 1
    elif kind == "band_late":
        mk = dict(lo=1, hi=1)
    elif kind == "band_short":
        mk = dict(hi=-1)
    elif kind == "window":
        kw = dict(weights=np.outer(*window).astype(np.float64))
    elif kind == "owner_only":
        kw = dict(owner_only=True)
    else:
        raise ValueError(kind)
    var, k = variance(plan, tiles, **kw)
    rows, cols = near_masks(plan, band, **mk)
    return np.sqrt(var).astype(np.float32), scores(var, k, rows, cols, least)


def within_contract(got_map, got, want_map, want):
    """What the GPU test asserts of the device, as a predicate: map bits, counts and min / max equal, sums within the bound"""
    return bool(np.array_equal(np.asarray(got_map).view(np.int32), want_map.view(np.int32)) and
                np.array_equal(got["count"], want["count"]) and
                np.array_equal(np.asarray(got["min_var"]).view(np.int64), want["min_var"].view(np.int64)) and
                np.array_equal(np.asarray(got["max_var"]).view(np.int64), want["max_var"].view(np.int64)) and
                (np.abs(np.asarray(got["sum_var"]) - want["sum_var"]) <= want["bound"]).all())
