"""Float64 restatement of dsx_consistency (include/dsx.h) with an error bound derived from the arithmetic alone -- no
tolerance is typed in by hand -- and the inputs the CPU and the GPU tests share.

Per pixel, in float64, every operation rounded on its own (numpy fuses nothing), channels in ascending order:

    x   = float64(input)
    sat = clip >= 0 and x >= clip
    p_c = float64(mean[c]) * a_c + b_c
    m   = ((0 + w_0 p_0) + w_1 p_1) + ..
    r   = x - m                                     map = float32(r), for every pixel
    v_c = (float64(std[c]) * a_c)^2  or 1.0 without std
    den = (sum_c (w_c w_c) v_c) + noise_var
    not sat and den > 0:   p'_c = p_c + ((v_c w_c) r) / den          out_mean[c] = float32((p'_c - b_c) / a_c)
                           v'_c = v_c - ((v_c w_c)(v_c w_c)) / den   out_std[c]  = float32(sqrt(max(v'_c, 0)) / a_c)
    otherwise:             out_mean[c] = mean[c],  out_std[c] = std[c] (0 without std): the bits copied

The row of a frame: {k unsaturated, saturated, S r, S r r, S x, S x x, k_den = #(unsaturated, den > 0), S (r r) / den over
those, min r, max r}; sums, min and max over the unsaturated pixels.  map, out_mean, out_std must equal this file bit
for bit; counts, min and max are integers or inputs' own values: exact.

The sums.  Device and restatement add the SAME float64 terms: r, r * r, x, x * x and (r * r) / den are formed by the
rounded operations above, so their bits agree on both sides.  What differs is the order.  u = 2^-53, T = sum |t_i| of
a frame's k terms:

    k terms added in ANY order:             gamma_(k-1) = (k - 1) u / (1 - (k - 1) u) of T
                                            (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4))
    this file's one rounding (math.fsum):   u |S| <= u T

    |device - this| <= ((k - 1) + 1) u T + O(k^2 u^2) T  <=  (k + 4) u T      while k^2 u < 1 / 2, i.e. k < 6.7e7:

the second-order term (k - 1)^2 u^2 T stays below the spare 4 u T.  For the sums of non-negative terms T is the sum
itself, so the bound is relative; for S r it is (k + 4) u S |r|, for S x (a float32 acquisition may be negative)
(k + 4) u S |x|.  (k + 4) is the factor tests/calibration_ref.py arrives at; it is kept so that the two read alike.

`mistaken` holds the typical mistakes the contract must reject, each injected into a copy of the restatement."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SLOTS = 10
INT_SLOTS = (0, 1, 6)
A = (1234.5, 987.25, 2000.0, 555.125)       # std_target per channel
B = (1500.0, 1100.5, 900.25, 700.0)         # mean_target
W = (0.9, 0.7, 1.3, 0.45)                   # none of them 1: w and w^2 must not be confused


def _fma(a, b, c):
    """round(a * b + c) with ONE rounding, element by element (exact rational arithmetic)"""
    out = np.empty(np.broadcast(a, b, c).shape)
    it = np.nditer([a, b, c, out], op_flags=[["readonly"]] * 3 + [["writeonly"]])
    for x, y, z, o in it:
        o[...] = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
    return out


def pointwise(x, mean, std, a, b, w, clip, noise_var, mistake=None):
    """x (frames, plane); mean, std (frames, plane, C) fp32, std may be None -> dict of float64 arrays r, den, x, sat and
    the fp32 outputs map, out_mean, out_std (None without std: the entry point refuses that output)"""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32 and (std is None or (std.dtype == np.float32 and std.shape == mean.shape))
    C = mean.shape[-1]
    a, b, w = (np.asarray(v, dtype=np.float64)[:C] for v in (a, b, w))
    x = np.asarray(x).astype(np.float64)
    sat = (x >= clip) if clip >= 0 else np.zeros(x.shape, dtype=bool)
    p = mean.astype(np.float64) * a + b
    m = np.zeros(x.shape)
    for c in range(C):
        m = _fma(w[c], p[..., c], m) if mistake == "fma_m" else m + w[c] * p[..., c]
    r = x - m
    if std is not None:
        t = std.astype(np.float64) * a
        v = t * t
    else:
        v = np.ones(mean.shape)
    den = np.zeros(x.shape)
    for c in range(C):
        den = den + (w[c] * w[c]) * v[..., c]
    if mistake != "no_noise":
        den = den + noise_var
    upd = ~sat & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        vw = v * w
        num = (v * w * w) if mistake == "vw2" else vw
        pc = p + (num * r[..., None]) / den[..., None]
        om = ((pc - b) / a).astype(np.float32)
        vp = v - (vw * vw) / den[..., None]
        os_ = (np.sqrt(np.maximum(vp, 0.0)) / a).astype(np.float32)
    return {"x": x, "r": r, "den": den, "sat": sat, "map": r.astype(np.float32),
            "out_mean": np.where(upd[..., None], om, mean),
            "out_std": None if std is None else np.where(upd[..., None], os_, std),      # no spread in, none out
            "p": p, "v": v}


def _acc32(t):
    return float(np.cumsum(np.asarray(t, dtype=np.float32), dtype=np.float32)[-1]) if len(t) else 0.0


def rows(pw, mistake=None, with_bounds=False):
    """(frames, 10) float64 in the layout of out_dev [, the bounds on |device - this|: 0 for counts, min and max]"""
    x, r, den, sat = pw["x"], pw["r"], pw["den"], pw["sat"]
    if mistake == "sat_summed":
        sat = np.zeros(sat.shape, dtype=bool)
    acc = _acc32 if mistake == "acc32" else math.fsum
    frames = x.shape[0]
    out, bnd = np.zeros((frames, SLOTS)), np.zeros((frames, SLOTS))
    for f in range(frames):
        ok = ~sat[f]
        xf, rf, df = x[f][ok], r[f][ok], den[f][ok]
        pos = df > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            chi = ((rf * rf) / df)[pos]
        k, kd = int(ok.sum()), int(pos.sum())
        out[f] = [k, int(sat[f].sum()), acc(rf), acc(rf * rf), acc(xf), acc(xf * xf), kd, acc(chi),
                  rf.min() if k else np.inf, rf.max() if k else -np.inf]
        bnd[f, 2] = (k + 4) * U * math.fsum(np.abs(rf))
        bnd[f, 3] = (k + 4) * U * out[f, 3]
        bnd[f, 4] = (k + 4) * U * math.fsum(np.abs(xf))
        bnd[f, 5] = (k + 4) * U * out[f, 5]
        bnd[f, 7] = (kd + 4) * U * out[f, 7]
    return (out, bnd) if with_bounds else out


def restate(x, mean, std, a, b, w, clip=-1.0, noise_var=0.0):
    """everything the device writes: dict with map, out_mean, out_std, rows, bounds"""
    pw = pointwise(x, mean, std, a, b, w, clip, noise_var)
    pw["rows"], pw["bounds"] = rows(pw, with_bounds=True)
    return pw


def mistaken(x, mean, std, a, b, w, clip, noise_var, which):
    """`restate` with one typical mistake: 'fma_m' (w_c p_c + m fused), 'sat_summed' (saturated pixels enter the sums and
    the unsaturated count), 'vw2' (v_c w_c^2 as the correction's numerator), 'acc32' (fp32 accumulation), 'no_noise' (den
    without noise_var)."""
    pw = pointwise(x, mean, std, a, b, w, clip, noise_var, mistake=which)
    pw["rows"] = rows(pw, mistake=which)
    return pw


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def rows_agree(got, ref, bnd):
    """counts, min and max equal; sums within the bound"""
    exact = [j for j in range(SLOTS) if j in INT_SLOTS or j >= 8]
    sums = [j for j in range(SLOTS) if j not in exact]
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.array_equal(got[:, exact], ref[:, exact]) and (np.abs(got[:, sums] - ref[:, sums]) <= bnd[:, sums]).all())


def agrees(got, ref):
    """the contract: the fp32 outputs bit for bit, the rows as `rows_agree` says; `got` may lack an output"""
    for k in ("map", "out_mean", "out_std"):
        if got.get(k) is not None and not same_bits(got[k], ref[k]):
            return False
    return got.get("rows") is None or rows_agree(got["rows"], ref["rows"], ref["bounds"])


PIX = {"u8": (np.uint8, 255), "u16": (np.uint16, 65535), "f32": (np.float32, 65535)}


def case(pix, frames, plane, C, seed=0, clip="off", std="given", tight=False):
    """-> dict(x, mean, std, a, b, w, clip, noise_var): the inputs on which a careless implementation shows.
    x: (frames, plane) of `pix` with 0 and the type's largest count present; the prediction splits x over the channels
    with an error of a few counts (`tight`: only the fp32 rounding of the normalised mean, so that r is rounding noise
    and one fused product shows in it).  clip: 'off'; 'on': three quarters of the range, some pixels exactly at it and
    above; 'all': the LAST frame saturated throughout (its row holds +-inf).  std: 'none'; 'given': positive, a few
    counts; 'zero': all 0 with noise_var = 0 (den == 0: everything copied); 'huge': given, with one value of 1e30."""
    dtype, top = PIX[pix]
    rng = np.random.default_rng([seed, frames, plane, C])
    a, b, w = (np.asarray(v[:C], dtype=np.float64) for v in (A, B, W))
    xf = rng.integers(0, top + 1, (frames, plane)).astype(np.float64)
    if pix == "f32":
        xf = xf + rng.random((frames, plane))
    xf[0, 0], xf[-1, -1] = 0, top
    limit = -1.0
    if clip != "off":
        limit = float(int(0.75 * top))
        xf[0, 1 % plane], xf[0, 2 % plane] = limit, limit + 1
        if clip == "all":
            xf[-1] = np.maximum(xf[-1], limit)
    x = xf.astype(dtype)
    share = rng.dirichlet(np.ones(C), (frames, plane))
    p = share * x.astype(np.float64)[..., None] / w
    if not tight:
        p = p + 3.0 * rng.standard_normal(p.shape)
    mean = ((p - b) / a).astype(np.float32)
    sd, noise_var = None, 2.25
    if std != "none":
        sd = ((1.0 + 4.0 * rng.random(p.shape)) / a).astype(np.float32)
        if std == "zero":
            sd[...] = 0
            noise_var = 0.0
        if std == "huge":
            sd[0, 3 % plane, 0] = 1e30
    return dict(x=x, mean=mean, std=sd, a=a, b=b, w=w, clip=limit, noise_var=noise_var)
