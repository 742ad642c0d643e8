"""Float64 restatement of dsx_comoments (include/dsx.h) and of the curve built on it, with error bounds derived from
the arithmetic alone -- no tolerance is typed in by hand.

The 12 numbers of a plane triple (g, p1, p2), n fp32 pixels each:

    {n, min g, max g, mean g, mean p1, mean p2, Cgg, C11, C22, Cg1, Cg2, C12},   Cxy = sum (x - mean x)(y - mean y)

are restated the way the kernel centres them: x' = (double)x[i] - (double)x[0] (one IEEE subtraction: the kernel holds
the SAME x'), Sx = sum x', Sxy = sum x' y', mean x = x[0] + Sx / n, Cxy = Sxy - Sx Sy / n; every sum with math.fsum.

Bounds, u = 2^-53, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4):
recursive summation of n terms IN ANY ORDER, an fma's product entering unrounded, has |error| <= gamma_(n-1) sum |t_i|;
gamma_n also covers a rounded product):

    E(Sx)  = (gamma_n + 2 u) Ax,   Ax  = sum |x'|        device sum in any order + fsum's one rounding
    E(Sxy) = (gamma_n + 2 u) Axy,  Axy = sum |x' y'|     ... + this file's rounded products
    E(mean x) = E(Sx) / n + 4 u (|x0| + |Sx| / n)        the division and the addition, on both sides
    E(Cxy) = E(Sxy) + (|Sx| E(Sy) + |Sy| E(Sx) + E(Sx) E(Sy)) / n + 8 u (|Sx Sy| / n + |Sxy|)
                                                         the product, the division and the subtraction, on both sides

The curve.  With D = Cgg - gp^2 / pp (the residual sum of squares of the least-squares fit; gp = a Cg1 + b Cg2,
pp = a^2 C11 + 2 a b C12 + b^2 C22) the definition collapses to PSNR = 10 log10((max g - min g)^2 n / D), so

    E(gp) = |a| E(Cg1) + |b| E(Cg2),   E(pp) = a^2 E(C11) + 2 |a b| E(C12) + b^2 E(C22)
    E(D)  = E(Cgg) + (2 |gp| / pp) E(gp) + (gp^2 / pp^2) E(pp) + 16 u (Cgg + gp^2 / pp)     (first order in E(gp), E(pp);
                                                         the last term: the curve's own dozen float64 operations)
    E(PSNR) = (10 / ln 10) E(D) / (D - E(D)) + 8 u |PSNR|                  inf where E(D) >= D: nothing can be said
"""
import math

import numpy as np

U = 2.0 ** -53
NAMES = ("n", "min_g", "max_g", "mean_g", "mean_p1", "mean_p2", "Cgg", "C11", "C22", "Cg1", "Cg2", "C12")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))     # Cgg, C11, C22, Cg1, Cg2, C12 over (g, p1, p2)


def gamma(n):
    return n * U / (1.0 - n * U)


def _planes(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, "the planes are fp32 values"
    return x.reshape(x.shape[0], -1).astype(np.float64)


def moments(g, p1, p2, with_bounds=False):
    """(planes, 12) float64 [, the (planes, 12) bounds on |device - this|] of fp32 stacks (planes, ...)."""
    ops = [_planes(g), _planes(p1), _planes(p2)]
    P, n = ops[0].shape
    out, bnd = np.zeros((P, 12)), np.zeros((P, 12))
    gn = gamma(n) + 2 * U
    for p in range(P):
        x0 = [o[p, 0] for o in ops]
        sh = [o[p] - o[p, 0] for o in ops]
        S = [math.fsum(s) for s in sh]
        ES = [gn * math.fsum(np.abs(s)) for s in sh]
        out[p, 0:3] = n, ops[0][p].min(), ops[0][p].max()
        for k in range(3):
            out[p, 3 + k] = x0[k] + S[k] / n
            bnd[p, 3 + k] = ES[k] / n + 4 * U * (abs(x0[k]) + abs(S[k]) / n)
        for j, (x, y) in enumerate(PAIRS):
            prod = sh[x] * sh[y]
            Sxy = math.fsum(prod)
            out[p, 6 + j] = Sxy - S[x] * S[y] / n
            bnd[p, 6 + j] = (gn * math.fsum(np.abs(prod)) + (abs(S[x]) * ES[y] + abs(S[y]) * ES[x] + ES[x] * ES[y]) / n
                             + 8 * U * (abs(S[x] * S[y]) / n + abs(Sxy)))
    return (out, bnd) if with_bounds else out


def moments_raw_fp32(g, p1, p2):
    """What the contract forbids: raw (unshifted) sums accumulated in fp32, Cxy = Sxy - Sx Sy / n."""
    ops = [np.asarray(o, dtype=np.float32).reshape(np.asarray(o).shape[0], -1) for o in (g, p1, p2)]
    P, n = ops[0].shape
    out = np.zeros((P, 12))
    f32sum = lambda v: float(np.cumsum(v, dtype=np.float32)[-1])       # a serial fp32 accumulation
    for p in range(P):
        S = [f32sum(o[p]) for o in ops]
        out[p, 0:3] = n, ops[0][p].min(), ops[0][p].max()
        for k in range(3):
            out[p, 3 + k] = S[k] / n
        for j, (x, y) in enumerate(PAIRS):
            out[p, 6 + j] = f32sum(ops[x][p] * ops[y][p]) - S[x] * S[y] / n
    return out


def curve(m, a, b, ddof=1, cross=True):
    """The definition, as include/dsx.h states it -> (curve (planes, G), t_star (planes,)).  ``ddof=0`` and
    ``cross=False`` are the two mistakes the sensitivity test must see: var = Cgg / n, and pp without 2 a b C12."""
    m = np.asarray(m, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.float64).reshape(1, -1), np.asarray(b, dtype=np.float64).reshape(1, -1)
    n, lo, hi = m[:, 0:1], m[:, 1:2], m[:, 2:3]
    Cgg, C11, C22, Cg1, Cg2, C12 = (m[:, k:k + 1] for k in range(6, 12))
    with np.errstate(all="ignore"):
        var = Cgg / (n - ddof)
        gp = a * Cg1 + b * Cg2
        pp = a * a * C11 + (2 * a * b * C12 if cross else 0.0) + b * b * C22
        mse = np.maximum(((n - 1) - gp * gp / (var * pp)) / n, 0.0)     # an exact fit may round below 0: +inf dB
        c = 10 * np.log10((hi - lo) ** 2 / var / mse)
        c = np.where((hi == lo) | ~(pp > 0), np.nan, c)
        det = C11 * C22 - C12 * C12
        u0, u1 = C22 * Cg1 - C12 * Cg2, C11 * Cg2 - C12 * Cg1
        t = np.where((det == 0) | (u0 + u1 == 0), np.nan, u0 / (u0 + u1))
    return c, t[:, 0]


def curve_bound(m, mb, a, b):
    """E(PSNR) in dB (planes, G) from the moments and their bounds (the module docstring); NaN where the curve is."""
    m, mb = np.asarray(m, dtype=np.float64), np.asarray(mb, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.float64).reshape(1, -1), np.asarray(b, dtype=np.float64).reshape(1, -1)
    Cgg, C11, C22, Cg1, Cg2, C12 = (m[:, k:k + 1] for k in range(6, 12))
    Egg, E11, E22, Eg1, Eg2, E12 = (mb[:, k:k + 1] for k in range(6, 12))
    c, _ = curve(m, a, b)
    with np.errstate(all="ignore"):
        gp = a * Cg1 + b * Cg2
        pp = a * a * C11 + 2 * a * b * C12 + b * b * C22
        Egp, Epp = np.abs(a) * Eg1 + np.abs(b) * Eg2, a * a * E11 + 2 * np.abs(a * b) * E12 + b * b * E22
        fit = gp * gp / pp
        D = Cgg - fit
        ED = Egg + 2 * np.abs(gp) / pp * Egp + fit / pp * Epp + 16 * U * (Cgg + fit)
        e = np.where(ED < D, (10 / math.log(10)) * ED / (D - ED), np.inf) + 8 * U * np.abs(c)
    return np.where(np.isnan(c), np.nan, e)


def t_star_bound(m, mb):
    """First-order bound of t* = u0 / (u0 + u1), u0 = C22 Cg1 - C12 Cg2, u1 = C11 Cg2 - C12 Cg1:
    E(u0) = |C22| E(Cg1) + |Cg1| E(C22) + |C12| E(Cg2) + |Cg2| E(C12) + 4 u (|C22 Cg1| + |C12 Cg2|), E(u1) alike;
    E(t*) = (|u1| E(u0) + |u0| E(u1)) / ((u0 + u1)^2 - |u0 + u1| (E(u0) + E(u1))) + 4 u |t*|; inf when the sum's sign is open."""
    m, mb = np.asarray(m, dtype=np.float64), np.asarray(mb, dtype=np.float64)
    Cgg, C11, C22, Cg1, Cg2, C12 = (m[:, k] for k in range(6, 12))
    Egg, E11, E22, Eg1, Eg2, E12 = (mb[:, k] for k in range(6, 12))
    with np.errstate(all="ignore"):
        u0, u1 = C22 * Cg1 - C12 * Cg2, C11 * Cg2 - C12 * Cg1
        E0 = np.abs(C22) * Eg1 + np.abs(Cg1) * E22 + np.abs(C12) * Eg2 + np.abs(Cg2) * E12 \
            + 4 * U * (np.abs(C22 * Cg1) + np.abs(C12 * Cg2))
        E1 = np.abs(C11) * Eg2 + np.abs(Cg2) * E11 + np.abs(C12) * Eg1 + np.abs(Cg1) * E12 \
            + 4 * U * (np.abs(C11 * Cg2) + np.abs(C12 * Cg1))
        s = np.abs(u0 + u1)
        den = s * s - s * (E0 + E1)
        return np.where(den > 0, (np.abs(u1) * E0 + np.abs(u0) * E1) / den, np.inf) + 4 * U * np.abs(u0 / (u0 + u1))


def direct_curve(g, p, weights):
    """RangeInvariantPsnr(g, p_j) of core/psnr.py:23-34, every line of it in float64, for predictions built by the
    caller: ``weights`` = [(a, b), ...] gives p_j = a p1 + b p2 with ``p`` = (p1, p2).  -> (planes, G)."""
    gt, p1, p2 = _planes(g), _planes(p[0]), _planes(p[1])
    cols = []
    for a, b in weights:
        pred = a * p1 + b * p2
        std = gt.std(axis=1, ddof=1, keepdims=True)
        ra = (gt.max(axis=1) - gt.min(axis=1)) / std[:, 0]
        gs = (gt - gt.mean(axis=1, keepdims=True)) / std
        gs = gs - gs.mean(axis=1, keepdims=True)
        pc = pred - pred.mean(axis=1, keepdims=True)
        alpha = (gs * pc).sum(axis=1, keepdims=True) / (pc * pc).sum(axis=1, keepdims=True)
        mse = ((gs - alpha * pc) ** 2).mean(axis=1)
        cols.append(20 * np.log10(ra / np.sqrt(mse)))
    return np.stack(cols, axis=1)


def planted(shape, seed=0, t=0.3):
    """The generator of the checks: g = 3 (t p1 + (1 - t) p2 + 0.05 N) + 5 on p1 = 2 N + 1, p2 = 0.7 N - 3, all fp32,
    drawn from ONE default_rng(seed) in the order p1, p2, g."""
    rng = np.random.default_rng(seed)
    N = lambda: rng.standard_normal(shape).astype(np.float32)
    p1 = (2 * N() + 1).astype(np.float32)
    p2 = (np.float32(0.7) * N() - 3).astype(np.float32)
    g = (3 * (np.float32(t) * p1 + np.float32(1 - t) * p2 + np.float32(0.05) * N()) + 5).astype(np.float32)
    return g, p1, p2


def hostile(n=1023, seed=1):
    """name -> (g, p1, p2), each (3, n) fp32 with distinct data per plane: inputs on which a careless implementation
    shows.  'counts': raw-count-like planes (mean 1e4, spread 30), where raw moments cancel 1e5-fold; 'offset': the same
    with the first pixel an outlier (the shift is a poor centre); 'equal': p1 == p2 (S singular, t* NaN); 'constant':
    a constant g (every curve value NaN); 'anti': p1 and p2 strongly anti-correlated (the cross term carries the curve)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    N = lambda: rng.standard_normal((3, n)).astype(f)
    cases = {}
    p1, p2 = (1e4 + 30 * N()).astype(f), (1e4 + 30 * N()).astype(f)
    g = (f(0.3) * p1 + f(0.7) * p2 + f(3) * N()).astype(f)
    cases["counts"] = (g, p1, p2)
    g2, q1, q2 = g.copy(), p1.copy(), p2.copy()
    g2[:, 0] += 500; q1[:, 0] -= 400; q2[:, 0] += 300
    cases["offset"] = (g2, q1, q2)
    e = (2 * N() + 1).astype(f)
    cases["equal"] = ((e + f(0.1) * N()).astype(f), e, e.copy())
    cases["constant"] = (np.full((3, n), 2.5, dtype=f), (2 * N()).astype(f), N())
    base = N()
    a1, a2 = (base + f(0.05) * N()).astype(f), (-base + f(0.05) * N()).astype(f)
    cases["anti"] = ((f(0.6) * a1 + f(0.4) * a2 + f(0.01) * N()).astype(f), a1, a2)
    return cases
