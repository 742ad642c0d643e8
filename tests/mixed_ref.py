"""Version-independent restatements of the mixed-input arithmetic, and the error bound of its fp32 chain.

Nothing here calls the project's kernels; numpy only.  tests/test_mixed_cpu.py checks these restatements against the
fixture the reference's own code produced (tests/golden/mix_range.npz, tools/gen_mix_range_golden.py) and against
torch's float32 evaluation of the notebook expressions; the GPU tests compare the kernels with them bitwise.

`range_table`     compute_input_normalization_dict (data/time_predictor_dataset.py:6-21) in float64.
`normalize`       normalize_target (data/split_dataset.py:199-201): float64 arithmetic, rounded to float32 once.
`chain_f32`       the op list of include/dsx.h (dsx_tiles_gather_mix) with every operand an explicit np.float32, so that
                  neither numpy 1.x's value-based casting nor numpy 2's promotion rules decide a precision.
`chain_f64`       the same formulas from the same float32 channels, everything else in float64: "the exact value".
`chain_bound`     |chain_f32 - chain_f64| per element, from the fp32 unit roundoff u = 2^-24 and the operand magnitudes.

Derivation of the bound (g_k = k u / (1 - k u), the usual accumulated-rounding constant).  Per element, with the exact
weights a = 1 - t, b = t and the channels x, y (fp32 values, no error of their own):
    w0 = fl(a), w1 = fl(b)                         one rounding each
    p = fl(x w0), q = fl(y w1)                     one each: |p - x a| <= g_2 |x a|, likewise q
    m = fl(p + q)                                  one:      |m - (x a + y b)| <= g_3 (|x a| + |y b|)            =: E_m
    d = fl(m - fl(lo))                             fl(lo): u |lo|; the subtraction: u |d|
                                                             |d - (M - lo)| <= E_m + u |lo| + u (|D| + E_m + u |lo|) =: E_d
    e = fl(2 d)                                    exact (a power of two)
    r = fl(hi - lo)                                hi - lo in float64 (its own rounding, 2^-53, is neglected), then one
    s = fl(e / r)                                  one:      |s - 2 D / R| <= (2 E_d / R) (1 + g_2) + g_2 |2 D / R| =: E_s
    c = fl(s - 1)                                  one:      |c - C| <= E_s + u (|C| + E_s)                       =: E_c
where capitals are the exact values (M = x a + y b, D = M - lo, R = hi - lo, C = 2 D / R - 1).  The mix channels are
bounded by E_m, the classifier channels by E_c.  Six roundings lie on the path from a channel value to `cls`
(weight, product, sum, difference, quotient, difference), plus the two of the table constants.
"""
import numpy as np

U32 = 2.0 ** -24


def _g(k):
    return k * U32 / (1 - k * U32)


def range_table(ch0, ch1, n, mean, std):
    """(n + 1, 2) float64 {min, max}: as the reference, frame by frame, all in float64."""
    mean, std = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
    a = [(np.asarray(x).astype(np.float64) - mean[0]) / std[0] for x in ch0]
    b = [(np.asarray(x).astype(np.float64) - mean[1]) / std[1] for x in ch1]
    out = np.empty((n + 1, 2), dtype=np.float64)
    for t_int in range(n + 1):
        t = np.float64(t_int) / np.float64(n)
        lo, hi = np.inf, -np.inf
        for x, y in zip(a, b):
            v = t * x + (np.float64(1) - t) * y
            lo, hi = min(lo, v.min()), max(hi, v.max())
        out[t_int] = lo, hi
    return out


def normalize(patch, mean, std):
    return ((np.asarray(patch).astype(np.float64) - np.float64(mean)) / np.float64(std)).astype(np.float32)


def rows(table, t):
    """(lo0, hi0, lo1, hi1) of the table rows int((1 - t) n), int(t n) (Python's truncating int: the notebook's)."""
    n = len(table) - 1
    r0, r1 = int((1 - t) * n), int(t * n)
    return (table[r0][0], table[r0][1], table[r1][0], table[r1][1])


def _cls32(m, lo, hi):
    f = np.float32
    return (f(2) * (m - f(lo))) / f(np.float64(hi) - np.float64(lo)) - f(1)


def chain_f32(t0, t1, t, lohi=None):
    """-> (mix (2, ...), cls (2, ...) or None): float32 arrays, one IEEE operation per step."""
    t0, t1 = np.asarray(t0, dtype=np.float32), np.asarray(t1, dtype=np.float32)
    w1, w0 = np.float32(t), np.float32(1.0 - float(t))
    m0 = t0 * w0 + t1 * w1
    m1 = t1 * w0 + t0 * w1
    assert m0.dtype == np.float32 and m1.dtype == np.float32
    mix = np.stack([m0, m1])
    if lohi is None:
        return mix, None
    cls = np.stack([_cls32(m0, lohi[0], lohi[1]), _cls32(m1, lohi[2], lohi[3])])
    assert cls.dtype == np.float32
    return mix, cls


def chain_f64(t0, t1, t, lohi=None):
    x, y = np.asarray(t0, dtype=np.float32).astype(np.float64), np.asarray(t1, dtype=np.float32).astype(np.float64)
    t = np.float64(t)
    m0, m1 = x * (1 - t) + y * t, y * (1 - t) + x * t
    mix = np.stack([m0, m1])
    if lohi is None:
        return mix, None
    lo0, hi0, lo1, hi1 = [np.float64(v) for v in lohi]
    return mix, np.stack([2 * (m0 - lo0) / (hi0 - lo0) - 1, 2 * (m1 - lo1) / (hi1 - lo1) - 1])


def chain_bound(t0, t1, t, lohi=None):
    """Per-element bounds (mix (2, ...), cls (2, ...) or None) on |chain_f32 - chain_f64|: the docstring's E_m, E_c."""
    x, y = np.abs(np.asarray(t0, dtype=np.float32).astype(np.float64)), np.abs(np.asarray(t1, dtype=np.float32).astype(np.float64))
    t = np.float64(t)
    a, b = abs(1 - t), abs(t)
    e_m = np.stack([_g(3) * (x * a + y * b), _g(3) * (y * a + x * b)])
    if lohi is None:
        return e_m, None
    mix, cls = chain_f64(t0, t1, t, lohi)
    e_c = []
    for c in range(2):
        lo, hi = np.float64(lohi[2 * c]), np.float64(lohi[2 * c + 1])
        R, D = abs(hi - lo), np.abs(mix[c] - lo)
        e_d = e_m[c] + U32 * abs(lo) + U32 * (D + e_m[c] + U32 * abs(lo))
        e_s = (2 * e_d / R) * (1 + _g(2)) + _g(2) * (2 * D / R)
        e_c.append(e_s + U32 * (np.abs(cls[c]) + e_s))
    return e_m, np.stack(e_c)
