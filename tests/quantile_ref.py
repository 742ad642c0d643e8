"""The contract of dsx_sample_quantiles (include/dsx.h) restated in numpy, the inputs the quantile tests share, and the
typical mistakes of an implementation, each as a variant the restatement must differ from.

Per element: the n samples in ascending order of the order-preserving integer image of the fp32 value (-0 before +0);
on the host, in double, pos = (n - 1) q, lo = floor(pos), hi = min(lo + 1, n - 1), t = pos - lo; then in double, every
operation rounded on its own, a = v[lo], b = v[hi], d = b - a, r = t < 0.5 ? a + d t : b - d (1 - t), and the cast to
fp32.  rank = #{ r : x_r < target }, strict, on the fp32 values."""
import fractions

import numpy as np

Q6 = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.975, 1.0)       # lo == hi, both lerp branches, integral positions at odd n
Q8 = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0)


def image(x):
    """The order-preserving integer image of fp32 values: negative floats with their magnitude bits flipped."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & 0x7fffffff)


def sort_samples(x):
    """x (n, ...) fp32 sorted along axis 0 by the integer image."""
    x = np.asarray(x, dtype=np.float32)
    return np.take_along_axis(x, np.argsort(image(x), axis=0, kind="stable"), axis=0)


def positions(n, q):
    """(lo, hi, t) of every q, formed in double as the host entry point forms them."""
    pos = np.float64(n - 1) * np.asarray(q, dtype=np.float64)
    lo = np.floor(pos)
    return lo.astype(np.int64), np.minimum(lo.astype(np.int64) + 1, n - 1), pos - lo


def quantiles(x, q):
    """(len(q), ...) fp32: the contract."""
    x = np.asarray(x, dtype=np.float32)
    v = sort_samples(x).astype(np.float64)
    out = np.empty((len(q),) + x.shape[1:], dtype=np.float32)
    for k, (lo, hi, t) in enumerate(zip(*positions(x.shape[0], q))):
        a, b = v[lo], v[hi]
        d = b - a
        out[k] = (a + d * t if t < 0.5 else b - d * (1.0 - t)).astype(np.float32)
    return out


def ranks(x, target):
    """(...) fp32: samples strictly below the target, compared as fp32 values."""
    x, target = np.asarray(x, dtype=np.float32), np.asarray(target, dtype=np.float32)
    return (x < target[None]).sum(axis=0).astype(np.float32)


def _fma(a, d, t):
    """a + d * t rounded ONCE (what a fused multiply-add returns), element by element in exact rational arithmetic"""
    F = fractions.Fraction
    flat = [float(F(float(u)) + F(float(w)) * F(float(t))) for u, w in zip(a.reshape(-1), d.reshape(-1))]
    return np.array(flat, dtype=np.float64).reshape(a.shape)


MISTAKES = ("lerp32", "single_branch", "fma", "padded_pos", "last_unsorted")


def mistaken(x, q, which):
    """The quantiles of an implementation with one of MISTAKES."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    v = sort_samples(x)
    if which == "last_unsorted":                       # a network whose last wire never takes part
        v = np.concatenate([sort_samples(x[:-1]), x[-1:]]) if n > 1 else v
    wires = max(2, 1 << (n - 1).bit_length())
    if which == "padded_pos":                          # positions taken from the padded length
        v = np.concatenate([v, np.full((wires - n,) + x.shape[1:], np.inf, dtype=np.float32)])
    lo, hi, t = positions(wires if which == "padded_pos" else n, q)
    out = np.empty((len(q),) + x.shape[1:], dtype=np.float32)
    for k in range(len(q)):
        if which == "lerp32":
            a, b, tk = v[lo[k]], v[hi[k]], np.float32(t[k])
            d = b - a
            out[k] = a + d * tk if tk < 0.5 else b - d * (np.float32(1) - tk)
            continue
        a, b = v[lo[k]].astype(np.float64), v[hi[k]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = b - a
            if which == "single_branch":
                r = a + d * t[k]
            elif which == "fma":
                r = _fma(a, d, t[k]) if t[k] < 0.5 else _fma(b, -d, 1.0 - t[k])
            else:
                r = a + d * t[k] if t[k] < 0.5 else b - d * (1.0 - t[k])
        out[k] = r.astype(np.float32)
    return out


def ranks_le(x, target):
    """The rank with <= in place of <."""
    return (np.asarray(x, dtype=np.float32) <= np.asarray(target, dtype=np.float32)[None]).sum(axis=0).astype(np.float32)


# ----------------------------------------------------------------------------- shared inputs
def stack(n, count, seed=0):
    """(n, count) standard normal fp32 samples and a target drawn like them; no -0, ties have probability ~0."""
    rng = np.random.default_rng([seed, n, count])
    return rng.standard_normal((n, count)).astype(np.float32), rng.standard_normal(count).astype(np.float32)


WITNESS_Q = (0.25 + 2.0 ** -52, 0.75 - 2.0 ** -52)


def witnesses(count):
    """(2, count) samples a = 1, b = 1 + D 2^-22 (D odd, 2^21 < D < 2^22: 0.5 < d = b - a < 1) for q = WITNESS_Q, where
    a rounding in double survives the cast to fp32.  The cast hides nearly every one-ulp difference between two double
    lerps: on random inputs a fused multiply-add or the single-branch lerp would pass.  Here a + d / 4 = 1 + D 2^-24 is
    exactly the midpoint of two fp32 neighbours, and the second term of t moves the exact value off it by d 2^-52,
    just over half an ulp of the double sum.
    First half, D from 2^21 + 1 (d just above 0.5) at t = 0.25 + 2^-52: the separately rounded product d t carries
    2^-53 of that term, the sum is a tie in double, rounds to the fp32 midpoint and the cast rounds to even; a fused
    multiply-add sees the whole term, rounds up in double and so in the cast: every second element differs.
    Second half, D from 2^21 + 2^18 + 1 (d >= 0.5625) at t = 0.75 - 2^-52: the two-branch form b - d (1 - t) and the
    single branch a + d t round their products differently, and again every second element differs."""
    half = count // 2
    D = np.concatenate([2 ** 21 + 1 + 2 * np.arange(half, dtype=np.int64),
                        2 ** 21 + 2 ** 18 + 1 + 2 * np.arange(count - half, dtype=np.int64)])
    assert D.max() < 2 ** 22
    b = (1.0 + D * 2.0 ** -22).astype(np.float32)
    assert (b.astype(np.float64) == 1.0 + D * 2.0 ** -22).all()
    return np.stack([np.ones(count, dtype=np.float32), b])


def tied(n, count, seed=0):
    """Heavily tied samples: eight levels (-1.5 .. 1.5 and both zeros), and a target that equals one of the samples of
    its element wherever the element index is even."""
    rng = np.random.default_rng([seed, n, count, 8])
    levels = np.array([-1.5, -0.75, -0.0, 0.0, 0.25, 0.75, 1.0, 1.5], dtype=np.float32)
    x = levels[rng.integers(0, 8, (n, count))]
    t = levels[rng.integers(0, 8, count)]
    even = np.arange(count) % 2 == 0
    t[even] = x[rng.integers(0, n, count), np.arange(count)][even]
    return x, t
