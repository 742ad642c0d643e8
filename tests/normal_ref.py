"""The engine's normal stream restated with numpy, from the definition in ``dsx_kernels.h`` (helper module, no test).

Element i of the stream (seed, subseq) is component ``i % 4`` of ``normal4(seed, subseq, i // 4)``:

    r        = philox4x32_10(counter = (idx4 lo, idx4 hi, subseq lo, subseq hi), key = (seed lo, seed hi))
    u_k      = (float32(r_k) + 0.5f) * 2^-32                     every operation in float32, in (0, 1]
    ra, rb   = sqrt(-2 ln u_0), sqrt(-2 ln u_2)
    angle_k  = float32(6.283185307179586) * u_k                  in float32, k = 1 and 3
    z        = (ra cos angle_1, ra sin angle_1, rb cos angle_3, rb sin angle_3)

The integer part and the float32 conversions and products are reproduced exactly; the logarithm, the root, the sine and
the cosine of those float32 operands are taken in float64, so that ``z`` is the value that the device's float32 libm
approximates.  ``close`` bounds the difference in units of ``2^-24 * radius``: |cos|, |sin| <= 1, so one float32 ulp of
a component is at most that.

``MUTANTS`` names the ways in which an implementation can be wrong and still produce plausible normals; ``stream``
takes one of them by name so that the tests can show that the comparison rejects each.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TWO_PI_F = np.float32(6.283185307179586)
INV_2_32_F = np.float32(2.0 ** -32)
# The bound of the device comparisons (tests/test_gpu_normal_stream.py states how it was measured and refuses a value
# above K_LIMIT): the device's logf, sqrtf, sincosf and product in float32 against the float64 values here.  Twice the
# measured maximum of 3.617, rounded up.
K_DEVICE = 8
K_LIMIT = 8
MUTANTS = ("swap_sincos", "seed_hi_dropped", "subseq_hi_dropped", "one_angle", "block_off_by_one", "order", "nine_rounds")


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox-4x32 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words -> four such arrays."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniforms(r):
    """(float32(r) + 0.5f) * 2^-32 with every operation rounded to float32, as the device does it."""
    f = _u64(r).astype(np.float32)                                # round to nearest even, like v_cvt_f32_u32
    return (f + np.float32(0.5)).astype(np.float32) * INV_2_32_F


def sample_subseq(sample_id, draw):
    return ((int(sample_id) << 24) | int(draw)) & (2 ** 64 - 1)


def stream(seed, subseq, n, mutant=None):
    """The first n elements of the stream (seed, subseq) -> (z, radius), float64 each; radius[i] is the Box-Muller
    radius that element i was multiplied by."""
    assert mutant is None or mutant in MUTANTS
    seed, subseq, n = int(seed), int(subseq), int(n)
    assert 0 <= seed < 2 ** 64 and 0 <= subseq < 2 ** 64 and n >= 0
    idx4 = np.arange((n + 3) // 4, dtype=np.uint64)
    if mutant == "block_off_by_one":
        idx4 = idx4 + np.uint64(1)
    s_hi = 0 if mutant == "subseq_hi_dropped" else subseq >> 32
    k_hi = 0 if mutant == "seed_hi_dropped" else seed >> 32
    r = philox4x32_10(idx4 & M32, idx4 >> np.uint64(32), np.uint64(subseq & 0xFFFFFFFF), np.uint64(s_hi),
                      np.uint64(seed & 0xFFFFFFFF), np.uint64(k_hi), rounds=9 if mutant == "nine_rounds" else 10)
    u = [uniforms(w) for w in r]
    ra = np.sqrt(-2.0 * np.log(u[0].astype(np.float64)))
    rb = np.sqrt(-2.0 * np.log(u[2].astype(np.float64)))
    ang_a = (TWO_PI_F * u[1]).astype(np.float64)
    ang_b = ang_a if mutant == "one_angle" else (TWO_PI_F * u[3]).astype(np.float64)
    cos, sin = (np.sin, np.cos) if mutant == "swap_sincos" else (np.cos, np.sin)
    comps = [ra * cos(ang_a), ra * sin(ang_a), rb * cos(ang_b), rb * sin(ang_b)]
    if mutant == "order":
        comps = [comps[0], comps[2], comps[1], comps[3]]
    z = np.stack(comps, axis=1).reshape(-1)[:n]
    radius = np.stack([ra, ra, rb, rb], axis=1).reshape(-1)[:n]
    return z, radius


def worst_ratio(got, z, radius):
    """max over the elements of |got - z| / (2^-24 * radius) and its index.  Where the radius is 0, z is 0 and so must
    got be: any other value counts as an infinite ratio, and so does a value that is not finite."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert got.shape == z.shape == radius.shape, (got.shape, z.shape, radius.shape)
    if got.size == 0:
        return 0.0, -1
    err = np.abs(got - z)
    unit = radius * 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


def close(got, z, radius, K):
    """elementwise |got - z| <= K * 2^-24 * radius -> (ok, worst ratio, its index)"""
    worst, i = worst_ratio(got, z, radius)
    return worst <= K, worst, i
