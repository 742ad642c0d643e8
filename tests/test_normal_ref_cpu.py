"""tests/normal_ref.py, the restatement that the device's normal stream is compared with, checked on its own: the Philox
known answers of Random123, the end points of the uniforms, that the construction yields independent N(0, 1) values,
and that the comparator rejects every way of being plausibly wrong.  No GPU."""
import numpy as np
import pytest

from tests import normal_ref as nr

# Random123, kat_vectors: philox4x32 with 10 rounds -- counter (4 words), key (2 words), result (4 words)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = nr.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want
    vec = nr.philox4x32_10(*(np.full(3, c, dtype=np.uint64) for c in ctr), *key)     # arrays as well as scalars
    assert all(w.shape == (3,) and (w == v).all() for w, v in zip(vec, want))


def test_uniform_end_points():
    r = np.array([0, 2 ** 24, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint64)
    u = nr.uniforms(r)
    assert u.dtype == np.float32 and np.isfinite(u).all() and (u > 0).all() and (u <= 1).all()
    assert u[0] == np.float32(2.0 ** -33)
    assert u[1] == np.float32((2.0 ** 24 + 0.5) * 2.0 ** -32) == np.float32(2.0 ** -8)  # 2^24 + 0.5 rounds to 2^24
    assert u[2] == 1.0                                                # a tie between 2^32 - 256 and 2^32, to even
    assert u[3] == 1.0                                                # float32(2^32 - 1) rounds to 2^32: the range is (0, 1]
    assert nr.uniforms(np.uint64(2 ** 32 - 129)) == np.float32(1 - 2.0 ** -24)        # the largest value below 1
    ra = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    assert np.isfinite(ra).all() and ra[3] == 0.0                     # radius 0, z = 0: no NaN


SEED, SUBSEQ, N = 7 | 5 << 40, (3 << 24) | 1 | 1 << 60, 2 ** 20
LAGS = (1, 2, 3, 4, 5, 8)


@pytest.fixture(scope="module")
def z():
    out = nr.stream(SEED, SUBSEQ, N)[0]
    out.setflags(write=False)
    return out


def test_stream_moments(z):
    n = z.size
    assert n == N and np.isfinite(z).all()
    m = z.mean()
    assert abs(m) <= 5 / np.sqrt(n), m
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n), z.var()
    assert abs((z ** 3).mean()) <= 5 * np.sqrt(15 / n), (z ** 3).mean()
    assert abs((z ** 4).mean() - 3) <= 5 * np.sqrt(96 / n), (z ** 4).mean()


def _phi(x):
    from math import erf
    return 0.5 * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def test_stream_kolmogorov(z):
    n = z.size
    cdf = _phi(np.sort(z))
    i = np.arange(1, n + 1)
    d = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    assert np.sqrt(n) * d <= 1.95, np.sqrt(n) * d                    # the asymptotic 0.1 % point


@pytest.mark.parametrize("k", LAGS)
def test_stream_lags(z, k):
    n = z.size
    assert abs((z[:-k] * z[k:]).mean()) <= 5 / np.sqrt(n)
    w = z ** 2 - 1                                                    # variance 2: the product of two has variance 4
    assert abs(0.5 * (w[:-k] * w[k:]).mean()) <= 5 / np.sqrt(n)


def test_streams_are_independent():
    n, seed, sid, draw = 2 ** 18, 2024, 9, 1
    base = nr.stream(seed, nr.sample_subseq(sid, draw), n)[0]
    assert nr.sample_subseq(sid, draw) == (9 << 24) | 1
    others = {"draw + 1": (seed, nr.sample_subseq(sid, draw + 1)), "id + 1": (seed, nr.sample_subseq(sid + 1, draw)),
              "id + 2^32": (seed, nr.sample_subseq(sid + 2 ** 32, draw)), "seed + 1": (seed + 1, nr.sample_subseq(sid, draw)),
              "seed bit 32": (seed | 1 << 32, nr.sample_subseq(sid, draw))}
    for name, (s, q) in others.items():
        o = nr.stream(s, q, n)[0]
        assert not np.array_equal(o, base), name
        assert abs((o * base).mean()) <= 5 / np.sqrt(n), (name, (o * base).mean() * np.sqrt(n))


K_TEETH = nr.K_LIMIT   # the largest K that the device comparisons may use


@pytest.mark.parametrize("seed,subseq", [(SEED, SUBSEQ), (2 ** 64 - 1, 2 ** 64 - 1)])
def test_close_accepts_one_ulp(seed, subseq):
    z, radius = nr.stream(seed, subseq, 1027)
    f = z.astype(np.float32)
    for got in (f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        # an ulp of z is at most 2^-23 |z| <= 2 units of 2^-24 radius: 1/2 ulp of rounding + 1 ulp <= 3 units
        ok, worst, i = nr.close(got, z, radius, 3)
        assert ok, (worst, i)
    assert nr.close(f.reshape(13, 79), z, radius, 1)[0]               # any shape, flat order
    bad = f.copy()
    bad[1000] = np.nan
    assert nr.close(bad, z, radius, K_TEETH)[1:] == (np.inf, 1000)


@pytest.mark.parametrize("mutant", nr.MUTANTS)
def test_close_rejects(mutant):
    z, radius = nr.stream(SEED, SUBSEQ, 1027)
    got = nr.stream(SEED, SUBSEQ, 1027, mutant=mutant)[0].astype(np.float32)
    ok, worst, i = nr.close(got, z, radius, K_TEETH)
    assert not ok and worst > 1000, (mutant, worst, i)               # not a near miss: thousands of units off
    assert nr.close(z.astype(np.float32), z, radius, 1)[0]
