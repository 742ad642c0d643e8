"""Float64 restatement of dsx_calibration (include/dsx.h) with an error bound derived from the arithmetic alone -- no
tolerance is typed in by hand -- and the inputs the CPU and the GPU tests share.

Per channel c of three channel-last fp32 canvases (mean, std, target), n pixels each:

    s   = float64(std),   e = float64(target) - float64(mean)
    bin = searchsorted(edges[c], s, side='right')                 edges[c] = np.quantile(s, j / nbins), j = 1 .. nbins - 1
    count[bin] = bincount,   Sv[bin] = sum s^2,   Se[bin] = sum e^2,   cover[k] = #(s >= 0 and |e| <= z[k] * s)

Counts and coverage are integers: the device must give the same.  (z[k] * s is one float64 product on both sides, and
the comparison is against |e| as the device holds it: e with its one rounding.)

The sums here are the exactly rounded sums of the EXACT terms.  s^2 is exact in float64 (a 24-bit significand squared),
so Sv is math.fsum of the float64 products.  e^2 is not a float64 in general, nor is e itself (two fp32 values far
apart in exponent), so Se is summed in integer arithmetic: every fp32 is an integer multiple of 2^-149, e^2 one of
2^-298, and the total is rounded once by Python's correctly rounded integer division.

Bound on |device - this| for a bin of k pixels, u = 2^-53, all terms non-negative, T = their exact sum:

    the device's e carries one rounding:        e' = e (1 + d1),            |d1| <= u
    its square one more:                        fl(e'^2) = e^2 (1 + d1)^2 (1 + d2)   -> each term within (3 u + 3 u^2) of exact
    k terms added in ANY order:                 gamma_(k-1) = (k - 1) u / (1 - (k - 1) u)  of the sum of the terms
                                                (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4))
    this file's one rounding of T:              u

    |device - this| <= ((k - 1) + 3 + 1) u T + O(k^2 u^2) T  <=  (k + 4) u T      while k^2 u < 1 / 2, i.e. k < 6.7e7:

the second-order terms ((k - 1)^2 u^2 of gamma, 3 (k - 1) u^2 of the cross term, 3 u^2) stay below the one spare u.  Sv
needs only (k - 1) + 1 of it (its terms are exact on both sides); it gets the same bound.  A fused multiply-add in place
of the rounded square drops d2 and stays inside.

`emulate` restates the ORDER of csrc/dsx_calib.hip on the CPU (workgroups of span pixels, threads taking groups of four
values, batches of 64 lanes, a slot's terms in ascending lane order or, from nine lanes of one slot in a batch, by the 32,
16, .. 1 butterfly, the four waves pairwise, the workgroup rows lane by lane and the butterfly again), and `mistaken`
holds the typical mistakes the bound must reject."""
import math

import numpy as np

U = 2.0 ** -53
SERIAL_MAX = 8      # kCalSerial of csrc/dsx_calib.hip: lanes of one key in a batch that still add one after the other
Z_OF = {0: (), 3: (1.0, 2.0, 3.0), 8: (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0)}


def edges_of(std, nbins):
    """(C, nbins - 1) float64: np.quantile of every channel of an (n, C) fp32 spread"""
    s = np.asarray(std)
    assert s.dtype == np.float32 and s.ndim == 2
    q = np.arange(1, nbins, dtype=np.float64) / nbins
    return np.stack([np.quantile(s[:, c].astype(np.float64), q) if nbins > 1 else np.zeros(0) for c in range(s.shape[1])])


def _units(x32):
    """fp32 values -> Python ints in units of 2^-149 (exact)"""
    m, ex = np.frexp(np.asarray(x32, dtype=np.float64))
    mi, sh = (m * 2.0 ** 24).astype(np.int64).tolist(), (ex.astype(np.int64) - 24 + 149).tolist()
    return [(a << b) if b >= 0 else (a >> -b) for a, b in zip(mi, sh)]       # b < 0: only zeros are shifted out


def _bins(s, edges, side="right"):
    return np.searchsorted(edges, s, side=side) if edges.size else np.zeros(s.shape, dtype=np.int64)


def stats(mean, std, target, edges, z, with_bounds=False):
    """(C, 3 * nbins + nz) float64 in the layout of out_dev [, the bounds on |device - this|: 0 for the integers]."""
    mean, std, target = (np.asarray(x) for x in (mean, std, target))
    assert mean.dtype == std.dtype == target.dtype == np.float32 and mean.shape == std.shape == target.shape
    n, C = std.shape
    edges = np.asarray(edges, dtype=np.float64).reshape(C, -1)
    nbins, nz = edges.shape[1] + 1, len(z)
    out, bnd = np.zeros((C, 3 * nbins + nz)), np.zeros((C, 3 * nbins + nz))
    for c in range(C):
        s = std[:, c].astype(np.float64)
        e = target[:, c].astype(np.float64) - mean[:, c].astype(np.float64)
        b = _bins(s, edges[c])
        cnt = np.bincount(b, minlength=nbins)
        assert cnt.size == nbins and cnt.sum() == n
        d = [t - m for t, m in zip(_units(target[:, c]), _units(mean[:, c]))]
        s2 = s * s                                                  # exact
        for k in range(nbins):
            idx = np.flatnonzero(b == k)
            sv = math.fsum(s2[idx])
            se = sum(d[i] * d[i] for i in idx) / (1 << 298)          # int / int: correctly rounded
            out[c, 3 * k:3 * k + 3] = cnt[k], sv, se
            bnd[c, 3 * k + 1], bnd[c, 3 * k + 2] = (cnt[k] + 4) * U * sv, (cnt[k] + 4) * U * se
        for k, zk in enumerate(z):
            out[c, 3 * nbins + k] = np.count_nonzero((s >= 0) & (np.abs(e) <= np.float64(zk) * s))
    return (out, bnd) if with_bounds else out


def mistaken(mean, std, target, edges, z, which):
    """`stats` with one typical mistake: 'left' (searchsorted side), 'strict' (< in the coverage), 'e32' (the error
    formed in fp32), 'acc32' (fp32 accumulation), 'nosquare' (Sv sums std, not std^2).  Plain float64 sums otherwise."""
    mean, std, target = (np.asarray(x) for x in (mean, std, target))
    n, C = std.shape
    edges = np.asarray(edges, dtype=np.float64).reshape(C, -1)
    nbins, nz = edges.shape[1] + 1, len(z)
    out = np.zeros((C, 3 * nbins + nz))
    for c in range(C):
        s = std[:, c].astype(np.float64)
        e = (target[:, c] - mean[:, c]).astype(np.float64) if which == "e32" else \
            target[:, c].astype(np.float64) - mean[:, c].astype(np.float64)
        b = _bins(s, edges[c], side="left" if which == "left" else "right")
        v = s if which == "nosquare" else s * s
        for k in range(nbins):
            sel = b == k
            if which == "acc32":
                acc = lambda t: float(np.cumsum(t.astype(np.float32), dtype=np.float32)[-1]) if t.size else 0.0
            else:
                acc = lambda t: math.fsum(t)
            out[c, 3 * k:3 * k + 3] = np.count_nonzero(sel), acc(v[sel]), acc((e * e)[sel])
        for k, zk in enumerate(z):
            lim = np.float64(zk) * s
            out[c, 3 * nbins + k] = np.count_nonzero((s >= 0) & ((np.abs(e) < lim) if which == "strict" else (np.abs(e) <= lim)))
    return out


def is_integer_slot(nbins, nz):
    """mask over a row of 3 * nbins + nz slots: True where the slot is a count"""
    m = np.zeros(3 * nbins + nz, dtype=bool)
    m[0:3 * nbins:3] = True
    m[3 * nbins:] = True
    return m


def agrees(got, ref, bnd, nbins, nz):
    """the contract: integer slots equal, sums within the bound"""
    ints = is_integer_slot(nbins, nz)
    return bool(np.array_equal(got[:, ints], ref[:, ints]) and (np.abs(got - ref) <= bnd)[:, ~ints].all())


def _butterfly_down(v):
    v = np.asarray(v, dtype=np.float64).copy()
    lanes = np.arange(64)
    o = 32
    while o:
        v = v + v[lanes ^ o]
        o >>= 1
    return v[0]


def emulate(mean, std, target, edges, z, span):
    """The sums in the order of csrc/dsx_calib.hip; ``span`` = the pixels one workgroup takes before a second one joins
    (read from dsx_calibration_blocks).  The cap on the number of workgroups is not restated (tests stay below it)."""
    mean, std, target = (np.asarray(x) for x in (mean, std, target))
    n, C = std.shape
    edges = np.asarray(edges, dtype=np.float64).reshape(C, -1)
    nbins, nz = edges.shape[1] + 1, len(z)
    R = C * (3 * nbins + nz)
    blocks = max(1, -(-n // span))
    per = (-(-n // blocks) + 3) // 4 * 4 * C                         # values per workgroup
    s = std.reshape(-1).astype(np.float64)
    e = target.reshape(-1).astype(np.float64) - mean.reshape(-1).astype(np.float64)
    ch = np.arange(n * C) % C
    b = np.zeros(n * C, dtype=np.int64)
    for c in range(C):
        b[ch == c] = _bins(s[ch == c], edges[c])
    slot = ch * (3 * nbins + nz) + 3 * b
    rows = np.zeros((blocks, R))
    for blk in range(blocks):
        e0, e1 = blk * per, min(n * C, (blk + 1) * per)
        red = np.zeros((4, R))
        for it in range(max(0, -(-(e1 - e0) // 1024))):
            for wave in range(4):
                for j in range(4):                                   # a batch: value j of every lane's group
                    fs = [e0 + 1024 * it + 4 * (64 * wave + lane) + j for lane in range(64)]
                    keys = {}
                    for lane, f in enumerate(fs):
                        if f < e1:
                            keys.setdefault(slot[f], []).append(lane)
                    for sl, lanes in keys.items():
                        red[wave, sl] += len(lanes)
                        if len(lanes) > SERIAL_MAX:                  # a crowded key: the butterfly, +0.0 in the other lanes
                            for q, term in ((1, s), (2, e)):
                                v = np.zeros(64)
                                v[lanes] = [term[fs[l]] * term[fs[l]] for l in lanes]
                                red[wave, sl + q] += _butterfly_down(v)
                        else:                                        # one after the other, in ascending lane order
                            for l in lanes:
                                red[wave, sl + 1] += s[fs[l]] * s[fs[l]]
                                red[wave, sl + 2] += e[fs[l]] * e[fs[l]]
                    for f in fs:
                        if f < e1:
                            for k, zk in enumerate(z):
                                red[wave, ch[f] * (3 * nbins + nz) + 3 * nbins + k] += bool(s[f] >= 0 and abs(e[f]) <= np.float64(zk) * s[f])
        rows[blk] = (red[0] + red[1]) + (red[2] + red[3])
    out = np.zeros(R)
    for j in range(R):
        lanes = np.zeros(64)
        for r in range(blocks):
            lanes[r % 64] += rows[r, j]
        out[j] = _butterfly_down(lanes)
    return out.reshape(C, -1)


def cases(n, C, seed=0):
    """name -> (mean, std, target), each (n, C) fp32: the inputs on which a careless implementation shows.
    'random': finite data with a few negative spreads; 'ties': std drawn from the multiples of 1/8, 0 included, so that
    many values sit exactly on an edge; 'equal': one std for every pixel (every edge equals it: all pixels fall into the
    last bin, the others stay empty); 'zeros': a third of the pixels with std = 0, half of those with no error either;
    'boundary': std = 0.5 and an error of exactly +-1 (|e| = z std at z = 2) or +-0.5 (z = 1); 'wide': std from 1e-20
    to 1e20 with errors to scale."""
    rng = np.random.default_rng([seed, n, C])
    f = np.float32
    N = lambda: rng.standard_normal((n, C)).astype(f)
    out = {}
    mean, std = N(), (np.abs(N()) * f(0.5) + f(0.01)).astype(f)
    std[rng.random((n, C)) < 0.05] *= f(-1)
    out["random"] = (mean, std, (mean + f(1.3) * std * N()).astype(f))
    mean, std = N(), (rng.integers(0, 17, (n, C)) / 8).astype(f)
    out["ties"] = (mean, std, (mean + std * N()).astype(f))
    mean, std = N(), np.full((n, C), 0.75, dtype=f)
    out["equal"] = (mean, std, (mean + std * N()).astype(f))
    mean, std = N(), (np.abs(N()) + f(0.1)).astype(f)
    zero = rng.random((n, C)) < 1 / 3
    std[zero] = 0
    target = (mean + N()).astype(f)
    still = zero & (rng.random((n, C)) < 0.5)
    target[still] = mean[still]
    out["zeros"] = (mean, std, target)
    mean = (rng.integers(-8, 9, (n, C)) / 4).astype(f)
    step = rng.choice(np.array([-1, -0.5, 0.5, 1, 1.25], dtype=f), (n, C))
    out["boundary"] = (mean, np.full((n, C), 0.5, dtype=f), (mean + step).astype(f))
    std = (10.0 ** rng.uniform(-20, 20, (n, C))).astype(f)
    mean = (std * N()).astype(f)
    out["wide"] = (mean, std, (mean + std * N()).astype(f))
    return out
