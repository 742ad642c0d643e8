"""float64 numpy / scipy restatement of the multi-scale SSIM that include/dsx.h defines (dsx_msssim), the yardstick of
the MS-SSIM tests, and the structured test images they share.  Nothing here calls the engine.

The keyword switches of ``scale_means`` (``pool``, ``fine``, ``c2_per_scale``) state typical mistakes, so that the CPU
suite can show the restatement tells them apart; the defaults are the definition."""
import numpy as np
from scipy import ndimage

from tests.metrics_ref import _filter_valid, gaussian_window

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def pool2(x):
    """2 x 2 mean pooling, an odd last row or column dropped: ((x00 + x01) + (x10 + x11)) * 0.25."""
    h, w = x.shape[0] // 2 * 2, x.shape[1] // 2 * 2
    x = x[:h, :w]
    return ((x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])) * 0.25


def pool2_keep_odd(x):
    """The mistake: an odd last row / column is kept (padded by repeating it) instead of dropped."""
    return pool2(np.pad(x, ((0, x.shape[0] % 2), (0, x.shape[1] % 2)), mode="edge"))


def cs_ssim_maps(a, b, c1, c2):
    """The cs map and the SSIM map of one plane pair over the valid region."""
    win = gaussian_window()
    mu1, mu2 = _filter_valid(a, win), _filter_valid(b, win)
    s11 = _filter_valid(a * a, win) - mu1 * mu1
    s22 = _filter_valid(b * b, win) - mu2 * mu2
    s12 = _filter_valid(a * b, win) - mu1 * mu2
    cs = (2 * s12 + c2) / (s11 + s22 + c2)
    return cs, (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs


def range_invariant_transform(pred, target):
    """RangeInvariantPsnr's transform (core/psnr.py) of one plane pair in double -> (p', g', L)."""
    p, g = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        std = g.std(ddof=1)
        gn = (g - g.mean()) / std
        pc = p - p.mean()
        alpha = (gn * pc).sum() / (pc * pc).sum()
        return alpha * pc, gn, (g.max() - g.min()) / std


def scale_means(pred, target, scales, data_range=None, range_invariant=False, pool=pool2, c2_per_scale=False):
    """The (scales, 2) means {cs_s, ssim_s} of one plane pair."""
    a, b = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    L = data_range
    if range_invariant:
        a, b, L = range_invariant_transform(a, b)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    out = np.empty((scales, 2))
    for s in range(scales):
        with np.errstate(invalid="ignore"):
            cs, ss = cs_ssim_maps(a, b, c1, c2 / 4.0 ** s if c2_per_scale else c2)
        out[s] = cs.mean(), ss.mean()
        if s + 1 < scales:
            a, b = pool(a), pool(b)
    return out


def from_means(means, weights=WEIGHTS, fine="cs"):
    """prod_{s < S-1} max(cs_s, 0)^w_s * max(ssim_{S-1}, 0)^w_{S-1}; ``fine='ssim'`` is the mistake of using ssim_s at
    the fine scales too."""
    means, w = np.asarray(means, np.float64), np.asarray(weights, np.float64)
    S = len(w)
    terms = np.append(means[:S - 1, 0 if fine == "cs" else 1], means[S - 1, 1])
    return float(np.prod(np.maximum(terms, 0.0) ** w))


def msssim(pred, target, data_range=None, range_invariant=False, weights=WEIGHTS, **mistakes):
    """MS-SSIM of one plane pair -> (value, (S, 2) means)."""
    fine = mistakes.pop("fine", "cs")
    means = scale_means(pred, target, len(weights), data_range, range_invariant, **mistakes)
    return from_means(means, weights, fine), means


def _unit_filtered(rng, shape, sigma):
    x = ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode="wrap")
    return x / x.std()


def structured_pair(shape, seed):
    """(target, pred) fp32 arrays of ``shape`` (..., H, W): target = 0.6 G_6 + 0.3 G_1.5 + 0.1 n with G_sigma
    unit-variance Gaussian-filtered noise per plane, pred = target + 0.25 n'.  Structure at several scales, so that the
    scales differ."""
    rng = np.random.default_rng(seed)
    lead = int(np.prod(shape[:-2], dtype=np.int64))
    t = np.empty((lead,) + tuple(shape[-2:]))
    for i in range(lead):
        t[i] = (0.6 * _unit_filtered(rng, shape[-2:], 6.0) + 0.3 * _unit_filtered(rng, shape[-2:], 1.5) +
                0.1 * rng.standard_normal(shape[-2:]))
    p = t + 0.25 * rng.standard_normal(t.shape)
    return t.reshape(shape).astype(np.float32), p.reshape(shape).astype(np.float32)
