"""float64 numpy / scipy restatements of the reference's core/metrics.py, the yardstick of the core.metrics tests.
cv2 and torchvision are not dependencies, so these restate what they compute; nothing here calls the engine."""
import math

import numpy as np
from scipy import ndimage


def np_make_grid(t, nrow, padding=2):
    """torchvision.utils.make_grid(t, nrow, padding=2, normalize=False, pad_value=0) of (B, C, H, W) numpy."""
    if t.shape[1] == 1:
        t = np.concatenate([t, t, t], axis=1)
    n, c, h, w = t.shape
    xm = min(nrow, n)
    ym = int(math.ceil(n / xm))
    grid = np.zeros((c, (h + padding) * ym + padding, (w + padding) * xm + padding), t.dtype)
    for k in range(n):
        y, x = divmod(k, xm)
        grid[:, y * (h + padding) + padding:y * (h + padding) + padding + h,
             x * (w + padding) + padding:x * (w + padding) + padding + w] = t[k]
    return grid


def np_tensor2img(x, min_max=(-1, 1)):
    """core/metrics.py:8-34 in numpy float32: clamp, (x - lo) / (hi - lo), * 255, round half to even, uint8."""
    x = np.squeeze(np.asarray(x, np.float32))
    lo, hi = np.float32(min_max[0]), np.float32(min_max[1])
    x = np.minimum(np.maximum(x, lo), hi)
    x = (x - lo) / np.float32(min_max[1] - min_max[0])
    if x.ndim == 4:
        x = np_make_grid(x, int(math.sqrt(len(x)))).transpose(1, 2, 0)
    elif x.ndim == 3:
        x = x.transpose(1, 2, 0)
    return np.rint(x * np.float32(255.0)).astype(np.uint8)


def gaussian_window():
    """cv2.getGaussianKernel(11, 1.5) outer itself (core/metrics.py:78-79)."""
    k = np.exp(-0.5 / (1.5 * 1.5) * (np.arange(11) - 5.0) ** 2)
    k = k * (1.0 / k.sum())
    return np.outer(k, k)


def _filter_valid(x, win):
    return ndimage.correlate(x, win, mode="reflect")[5:-5, 5:-5]


def ssim_map(img1, img2, L=255.0):
    """The SSIM map of one 2-D channel over the valid region (core/metrics.py:72-92), float64."""
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    a = np.asarray(img1, np.float64)
    b = np.asarray(img2, np.float64)
    win = gaussian_window()
    mu1, mu2 = _filter_valid(a, win), _filter_valid(b, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(a * a, win) - mu1_sq
    s2 = _filter_valid(b * b, win) - mu2_sq
    s12 = _filter_valid(a * b, win) - mu1_mu2
    return ((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))


def ssim(img1, img2, L=255.0):
    """ssim() on 2-D or H x W x C images: the mean of the map over the valid region and all channels (cv2.filter2D
    filters every channel of a multi-channel array)."""
    if img1.ndim == 2:
        return ssim_map(img1, img2, L).mean()
    return np.mean([ssim_map(img1[..., c], img2[..., c], L) for c in range(img1.shape[2])])


def psnr(img1, img2, peak=255.0):
    """calculate_psnr (core/metrics.py:62-69) in float64."""
    mse = np.mean((np.asarray(img1, np.float64) - np.asarray(img2, np.float64)) ** 2)
    return float("inf") if mse == 0 else 20 * math.log10(peak / math.sqrt(mse))


def range_invariant_psnr(gt, pred, dtype=np.float64):
    """RangeInvariantPsnr (core/psnr.py:28-39) per (frame, channel) of (N, ..., C) arrays, every step in ``dtype``."""
    N, C_ = gt.shape[0], gt.shape[-1]
    out = np.zeros((N, C_), dtype)
    for n in range(N):
        for c in range(C_):
            g, p = gt[n, ..., c].astype(dtype).ravel(), pred[n, ..., c].astype(dtype).ravel()
            ra = (g.max() - g.min()) / g.std(ddof=1)
            g_ = (g - g.mean()) / g.std(ddof=1)
            g_ = g_ - g_.mean()
            p0 = p - p.mean()
            alpha = (g_ * p0).sum() / (p0 * p0).sum()
            out[n, c] = 20 * np.log10(ra / np.sqrt(((g_ - alpha * p0) ** 2).mean()))
    return out


def tie_values(min_max, n_per_level=1):
    """fp32 inputs whose tensor2img value before rounding is exactly k + 0.5 (round half to even decides them)."""
    lo, rng = np.float32(min_max[0]), np.float32(min_max[1] - min_max[0])
    out = []
    for k in range(255):
        x0 = np.float32(min_max[0] + (k + 0.5) / 255.0 * (min_max[1] - min_max[0]))
        cand = [x0]
        up, dn = x0, x0
        for _ in range(8):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
            cand += [up, dn]
        hits = [c for c in cand if ((c - lo) / rng * np.float32(255.0)) % np.float32(1.0) == np.float32(0.5)]
        out += hits[:n_per_level]
    return np.array(out, np.float32)
