"""PIL's 8-bit antialiased resampler (``Image.resize`` with BILINEAR or BICUBIC: libImaging/Resample.c) restated with
numpy integers, the torchvision size / centre-crop arithmetic the reference's ``prepare_data.resize_and_convert`` goes
through, and ``ToTensor`` + ``min_max`` in float32.  The expected values of tests/test_resize_cpu.py and
tests/test_gpu_resize.py come from here and from tests/golden/resize_pil.npz (written by PIL itself).

PARITY UNPINNED against torchvision for ``resize_size`` / ``crop_offsets``: torchvision is not installed, the three
lines restate ``transforms.functional.resize`` (int size) and ``center_crop``.
"""
import numpy as np

BILINEAR, BICUBIC = 2, 3            # PIL.Image.BILINEAR / BICUBIC
PRECISION_BITS = 32 - 8 - 2
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}


def _filter(kind, x):
    x = abs(x)
    if kind == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size, kind):
    """precompute_coeffs + normalize_coeffs_8bpc -> (xmin [out], n [out], k [out][ksize] int64, zero padded)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[kind] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin, n, k = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        w = [_filter(kind, (x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], n[xx] = lo, hi - lo
        k[xx, :hi - lo] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, n, k


def _pass(img, out_size, kind, axis):
    """One pass along `axis` (0 rows, 1 columns) of an (H, W, C) uint8 image; skipped when the length stays."""
    if img.shape[axis] == out_size:
        return img
    xmin, n, k = coeffs(img.shape[axis], out_size, kind)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        kk = k[xx, :n[xx]].reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = (1 << (PRECISION_BITS - 1)) + (src[xmin[xx]:xmin[xx] + n[xx]] * kk).sum(0)
    return np.moveaxis(np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize(img, out_h, out_w, kind):
    """Image.resize((out_w, out_h), kind) of an (H, W, C) or (H, W) uint8 array: horizontal, then vertical, with the
    uint8 intermediate."""
    a = img[:, :, None] if img.ndim == 2 else img
    out = _pass(_pass(a, out_w, kind, 1), out_h, kind, 0)
    return out[:, :, 0] if img.ndim == 2 else out


def resize_size(h, w, size):
    """torchvision resize with an int size: the smaller edge -> size, the other -> int(size * long / short)."""
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def crop_offsets(h, w, size):
    """torchvision center_crop: (top, left)."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def resize_and_convert(img, size, kind):
    """prepare_data.resize_and_convert on an (H, W, C) uint8 array (PIL's img.size[0] is the width)."""
    h, w = img.shape[:2]
    if w == size:
        return img
    if min(h, w) != size:
        oh, ow = resize_size(h, w, size)
        img = resize(img, oh, ow, kind)
    h, w = img.shape[:2]
    top, left = crop_offsets(h, w, size)
    return img[top:top + size, left:left + size]


def resize_multiple(img, sizes=(16, 128), kind=BICUBIC):
    lr = resize_and_convert(img, sizes[0], kind)
    hr = resize_and_convert(img, sizes[1], kind)
    sr = resize_and_convert(lr, sizes[1], kind)
    return [lr, hr, sr]


def to_tensor(u8_hwc, min_max=(0, 1)):
    """ToTensor then the min_max map of data/util.py:74-83, float32 throughout -> (C, H, W)."""
    a = u8_hwc[:, :, None] if u8_hwc.ndim == 2 else u8_hwc
    v = np.transpose(a, (2, 0, 1)).astype(np.float32) / np.float32(255.0)
    return (v * np.float32(min_max[1] - min_max[0]) + np.float32(min_max[0])).astype(np.float32)
