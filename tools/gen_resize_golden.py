#!/usr/bin/env python3
"""Writes tests/golden/resize_pil.npz: what PIL's own ``Image.resize`` gives for prepare_data.resize_multiple, the
expected bytes of tests/test_resize_cpu.py and tests/test_gpu_resize.py.

    python tools/gen_resize_golden.py

The inputs are not stored: a test regenerates them from the case's seed (``make_input`` below, restated in
tests/test_resize_cpu.py).  Full cases store the lr / hr / sr bytes; digest cases (the large ones) store the SHA-256 of
each output and a strided 32 x 32 grid of it.  The size and crop arithmetic is tests/resize_ref.py's restatement of
torchvision's (torchvision is not a dependency); the resampling is PIL's.
"""
import hashlib
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resize_ref as R  # noqa: E402

# name, seed (None: ramp), H, W, mode, filter, sizes, full bytes or digest
CASES = [
    ("celeba_bicubic", 1, 218, 178, "RGB", R.BICUBIC, (16, 128), "full"),
    ("celeba_bilinear", 1, 218, 178, "RGB", R.BILINEAR, (16, 128), "full"),
    ("square_bicubic", 2, 256, 256, "RGB", R.BICUBIC, (16, 128), "full"),
    ("wide_bicubic", 3, 200, 300, "RGB", R.BICUBIC, (16, 128), "full"),
    ("wide_grey_bicubic", 3, 200, 300, "L", R.BICUBIC, (16, 128), "full"),
    ("small_bicubic", 4, 97, 131, "RGB", R.BICUBIC, (16, 128), "full"),
    ("small_bilinear", 4, 97, 131, "RGB", R.BILINEAR, (16, 128), "full"),
    ("ramp_bicubic", None, 256, 256, "RGB", R.BICUBIC, (16, 128), "full"),
    ("large_bicubic", 5, 1024, 768, "RGB", R.BICUBIC, (64, 512), "digest"),
    ("large_bilinear", 5, 1024, 768, "RGB", R.BILINEAR, (64, 512), "digest"),
]


def make_input(seed, h, w, mode):
    c = 3 if mode == "RGB" else 1
    if seed is None:      # ramp: a different slope per channel, wrapping
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * (ch + 1) + y * (3 - ch)) % 256 for ch in range(c)], axis=-1).astype(np.uint8)
    else:
        a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    return a if c == 3 else a[:, :, 0]


def pil_resize_and_convert(img, size, kind):
    """prepare_data.resize_and_convert with PIL's resize and the restated torchvision arithmetic."""
    w, h = img.size
    if w == size:
        return img
    if min(h, w) != size:
        oh, ow = R.resize_size(h, w, size)
        img = img.resize((ow, oh), kind)
    w, h = img.size
    top, left = R.crop_offsets(h, w, size)
    return img.crop((left, top, left + size, top + size))


def grid(a, size):
    s = size // 32 if size >= 32 else 1
    return np.ascontiguousarray(a[::s, ::s][:32, :32])


def main():
    out, meta = {}, []
    for i, (name, seed, h, w, mode, kind, sizes, how) in enumerate(CASES):
        img = Image.fromarray(make_input(seed, h, w, mode))
        lr = pil_resize_and_convert(img, sizes[0], kind)
        hr = pil_resize_and_convert(img, sizes[1], kind)
        sr = pil_resize_and_convert(lr, sizes[1], kind)
        m = dict(name=name, seed=seed, h=h, w=w, mode=mode, filter=kind, sizes=list(sizes), how=how)
        for key, im in (("lr", lr), ("hr", hr), ("sr", sr)):
            a = np.asarray(im)
            if how == "full":
                out[f"c{i}_{key}"] = a
            else:
                m[f"sha256_{key}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
                m[f"shape_{key}"] = list(a.shape)
                out[f"c{i}_{key}_grid"] = grid(a, a.shape[0])
        meta.append(m)
    out["meta"] = np.frombuffer(json.dumps(dict(pil_version=PIL.__version__, cases=meta)).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "resize_pil.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
