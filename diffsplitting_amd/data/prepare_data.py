#!/usr/bin/env python3
"""``data/prepare_data.py`` of the reference on the device: ``resize_and_convert`` / ``resize_multiple`` (:17-40) and
``prepare`` with the ``__main__`` flags (:161-182).

    python -m diffsplitting_amd.data.prepare_data --path <images> --out dataset/celebahq --size 16,128

The resampling is PIL's ``Image.resize`` restated as HIP kernels (``dsx_resize_u8``, include/dsx.h: fixed-point integer
arithmetic, equal to PIL byte for byte), on batches of images of one size.  The size arithmetic around it is
torchvision's ``resize`` (int size) and ``center_crop``, restated: the smaller edge goes to ``size``, the other to
``int(size * long / short)``, an image whose smaller edge already is ``size`` is not resampled, and the crop offsets are
``int(round((h - size) / 2.0))``.  PARITY UNPINNED AGAINST TORCHVISION for these three lines: torchvision is not a
dependency and was not available to compare with.

``--lmdb`` is refused by name (lmdb is not a dependency); ``n_worker`` is accepted and ignored: one process, images
batched by size.  Files are read and written through PIL.
"""
import argparse
import ctypes as C
import os
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib
from . import util as Util

BILINEAR, BICUBIC = _lib.RESIZE_BILINEAR, _lib.RESIZE_BICUBIC      # the values of PIL.Image.BILINEAR / BICUBIC
_MAX_BATCH = 65535


def resize_size(h, w, size):
    """torchvision ``resize(img, size: int)``: (new_h, new_w)."""
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def crop_offsets(h, w, size):
    """torchvision ``center_crop``: (top, left)."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def geometry(h, w, size):
    """What ``resize_and_convert`` does to an h x w image: None (left untouched: its width already is ``size``), or
    (resized_h, resized_w, crop_top, crop_left)."""
    if w == size:
        return None
    oh, ow = (h, w) if min(h, w) == size else resize_size(h, w, size)
    return (oh, ow) + crop_offsets(oh, ow, size)


class _Plan:
    """A ``dsx_resize_plan``: the coefficient tables of one (source size, target size, filter), uploaded once."""

    def __init__(self, in_h, in_w, oh, ow, top, left, size, resample, channels):
        self.handle = C.c_void_p()
        check(lib.dsx_resize_plan_create(in_h, in_w, oh, ow, top, left, size, size, int(resample), channels,
                                         C.byref(self.handle)))

    def __del__(self):
        if getattr(self, "handle", None):
            lib.dsx_resize_plan_destroy(self.handle)
            self.handle = None


_PLANS = {}


def _plan(in_h, in_w, size, resample, channels):
    key = (in_h, in_w, size, int(resample), channels)
    if key not in _PLANS:
        oh, ow, top, left = geometry(in_h, in_w, size)
        _PLANS[key] = _Plan(in_h, in_w, oh, ow, top, left, size, resample, channels)
    return _PLANS[key]


def _resize_batch(t, size, resample):
    """resize_and_convert on a (B, H, W, C) uint8 CUDA tensor -> (B, size, size, C), or ``t`` itself when untouched."""
    B, H, W, Cn = t.shape
    if geometry(H, W, size) is None:
        return t
    _lib.require_gpu()
    plan = _plan(H, W, size, resample, Cn)
    out = torch.empty((B, size, size, Cn), dtype=torch.uint8, device=t.device)
    for b0 in range(0, B, _MAX_BATCH):
        n = min(_MAX_BATCH, B - b0)
        ws_bytes = lib.dsx_resize_workspace_bytes(plan.handle, n)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=t.device)
        check(lib.dsx_resize_u8(plan.handle, t[b0:b0 + n], n, out[b0:b0 + n], ws, None))
    return out


def _open(img):
    """-> ((B, H, W, C) uint8 CUDA tensor, function that gives a result back in the caller's form)."""
    if torch.is_tensor(img):
        if img.dim() != 4:
            raise DsxError(f"a tensor input is a (B, H, W, C) uint8 batch, got {tuple(img.shape)}")
        return Util.to_device_u8(img), lambda t: t
    if isinstance(img, np.ndarray):
        grey = img.ndim == 2
        return Util.to_device_u8(img).unsqueeze(0), lambda t: t[0, :, :, 0].cpu().numpy() if grey else t[0].cpu().numpy()
    from PIL import Image
    if img.mode not in ("RGB", "L"):
        raise DsxError(f"the device resize takes RGB or L images, got mode {img.mode}: convert('RGB') first")
    grey = img.mode == "L"
    return (Util.to_device_u8(img).unsqueeze(0),
            lambda t: Image.fromarray(t[0, :, :, 0].cpu().numpy() if grey else t[0].cpu().numpy()))


def resize_and_convert(img, size, resample):
    """prepare_data.py:17-21: the smaller edge to ``size`` with PIL's ``resample`` filter, then the centre crop."""
    t, back = _open(img)
    return back(_resize_batch(t, size, resample))


def resize_multiple(img, sizes=(16, 128), resample=BICUBIC, lmdb_save=False):
    """prepare_data.py:30-40 on the device: ``[lr, hr, sr]`` with sr made from lr's uint8 bytes.  ``img`` is a PIL image
    (RGB or L), an (H, W, 3) uint8 array or a (B, H, W, 3) uint8 CUDA tensor; the results come back in the same form."""
    if lmdb_save:
        raise DsxError("resize_multiple(lmdb_save=True): lmdb output is out of scope (lmdb is not a dependency)")
    t, back = _open(img)
    lr = _resize_batch(t, sizes[0], resample)
    hr = _resize_batch(t, sizes[1], resample)
    sr = _resize_batch(lr, sizes[1], resample)
    return [back(lr), back(hr), back(sr)]


def prepare(img_path, out_path, n_worker, sizes=(16, 128), resample=BICUBIC, lmdb_save=False, batch=64):
    """prepare_data.py:100-159 without lmdb: every image file under ``img_path`` -> ``lr_{l}/``, ``hr_{r}/`` and
    ``sr_{l}_{r}/`` under ``out_path``, named by the file's stem zero-filled to five characters.  ``n_worker`` is
    ignored: images of one size are resized as batches on the device.  Returns the number of images written."""
    from PIL import Image
    if lmdb_save:
        raise DsxError("prepare(lmdb_save=True) / --lmdb: lmdb output is out of scope (lmdb is not a dependency); the "
                       "PNG folders are what LRHRDataset(datatype='img') reads")
    files = sorted(p for p in Path('{}'.format(img_path)).glob('**/*') if p.is_file() and Util.is_image_file(p.name))
    if not files:
        raise DsxError('{:s} has no valid image file'.format(str(img_path)))
    dirs = ['{}/lr_{}'.format(out_path, sizes[0]), '{}/hr_{}'.format(out_path, sizes[1]),
            '{}/sr_{}_{}'.format(out_path, sizes[0], sizes[1])]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    groups = {}                                      # images batched by size, in file order
    total = 0

    def flush(key):
        names, arrays = groups.pop(key)
        t = Util.to_device_u8(torch.from_numpy(np.stack(arrays)))
        outs = [o.cpu().numpy() for o in resize_multiple(t, sizes=sizes, resample=resample)]
        for k, name in enumerate(names):
            for d, o in zip(dirs, outs):
                Image.fromarray(o[k]).save('{}/{}.png'.format(d, name.zfill(5)))
        return len(names)

    for f in files:
        a = np.asarray(Image.open(f).convert('RGB'))
        names, arrays = groups.setdefault(a.shape, ([], []))
        names.append(f.name.split('.')[0])
        arrays.append(a)
        if len(names) >= batch:
            total += flush(a.shape)
    for key in list(groups):
        total += flush(key)
    return total


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--path', '-p', type=str, default='{}/Dataset/celebahq_256'.format(Path.home()))
    parser.add_argument('--out', '-o', type=str, default='./dataset/celebahq')
    parser.add_argument('--size', type=str, default='64,512')
    parser.add_argument('--n_worker', type=int, default=3)
    parser.add_argument('--resample', type=str, default='bicubic')
    parser.add_argument('--lmdb', '-l', action='store_true')
    args = parser.parse_args(argv)
    resample = {'bilinear': BILINEAR, 'bicubic': BICUBIC}[args.resample]
    sizes = [int(s.strip()) for s in args.size.split(',')]
    args.out = '{}_{}_{}'.format(args.out, sizes[0], sizes[1])
    n = prepare(args.path, args.out, args.n_worker, sizes=sizes, resample=resample, lmdb_save=args.lmdb)
    print('{} images written to {}'.format(n, args.out))


if __name__ == '__main__':
    main()
