"""``data/util.py`` of the reference: the image-folder helpers (host, :7-24) and ``transform_augment`` (:74-83) on the
device.

``transform_augment`` is torchvision's ``ToTensor`` followed by ``img * (max - min) + min``; here one HIP launch
(``dsx_u8_to_tensor``, include/dsx.h) turns uint8 HWC bytes into fp32 CHW on the device, bitwise equal to what torch
computes on the CPU.  The ``split='train'`` branch (a random horizontal flip) is training-time augmentation and raises
``DsxError``: the engine is inference-only.
"""
import os

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib

IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG',
                  '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP']


def is_image_file(filename):
    return any(filename.endswith(extension) for extension in IMG_EXTENSIONS)


def get_paths_from_images(path):
    assert os.path.isdir(path), '{:s} is not a valid directory'.format(path)
    images = []
    for dirpath, _, fnames in sorted(os.walk(path)):
        for fname in sorted(fnames):
            if is_image_file(fname):
                img_path = os.path.join(dirpath, fname)
                images.append(img_path)
    assert images, '{:s} has no valid image file'.format(path)
    return sorted(images)


def to_device_u8(img, device=None):
    """PIL image, (H, W[, C]) uint8 array or uint8 tensor -> contiguous uint8 CUDA tensor, channel-last; a 2-D image
    gets a channel axis, an alpha channel is dropped (transform2numpy, data/util.py:45-53)."""
    if not torch.is_tensor(img):
        a = np.array(img)                 # a writable copy (PIL hands out read-only views)
        if a.dtype != np.uint8:
            raise DsxError(f"the image path takes 8-bit images, got {a.dtype}")
        img = torch.from_numpy(np.ascontiguousarray(a))
    if img.dtype != torch.uint8:
        raise DsxError(f"the image path takes uint8 tensors, got {img.dtype}")
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    if img.shape[-1] > 3:
        img = img[..., :3]
    if not img.is_cuda:
        _lib.require_gpu()
        img = img.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return img.contiguous()


def u8_to_tensor(u8, min_max=(0, 1)):
    """(H, W, C) or (B, H, W, C) uint8 CUDA tensor -> (C, H, W) or (B, C, H, W) fp32: u / 255 * (max - min) + min."""
    _lib.require_gpu()
    single = u8.dim() == 3
    t = u8.unsqueeze(0) if single else u8
    if t.dim() != 4 or t.shape[3] not in (1, 3):
        raise DsxError(f"u8_to_tensor takes (B, H, W, 1 or 3) uint8, got {tuple(u8.shape)}")
    B, H, W, Cn = t.shape
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=t.device)
    check(lib.dsx_u8_to_tensor(t, B, H, W, Cn, float(min_max[0]), float(min_max[1]), out, None))
    return out[0] if single else out


def transform_augment(img_list, split='val', min_max=(0, 1)):
    """data/util.py:74-83 for uint8 device tensors ((H, W, C), or (B, H, W, C) batches) or PIL images -> fp32 CHW device
    tensors in ``min_max``."""
    if split == 'train':
        raise DsxError("transform_augment(split='train'): the random flip is training-time augmentation, out of scope "
                       "of the MI355X sampling engine; use split='val'")
    return [u8_to_tensor(to_device_u8(img), min_max) for img in img_list]
