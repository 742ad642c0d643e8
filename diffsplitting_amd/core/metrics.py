"""The reference's image-quality module (core/metrics.py), same names and signatures: tensor2img, save_img,
calculate_psnr and calculate_ssim, plus ``image_metrics``, the batched device form of PSNR and SSIM,
``calculate_lpips``, the evaluation notebooks' ``compute_lpips`` on the device, and ``msssim`` / ``calculate_msssim``,
a multi-scale SSIM (``dsx_msssim``) with a range-invariant form for stitched frames that have no natural peak.

SSIM runs on the MI355X (``dsx_image_metrics``, include/dsx.h): there is no CPU fallback, so calculate_ssim raises
DsxError without a device.  The reference writes its grid with torchvision's make_grid and its files with cv2; neither
is a dependency here, so the grid is written out below and files are written with PIL, to the same pixels.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib


def _make_grid(t, nrow, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid(t, nrow, padding=2, normalize=False) of a (B, C, H, W) tensor."""
    if t.size(1) == 1:
        t = torch.cat((t, t, t), 1)
    if t.size(0) == 1:
        return t.squeeze(0)
    nmaps = t.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(t.size(2) + padding), int(t.size(3) + padding)
    grid = t.new_full((t.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(
                2, x * width + padding, width - padding).copy_(t[k])
            k += 1
    return grid


def tensor2img(tensor, out_type=np.uint8, min_max=(-1, 1)):
    """Tensor (4-D (B, 3/1, H, W) as a grid, 3-D (C, H, W) or 2-D (H, W), any range) -> HWC or HW numpy image in
    [0, 255] (core/metrics.py:8-34): clamp to min_max, to [0, 1], * 255, round half to even, uint8."""
    tensor = tensor.squeeze().float().cpu().clamp_(*min_max)
    tensor = (tensor - min_max[0]) / (min_max[1] - min_max[0])
    n_dim = tensor.dim()
    if n_dim == 4:
        img_np = _make_grid(tensor, nrow=int(math.sqrt(len(tensor)))).numpy()
        img_np = np.transpose(img_np, (1, 2, 0))
    elif n_dim == 3:
        img_np = np.transpose(tensor.numpy(), (1, 2, 0))
    elif n_dim == 2:
        img_np = tensor.numpy()
    else:
        raise TypeError(f"Only support 4D, 3D and 2D tensor. But received with dimension: {n_dim:d}")
    if out_type == np.uint8:
        img_np = (img_np * 255.0).round()
    return img_np.astype(out_type)


def save_img(img, img_path, mode='RGB'):
    """Write a channel-first image as core/metrics.py:37-59 lays it out (6-channel CIFAR pairs and 2-channel Hagen
    pairs side by side), to the pixels cv2.imwrite would write: 3-channel arrays are BGR to cv2, so they are reversed
    before PIL writes RGB; other modes write a single-channel 8- or 16-bit image."""
    from PIL import Image
    if len(img.shape) == 3 and img.shape[0] not in [1, 3]:
        if mode == 'RGB':
            img = np.transpose(img, (1, 2, 0))
            img = img.reshape((img.shape[0], img.shape[1], 2, 3))
            img = img.transpose((0, 2, 1, 3))
            img = img.reshape((img.shape[0], img.shape[1] * img.shape[2], img.shape[3]))
        else:
            img = img.transpose((1, 0, 2))
            img = img.reshape((img.shape[0], -1, 1))
    else:
        assert len(img.shape) == 3, f'img shape is {img.shape}'
        img = img.transpose((1, 2, 0))
    if mode == 'RGB':
        img = img.astype(np.uint8)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    if img.ndim == 3:
        if img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError(f"save_img writes 3-channel uint8 or 1-channel uint8/uint16 images, got {img.shape} "
                             f"{img.dtype}")
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(img_path)
    elif img.dtype in (np.uint8, np.uint16):
        Image.fromarray(np.ascontiguousarray(img)).save(img_path)          # mode L / I;16
    else:
        raise ValueError(f"save_img writes uint8 or uint16 single-channel images, got {img.dtype}")


def calculate_psnr(img1, img2):
    """PSNR of two [0, 255] images in float64 (core/metrics.py:62-69); inf when they are equal."""
    img1 = img1.astype(np.float64)
    img2 = img2.astype(np.float64)
    mse = np.mean((img1 - img2) ** 2)
    if mse == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _psnr_from_ssd(ssd, n, data_range):
    mse = ssd / n
    if mse == 0:
        return float('inf')
    return 20 * math.log10(data_range / math.sqrt(mse))


def _run(a, b, quantize, lo, hi, data_range, stream=None):
    """dsx_image_metrics on (B, C, H, W) fp32 CUDA tensors -> (ssim [B], ssd [B]) float64 numpy arrays."""
    _lib.require_gpu()
    B, Cn, H, W = a.shape
    blocks = check(lib.dsx_image_metrics_blocks(H, W))
    part = torch.empty((B * Cn * blocks * 2,), dtype=torch.float64, device=a.device)
    ssim = np.empty(B, np.float64)
    ssd = np.empty(B, np.float64)
    pd = C.POINTER(C.c_double)
    check(lib.dsx_image_metrics(a, b, B, Cn, H, W, int(quantize), float(lo), float(hi), float(data_range), part,
                                ssim.ctypes.data_as(pd), ssd.ctypes.data_as(pd), stream))
    return ssim, ssd


def calculate_ssim(img1, img2):
    """SSIM of two [0, 255] images (core/metrics.py:95-113): 2-D, H x W x 1 or H x W x 3 (the mean over the valid
    region of all three channels, as the reference's three calls of ssim() on the whole array give).  Computed on
    the device from the images' fp32 values, with the reference's constants (L = 255)."""
    if not img1.shape == img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    if img1.ndim == 2:
        a, b = img1[None], img2[None]
    elif img1.ndim == 3 and img1.shape[2] in (1, 3):
        a, b = np.transpose(img1, (2, 0, 1)), np.transpose(img2, (2, 0, 1))
    else:
        raise ValueError('Wrong input image dimensions.')
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(dev)
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32))[None].to(dev)
    ssim, _ = _run(ta, tb, False, 0.0, 1.0, 255.0)
    return float(ssim[0])


def image_metrics(pred, target, min_max=(-1, 1), quantize=True, data_range=255.0, stream=None):
    """Per-image (psnr, ssim) of two (B, C, H, W) CUDA tensors in one launch, float64 CPU tensors of length B.

    quantize=True: for every i, equal to calculate_psnr(tensor2img(pred[i], min_max=min_max), tensor2img(target[i],
    min_max=min_max)) (bit-equal) and the matching calculate_ssim (the mean over all C channels) at the default
    data_range = 255, the reference's peak and L.  quantize=False: PSNR and SSIM of the raw fp32 values with
    peak = L = data_range (stitched prediction frames)."""
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"pred and target must be (B, C, H, W) of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    a = pred.to(torch.float32).contiguous()
    b = target.to(torch.float32).contiguous()
    ssim, ssd = _run(a, b, quantize, min_max[0], min_max[1], data_range, stream)
    n = a.shape[1] * a.shape[2] * a.shape[3]
    psnr = [_psnr_from_ssd(s, n, float(data_range)) for s in ssd.tolist()]
    return torch.tensor(psnr, dtype=torch.float64), torch.from_numpy(ssim)


def calculate_lpips(target_stitched, pred_stitched, loss_fn, chunk=0):
    """``compute_lpips(target, pred)`` of notebooks/EvaluateJointIndi.ipynb cell 31 / EvaluateJointIndiIterative.ipynb
    cell 28 on (N, H, W, C) channel-last frames: per channel, both stacks mapped to [-1, 1] with the TARGET channel's
    min / max over all frames, replicated to three channels, LPIPS per frame -> {channel: [N floats]}.  ``loss_fn`` is a
    ``core.lpips.LPIPS``; everything runs on the device (``dsx_lpips_frames``), numpy input is uploaded once."""
    _lib.require_gpu()
    dev = next((t.device for t in (target_stitched, pred_stitched) if torch.is_tensor(t) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    up = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).to(
        dev, torch.float32).contiguous()
    t, p = up(target_stitched), up(pred_stitched)
    if t.shape != p.shape or t.dim() != 4:
        raise ValueError(f"target and pred must be (N, H, W, C) of one shape, got {tuple(t.shape)} and {tuple(p.shape)}")
    return {ch: loss_fn.frames(t, p, ch, chunk).tolist() for ch in range(t.shape[3])}


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003


def msssim_min_side(scales):
    """The smallest admissible side for ``scales`` scales: the coarsest scale still holds the 11 x 11 window."""
    return 11 << (scales - 1)


def check_msssim_size(H, W, scales):
    """The size rule of ``dsx_msssim`` on the host: min(H, W) >> (scales - 1) >= 11, else ValueError."""
    if min(H, W) >> (scales - 1) < 11:
        raise ValueError(f"MS-SSIM with {scales} scales needs min(H, W) >= {msssim_min_side(scales)} (the coarsest scale "
                         f"still holds the 11 x 11 window), got {H} x {W}")


def _check_msssim_args(pred_shape, target_shape, data_range, range_invariant, weights):
    """Every refusal of ``msssim`` that needs no device -> the weights as a tuple of floats."""
    if tuple(pred_shape) != tuple(target_shape) or len(pred_shape) != 4:
        raise ValueError(f"pred and target must be (B, C, H, W) of one shape, got {tuple(pred_shape)} and "
                         f"{tuple(target_shape)}")
    weights = tuple(float(w) for w in weights)
    if not 1 <= len(weights) <= 5:
        raise ValueError(f"weights: one per scale, 1 to 5 of them, got {len(weights)}")
    if not all(math.isfinite(w) and w > 0 for w in weights):
        raise ValueError(f"weights must be positive, got {weights}")
    if range_invariant and data_range is not None:
        raise ValueError("data_range and range_invariant both name the dynamic range: give one (the range-invariant "
                         "form takes L from the target plane)")
    if not range_invariant and data_range is None:
        raise ValueError("give data_range (the dynamic range L) or range_invariant=True")
    if data_range is not None and not (math.isfinite(data_range) and data_range > 0):
        raise ValueError(f"data_range must be positive, got {data_range}")
    check_msssim_size(pred_shape[2], pred_shape[3], len(weights))
    return weights


def _msssim_means(pred, target, scales, range_invariant, data_range, stream=None, workspace=None):
    """dsx_msssim on (B, C, H, W) fp32 CUDA tensors -> the (B, C, scales, 2) means {cs_s, ssim_s}, float64 numpy.
    ``workspace``: a CUDA tensor of at least B * C * dsx_msssim_workspace(H, W, scales) bytes (default: a fresh one;
    its contents on entry do not matter)."""
    B, Cn, H, W = pred.shape
    need = check(lib.dsx_msssim_workspace(H, W, scales)) * B * Cn
    if workspace is None:
        workspace = torch.empty((need // 8,), dtype=torch.float64, device=pred.device)
    out = np.empty((B, Cn, scales, 2), np.float64)
    check(lib.dsx_msssim(pred, target, B * Cn, H, W, scales, int(bool(range_invariant)), float(data_range or 0.0),
                         workspace, workspace.numel() * workspace.element_size(), out, stream))
    return out


def msssim_from_means(means, weights):
    """prod_{s < S-1} max(cs_s, 0)^w_s * max(ssim_{S-1}, 0)^w_{S-1} in float64 from (..., S, 2) means {cs_s, ssim_s}."""
    means = np.asarray(means, np.float64)
    S = len(weights)
    terms = np.concatenate([means[..., :S - 1, 0], means[..., S - 1:S, 1]], axis=-1)
    return np.prod(np.maximum(terms, 0.0) ** np.asarray(weights, np.float64), axis=-1)


def msssim(pred, target, data_range=None, range_invariant=False, weights=MSSSIM_WEIGHTS, stream=None,
           return_scales=False):
    """Multi-scale SSIM of two (B, C, H, W) CUDA tensors, per plane -> a (B, C) float64 CPU tensor; with
    ``return_scales`` also the (B, C, S, 2) per-scale means {cs_s, ssim_s} it is formed from.  The definition is
    ``dsx_msssim``'s (include/dsx.h): 11-tap Gaussian window over the valid region, 2 x 2 mean pooling in double between
    the scales, S = len(weights) <= 5 scales, weights used as given (a shorter tuple means fewer scales, nothing is
    renormalised), min(H, W) >> (S - 1) >= 11.

    ``data_range``: the dynamic range L of c1 = (0.01 L)^2, c2 = (0.03 L)^2.  ``range_invariant=True`` (the form for
    microscopy frames, which have no natural peak) instead applies ``RangeInvariantPsnr``'s transform per plane first:
    the target standardised, the prediction centred and scaled by the least-squares alpha, L = (max - min) / std of the
    target; exactly one of the two is given.  A plane whose target is constant (std 0) or whose prediction is constant
    (sum p~ p~ = 0) gives NaN for that plane, not an error.  No CPU fallback: CPU tensors raise DsxError."""
    weights = _check_msssim_args(pred.shape, target.shape, data_range, range_invariant, weights)
    if not (pred.is_cuda and target.is_cuda):
        raise DsxError(f"msssim runs on the device: pred is on {pred.device}, target on {target.device}")
    _lib.require_gpu()
    a = pred.to(torch.float32).contiguous()
    b = target.to(torch.float32).contiguous()
    means = _msssim_means(a, b, len(weights), range_invariant, data_range, stream)
    value = torch.from_numpy(msssim_from_means(means, weights))
    return (value, torch.from_numpy(means)) if return_scales else value


def calculate_msssim(target_stitched, pred_stitched, weights=MSSSIM_WEIGHTS):
    """Range-invariant MS-SSIM of (N, H, W, C) channel-last frames, numpy or CUDA -> {channel: [N floats]}, mirroring
    ``calculate_lpips``: every (frame, channel) plane scored on its own by ``msssim(range_invariant=True)``, so raw
    counts and normalised frames score the same up to input rounding.  numpy input is uploaded once."""
    if tuple(target_stitched.shape) != tuple(pred_stitched.shape) or len(target_stitched.shape) != 4:
        raise ValueError(f"target and pred must be (N, H, W, C) of one shape, got {tuple(target_stitched.shape)} and "
                         f"{tuple(pred_stitched.shape)}")
    N, H, W, Cn = target_stitched.shape
    _check_msssim_args((N, Cn, H, W), (N, Cn, H, W), None, True, weights)
    _lib.require_gpu()
    dev = next((t.device for t in (target_stitched, pred_stitched) if torch.is_tensor(t) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    up = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).to(
        dev, torch.float32).permute(0, 3, 1, 2).contiguous()
    value = msssim(up(pred_stitched), up(target_stitched), range_invariant=True, weights=weights)
    return {ch: value[:, ch].tolist() for ch in range(Cn)}


def calculate_calibration(gt_frames, mean, std, bins=30, z=(1, 2, 3), edges=None):
    """The calibration curve of a predicted spread (core/calibration.py), the face beside ``calculate_msssim``:
    ``gt_frames``, ``mean`` and ``std`` are (N, H, W, C) channel-last frames, numpy or CUDA, in ONE normalisation (the
    stitched canvases of ``predict_stack(..., samples=N, return_std=True)`` against
    ``val_set.normalized_target_frames()``).  Returns ``calibration_stats``' object: per channel the equal-count bins
    of ``std`` with their rmv and rmse, and the coverage of the intervals ``mean +- z std``.  numpy input is uploaded
    once."""
    from .calibration import calibration_stats
    shapes = [tuple(x.shape) for x in (gt_frames, mean, std)]
    if len(set(shapes)) != 1 or len(shapes[0]) != 4:
        raise ValueError(f"gt_frames, mean and std must be (N, H, W, C) of one shape, got {shapes}")
    _lib.require_gpu()
    dev = next((t.device for t in (gt_frames, mean, std) if torch.is_tensor(t) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    up = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).to(
        dev, torch.float32).contiguous()
    return calibration_stats(up(mean), up(std), up(gt_frames), bins=bins, z=z, edges=edges)
