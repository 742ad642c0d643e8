"""The validation report of the reference's training loop (split.py:163-257) for a loaded checkpoint: the number behind
``# Validation # PSNR: ...`` in every training log and the ``*_target.png`` / ``*_input.png`` / ``*_pred.png`` triples.

Per item the block un-normalises input, target and prediction to uint16 detector counts (truncating casts, the
prediction clipped first), takes ``core.psnr.PSNR`` per channel on those counts and, for grey data, rescales the three
images to [0, 1] with the TARGET's per-channel minimum and maximum -- in uint16, so a prediction below the target's
minimum wraps round and comes out as 1.  All of that is one call of ``dsx_val_report`` (include/dsx.h) here: the counts
and the images' numerators are written on the device, the statistics are exact integers, and the host only divides.
There is no CPU fallback.

Departure: the reference hands the float [0, 1] arrays of 'L' mode to cv2.imwrite, which stores them as
0 / 1 bytes; here such a file is a 16-bit grey PNG of rint(65535 v), in save_img's side-by-side layout.
"""
import ctypes as C
import logging
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .._lib import DsxError, check, lib

VAL_CHUNK = 4096            # DSX_VAL_CHUNK
VAL_MAX_CHANNELS = 16       # DSX_VAL_MAX_CHANNELS
logger = logging.getLogger("base")


@dataclass
class ValidationResult:
    """What ``validation_report`` returns.  Tensors are on the device, statistics are host int64 arrays."""
    mode: str                                   # 'RGB' (three input channels) or 'L'
    input_q: torch.Tensor                       # (B, Cin, H, W) uint16
    target_q: torch.Tensor                      # (B, C, H, W) uint16
    pred_q: torch.Tensor
    ssd: np.ndarray                             # (B, C) sum (target_q - pred_q)^2
    tmin: np.ndarray                            # (B, C) min / max of target_q
    tmax: np.ndarray
    imin: np.ndarray                            # (B, Cin) min / max of input_q
    imax: np.ndarray
    psnr: np.ndarray                            # (B, C) float64
    undefined: int                              # pixels without a defined uint16 value (stored as 0)
    input_n: Optional[torch.Tensor] = None      # numerators of the [0, 1] images, uint16 (visuals in 'L' mode)
    target_n: Optional[torch.Tensor] = None
    pred_n: Optional[torch.Tensor] = None
    input_img: Optional[np.ndarray] = None      # the [0, 1] images, float64
    target_img: Optional[np.ndarray] = None
    pred_img: Optional[np.ndarray] = None


def psnr_from_stats(ssd, tmin, tmax, n):
    """core/psnr.py:44-49 per plane of n pixels, in float64 from the exact integers:
    20 log10((max - min) / sqrt(ssd / n)); inf for equal images, nan for equal flat ones, as the reference's."""
    ssd, rng = np.asarray(ssd, dtype=np.float64), np.asarray(tmax, dtype=np.float64) - np.asarray(tmin, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(rng / np.sqrt(ssd / float(n)))


def visuals_from_numerators(input_n, target_n, pred_n, tmin, tmax, imin, imax):
    """The reference's float64 [0, 1] images (split.py:215-229) from the uint16 numerators (B, C, H, W) and the integer
    statistics (B, C): numerator / denominator with the denominators tmax - tmin and imax - (the item's input minimum).
    A flat plane divides by zero, as the reference does."""
    tden = (np.asarray(tmax) - np.asarray(tmin)).astype(np.uint16)[:, :, None, None]
    iden = (np.asarray(imax) - np.asarray(imin).min(axis=1, keepdims=True)).astype(np.uint16)[:, :, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return input_n / iden, target_n / tden, pred_n / tden


def _tensor(t, what, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise DsxError(f"{what} must be a CUDA tensor: the validation report runs on the MI355X only (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise DsxError(f"{what} must be a contiguous float32 (B, C, H, W) tensor, got {t.dtype} {tuple(t.shape)}"
                       f"{'' if t.is_contiguous() else ', strided'}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise DsxError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach()


def _normalisation(nd, Cn):
    mean_in, std_in = np.asarray(nd["mean_input"], dtype=np.float64), np.asarray(nd["std_input"], dtype=np.float64)
    if mean_in.size != 1 or std_in.size != 1:
        raise DsxError("mean_input / std_input must be scalars")
    mean_t = np.ascontiguousarray(np.asarray(nd["mean_target"], dtype=np.float64).reshape(-1))
    std_t = np.ascontiguousarray(np.asarray(nd["std_target"], dtype=np.float64).reshape(-1))
    if mean_t.size != Cn or std_t.size != Cn:
        raise DsxError(f"mean_target / std_target must hold one value per target channel ({Cn}), got {mean_t.size} / "
                       f"{std_t.size}")
    return float(mean_in.reshape(())), float(std_in.reshape(())), mean_t, std_t


def validation_report(input, target, prediction, normalization_dict, visuals=True):
    """split.py:182-229 for a batch: ``input`` (B, Cin, H, W), ``target`` and ``prediction`` (B, C, H, W) contiguous
    float32 CUDA tensors (each item is what the reference's loop sees with batch size 1), ``normalization_dict`` as
    ``get_normalization_dict()`` returns it.  One ``dsx_val_report`` call and one copy of the statistics to the host.
    ``visuals``: in 'L' mode also the three [0, 1] images (numerators on the device, float64 arrays on the host)."""
    input = _tensor(input, "input")
    B, Cin, H, W = input.shape
    target = _tensor(target, "target")
    if target.shape[0] != B or tuple(target.shape[2:]) != (H, W):
        raise DsxError(f"target must be ({B}, C, {H}, {W}), got {tuple(target.shape)}")
    Cn = target.shape[1]
    prediction = _tensor(prediction, "prediction", target.shape)
    if Cn > VAL_MAX_CHANNELS:
        raise DsxError(f"{Cn} target channels, at most {VAL_MAX_CHANNELS}")
    mean_in, std_in, mean_t, std_t = _normalisation(normalization_dict, Cn)
    _lib.require_gpu()
    mode = "RGB" if Cin == 3 else "L"
    dev = input.device
    u16 = lambda like: torch.empty(like.shape, dtype=torch.uint16, device=dev)
    iq, tq, pq = u16(input), u16(target), u16(prediction)
    want = bool(visuals) and mode != "RGB"
    inum, tnum, pnum = (u16(input), u16(target), u16(prediction)) if want else (None, None, None)
    nblk = (H * W + VAL_CHUNK - 1) // VAL_CHUNK
    part = torch.empty(B * (Cn + Cin) * nblk * 4, dtype=torch.int64, device=dev)
    stats = torch.empty(1 + B * (3 * Cn + 2 * Cin), dtype=torch.int64, device=dev)
    pd = C.POINTER(C.c_double)
    check(lib.dsx_val_report(input, target, prediction, B, Cin, Cn, H, W, mean_in, std_in, mean_t.ctypes.data_as(pd),
                             std_t.ctypes.data_as(pd), iq, tq, pq, inum, tnum, pnum, part, stats, None))
    st = stats.cpu().numpy()
    tst = st[1:1 + 3 * B * Cn].reshape(B, Cn, 3)
    ist = st[1 + 3 * B * Cn:].reshape(B, Cin, 2)
    res = ValidationResult(mode=mode, input_q=iq, target_q=tq, pred_q=pq, ssd=tst[..., 0].copy(), tmin=tst[..., 1].copy(),
                           tmax=tst[..., 2].copy(), imin=ist[..., 0].copy(), imax=ist[..., 1].copy(),
                           psnr=psnr_from_stats(tst[..., 0], tst[..., 1], tst[..., 2], H * W), undefined=int(st[0]))
    if want:
        res.input_n, res.target_n, res.pred_n = inum, tnum, pnum
        res.input_img, res.target_img, res.pred_img = visuals_from_numerators(
            inum.cpu().numpy(), tnum.cpu().numpy(), pnum.cpu().numpy(), res.tmin, res.tmax, res.imin, res.imax)
    return res


def group_psnr(result):
    """The reference's grouping (split.py:206-209): one key per channel in 'L' mode, one per RGB triple (the mean of
    its three channels) otherwise -> {ch_idx: [one value per item]}."""
    ncols = 3 if result.mode == "RGB" else 1
    Cn = result.psnr.shape[1]
    return {ch: [float(np.mean(row[ch:ch + ncols])) for row in result.psnr] for ch in range(0, Cn, ncols)}


def save_visual_l16(img, img_path):
    """A float [0, 1] (C, H, W) image of 'L' mode as a 16-bit grey PNG of rint(65535 v), channels side by side as
    save_img lays them out.  NaN (a flat plane's 0 / 0) is written as 0."""
    from .metrics import save_img
    v = np.nan_to_num(np.asarray(img, dtype=np.float64), nan=0.0, posinf=1.0, neginf=0.0)
    save_img(np.rint(65535.0 * np.clip(v, 0.0, 1.0)).astype(np.uint16), img_path, mode="L")


def _save_triple(res, b, stem):
    from .metrics import save_img
    if res.mode == "RGB":                       # the uint16 counts; save_img's astype(uint8) wraps as the reference's
        arrs = [t[b].cpu().numpy() for t in (res.target_q, res.input_q, res.pred_q)]
        for arr, name in zip(arrs, ("target", "input", "pred")):
            save_img(arr, f"{stem}_{name}.png", mode="RGB")
    else:
        for arr, name in ((res.target_img, "target"), (res.input_img, "input"), (res.pred_img, "pred")):
            save_visual_l16(arr[b], f"{stem}_{name}.png")


def validate(diffusion, val_set, n_items=19, batch=4, result_path=None, current_step=0, on_batch=None):
    """The validation block of the training loop for a loaded model: the first ``n_items`` items of ``val_set`` (a
    ``SplitDataset``; the reference's loop stops after 19), ``batch`` at a time, through ``tiles`` -> ``feed_data`` ->
    ``test(continuous=False)`` -> ``netG.last_full_batch`` -> ``validation_report``.  Returns
    ``(avg_psnr, {ch_idx: [per item]})`` with avg_psnr = mean over the channel keys of the mean over the items.  With
    ``result_path`` the three images of item idx (from 1) go to ``<result_path>/<current_step>_<idx>_{target,input,pred}.png``.
    ``n_items=None``: every item.  ``on_batch(first_item, prediction)`` is called with each batch's normalised
    prediction (B, C, H, W), still on the device."""
    n = len(val_set) if n_items is None else min(int(n_items), len(val_set))
    if n < 1:
        raise DsxError("validate: no items")
    if result_path is not None:
        os.makedirs(result_path, exist_ok=True)
    nd = val_set.get_normalization_dict()
    psnr_values, undefined = {}, 0
    for i0 in range(0, n, int(batch)):
        data = val_set.tiles(list(range(i0, min(n, i0 + int(batch)))))
        diffusion.feed_data(data)
        diffusion.test(continuous=False)
        pred = diffusion.netG.last_full_batch
        res = validation_report(diffusion.data["input"], diffusion.data["target"], pred.contiguous(), nd,
                                visuals=result_path is not None)
        undefined += res.undefined
        if on_batch is not None:
            on_batch(i0, pred)
        for ch, vals in group_psnr(res).items():
            psnr_values.setdefault(ch, []).extend(vals)
        if result_path is not None:
            for b in range(pred.shape[0]):
                _save_triple(res, b, os.path.join(result_path, f"{current_step}_{i0 + b + 1}"))
    if undefined:
        logger.warning("validation: %d pixels had no defined uint16 value (NaN, or counts outside [0, 65536)); they "
                       "were taken as 0", undefined)
    avg_psnr = float(np.mean([np.mean(v) for v in psnr_values.values()]))
    return avg_psnr, psnr_values
