"""Does the split add back up to the acquisition?  The one check an input-only stack allows, and the correction it gives.

The network's input is by construction ``x = sum_c w_c p_c`` in raw counts, so for the prediction ``p^`` of a stack the
residual ``r = x - sum_c w_c p^_c`` can be formed at every pixel without ground truth.  ``consistency`` computes, in ONE
HIP pass over the resident acquisition and the stitched canvases (``dsx_consistency``, include/dsx.h: bit-equal to a
float64 restatement pixel by pixel, exact counts, bounded sums, equal bits run to run), the residual map, a report per
frame, and the prediction conditioned on the observation: an independent Gaussian posterior ``N(p^_c, v_c)`` conditioned
on ``sum_c w_c t_c = x`` (noise variance ``rho^2``) moves channel c by ``v_c w_c r / (sum w^2 v + rho^2)`` and shrinks
its variance to ``v_c - v_c^2 w_c^2 / (sum w^2 v + rho^2)``.  Without a spread (``v_c = 1``, ``rho = 0``) that is the
orthogonal projection onto the constraint, which never increases the squared error to any truth satisfying it.  The
channels of the posterior are taken as independent: their sample covariance is not used.

``chi2`` needs no ground truth either: with an honest spread ``r^2 / (sum w^2 v + rho^2)`` averages 1.

Saturated pixels (``x >= clip``) only say ``sum w p >= clip``: they are left alone and counted.  Everything after the
kernel runs in float64 on the host: a report is ten numbers per frame."""
import math

import numpy as np
import torch

from .._lib import DsxError

SLOTS = 10
MAX_C = 4


def norm_arrays(norm, channels):
    """(std_target, mean_target) of ``channels`` channels, float64, from a normalisation dict."""
    try:
        mean, std = (np.asarray(norm[k], dtype=np.float64).reshape(-1) for k in ("mean_target", "std_target"))
    except (KeyError, TypeError):
        raise DsxError("consistency: the normalisation dict must provide 'mean_target' and 'std_target'")
    if mean.size != channels or std.size != channels:
        raise DsxError(f"consistency: mean_target / std_target hold {mean.size} / {std.size} values, the prediction has "
                       f"{channels} channels")
    return std, mean


def check_weights(weights, channels):
    """``weights`` (None: ones) as ``channels`` finite float64 values, not all zero."""
    w = np.ones(channels) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != channels:
        raise DsxError(f"consistency: {w.size} channel weights for a prediction of {channels} channels; the residual "
                       "x - sum_c w_c p_c needs one weight per predicted channel")
    if not np.isfinite(w).all() or not w.any():
        raise DsxError(f"consistency: channel weights {w.tolist()}: finite, and not all zero")
    return w


def check_noise(noise):
    if not (isinstance(noise, (int, float)) and math.isfinite(noise) and noise >= 0):
        raise DsxError(f"consistency: noise = {noise!r}: rho in raw counts, finite and not negative")
    return float(noise)


def _ratio(a, b):
    return None if b == 0 else a / b


def report_of_row(row, with_chi2):
    """One report from a row of the ten sums (include/dsx.h), everything in raw counts; None where a count is zero."""
    k, sat, sr, srr, sx, sxx, kd, schi, mn, mx = (float(v) for v in row)
    out = {"pixels": int(k), "saturated": int(sat)}
    out["rms"] = math.sqrt(srr / k) if k else None
    out["bias"] = sr / k if k else None
    out["relative"] = math.sqrt(srr / sxx) if k and sxx > 0 else None
    centred = sxx - sx * sx / k if k else 0.0
    out["explained"] = 1.0 - srr / centred if k and centred > 0 else None
    out["min"] = mn if k else None
    out["max"] = mx if k else None
    if with_chi2:
        out["chi2_pixels"] = int(kd)
        out["chi2"] = _ratio(schi, kd)
    return out


def fold_rows(rows):
    """The total row of (frames, 10) rows: sums added and extremes taken in frame order, in double."""
    tot = [0.0] * 8 + [math.inf, -math.inf]
    for row in np.asarray(rows, dtype=np.float64):
        for j in range(8):
            tot[j] += float(row[j])
        tot[8], tot[9] = min(tot[8], float(row[8])), max(tot[9], float(row[9]))
    return tot


def consistency(mean, acquisition, norm, weights=None, std=None, clip=None, noise=0.0, project=False, want_map=False,
                pix=None):
    """``mean`` (frames, ..., C) and ``std`` (the same shape, or None): normalised CUDA fp32 canvases as ``predict_stack``
    returns them; ``acquisition``: the (frames, ...) pixels on the device in their file width (``engine.consistency``
    says how; ``pix`` names the type when the tensor holds raw bytes); ``norm``: the normalisation dict
    (``mean_target`` / ``std_target``, one per channel); ``weights``: w_c, None = ones; ``clip``: the input clip in raw
    counts (None: none), pixels at or above it are saturated; ``noise``: rho in raw counts.

    Returns a dict: ``'frames'`` (one report per frame) and ``'total'``, each with ``pixels`` (unsaturated),
    ``saturated``, ``rms = sqrt(sum r^2 / k)``, ``bias = sum r / k``, ``relative = sqrt(sum r^2 / sum x^2)``,
    ``explained = 1 - sum r^2 / (sum x^2 - (sum x)^2 / k)``, ``min``, ``max`` and, with ``std``, ``chi2`` over
    ``chi2_pixels`` -- all in raw counts, None where a count is zero; the totals are folded from the frame rows on the
    host in frame order.  ``'rows'`` holds the (frames, 10) sums.  ``want_map``: ``'map'``, the residual (frames, ...)
    float32 in raw counts.  ``project``: ``'mean'`` and, with ``std``, ``'std'``: the conditioned canvases, normalised
    like the inputs (the inputs are left as they are)."""
    from .. import engine
    if not isinstance(mean, torch.Tensor) or mean.dim() < 2 or not 1 <= mean.shape[-1] <= MAX_C:
        got = tuple(mean.shape) if isinstance(mean, torch.Tensor) else type(mean).__name__
        raise DsxError(f"consistency: mean must be a CUDA float32 tensor (frames, ..., C) with C in 1..{MAX_C}, got {got}")
    channels = int(mean.shape[-1])
    scale, shift = norm_arrays(norm, channels)
    w = check_weights(weights, channels)
    rho = check_noise(noise)
    if clip is not None and not (math.isfinite(clip) and clip >= 0):
        raise DsxError(f"consistency: clip = {clip!r}: a finite, non-negative count (None: no clip)")
    rows, fmap, pmean, pstd = engine.consistency(
        acquisition, mean, scale, shift, w, std=std, clip=-1.0 if clip is None else float(clip), noise_var=rho * rho,
        want_row=True, want_map=want_map, want_mean=bool(project), want_std=bool(project) and std is not None, pix=pix)
    rows = rows.cpu().numpy()
    out = {"rows": rows, "weights": w.tolist(), "noise": rho, "clip": clip,
           "frames": [report_of_row(r, std is not None) for r in rows],
           "total": report_of_row(fold_rows(rows), std is not None)}
    if want_map:
        out["map"] = fmap
    if project:
        out["mean"] = pmean
        if std is not None:
            out["std"] = pstd
    return out


def json_report(report):
    """The JSON-serialisable part of ``consistency``'s dict (no tensors; the raw sums as lists)."""
    return {"weights": report["weights"], "noise": report["noise"], "clip": report["clip"], "total": report["total"],
            "frames": report["frames"], "rows": [[float(v) for v in r] for r in report["rows"]]}
