"""The quality metrics the reference reports (core/psnr.py:44-82), on whatever device
the tensors live on: PSNR and the range-invariant PSNR of grayscale image batches (B,H,W).

``comoments`` / ``range_invariant_psnr_curve``: RangeInvariantPsnr(g, a p1 + b p2) for ANY weights from one pass over
the three planes (``dsx_comoments``, include/dsx.h) -- the scan of core/psnr_based_t_refinement.py:41-57 in closed form.
``range_invariant_psnr_from_sums``: the same metric from the raw sums taken while tiles are pasted or blended."""
import ctypes as C

import torch


def _flat(x):
    return x.reshape(x.shape[0], -1).to(torch.float32)


def _psnr(gt, pred, rng):
    mse = torch.mean((gt - pred) ** 2, dim=1)
    return 20 * torch.log10(rng / torch.sqrt(mse))


def PSNR(gt, pred, range_=None):
    assert gt.dim() == 3, "Images must be in shape: (batch,H,W)"
    gt, pred = _flat(torch.as_tensor(gt)), _flat(torch.as_tensor(pred))
    if range_ is None:
        range_ = gt.max(dim=1).values - gt.min(dim=1).values
    return _psnr(gt, pred, range_)


def RangeInvariantPsnr(gt, pred):
    """Rescales the prediction (least squares against the standardised ground truth)
    before computing PSNR (core/psnr.py:70-82)."""
    assert gt.dim() == 3, "Images must be in shape: (batch,H,W)"
    gt, pred = _flat(torch.as_tensor(gt)), _flat(torch.as_tensor(pred))
    std = gt.std(dim=1, keepdim=True)
    ra = (gt.max(dim=1).values - gt.min(dim=1).values) / std[:, 0]
    g = (gt - gt.mean(dim=1, keepdim=True)) / std
    g = g - g.mean(dim=1, keepdim=True)
    p = pred - pred.mean(dim=1, keepdim=True)
    alpha = (g * p).sum(dim=1, keepdim=True) / (p * p).sum(dim=1, keepdim=True)
    return _psnr(g, alpha * p, ra)


def range_invariant_psnr_from_sums(sp, spp, sg, sgg, sgp, gmin, gmax, n):
    """``RangeInvariantPsnr`` above in closed form from the raw plane sums the paste and blend kernels take (PsnrSums,
    csrc/dsx_reduce.h).  With g_ = (g - mean g) / std g (unbiased std, as torch.std) and
    p0 = p - mean p:  alpha = <g_, p0> / <p0, p0>,  mse = (<g_, g_> - <g_, p0>^2 / <p0, p0>) / n,
    PSNR = 20 log10( ((max g - min g) / std g) / sqrt(mse) ).
    ``range_invariant_psnr_curve`` below is the same form on centred moments: Cgg = sgg - n mean_g^2,
    Cgp = sgp - n mean_g mean_p, Cpp = spp - n mean_p^2; k_msssim_coef (csrc/dsx_msssim.hip) states it on the device."""
    mean_g, mean_p = sg / n, sp / n
    var_g = (sgg - n * mean_g * mean_g) / (n - 1.0)
    std_g = torch.sqrt(var_g)
    gg = (sgg - n * mean_g * mean_g) / var_g                        # = n - 1
    gp = (sgp - n * mean_g * mean_p) / std_g
    pp = spp - n * mean_p * mean_p
    mse = (gg - gp * gp / pp) / n
    ra = (gmax - gmin) / std_g
    return 20.0 * torch.log10(ra / torch.sqrt(mse))


MOMENT_NAMES = ("n", "min_g", "max_g", "mean_g", "mean_p1", "mean_p2", "Cgg", "C11", "C22", "Cg1", "Cg2", "C12")


def comoments(g, p1, p2):
    """The centred second moments of plane triples, one HIP pass (``dsx_comoments``): ``g``, ``p1``, ``p2`` are CUDA fp32
    tensors (planes, ...) of equal shape, read in place -- contiguous, or views whose dimensions behind the first
    collapse into one stride (a channel of a (b, 2, p, p) tensor, a channel of a channel-last canvas).  Returns
    (planes, 12) float64 on the device, the columns of ``MOMENT_NAMES``; nothing is synchronised."""
    from .. import _lib
    views = [_lib.plane_view(t, f"comoments: {name}") for t, name in ((g, "g"), (p1, "p1"), (p2, "p2"))]
    _lib.common_device("comoments", [t.device for t in (g, p1, p2)])
    planes, n = views[0][1], views[0][2]
    if any(v[1:3] != (planes, n) for v in views[1:]):
        raise _lib.DsxError(f"comoments: {[tuple(t.shape) for t in (g, p1, p2)]}: three stacks of equally many planes of "
                            "equally many pixels")
    out = torch.empty((planes, 12), dtype=torch.float64, device=g.device)
    if planes == 0:
        return out
    blocks = _lib.check(_lib.lib.dsx_comoments_blocks(n))
    part = torch.empty((planes, blocks, 12), dtype=torch.float64, device=g.device)
    strides = (C.c_int64 * 6)(*[s for v in views for s in v[3:5]])
    _lib.check(_lib.lib.dsx_comoments(views[0][0], views[1][0], views[2][0], planes, n, strides, part, out, None))
    return out


def range_invariant_psnr_curve(moments, a, b):
    """RangeInvariantPsnr(g, a_j p1 + b_j p2) for every weight pair, from ``moments`` (planes, 12) alone -> (curve
    (planes, len(a)) float64, t_star (planes,) float64), on the device of ``moments``.  With ddof = 1, as the metric:

        var = Cgg / (n - 1);  gp = a Cg1 + b Cg2;  pp = a^2 C11 + 2 a b C12 + b^2 C22
        mse = ((n - 1) - gp^2 / (var pp)) / n;  PSNR = 10 log10((max g - min g)^2 / var / mse)

    (``range_invariant_psnr_from_sums`` is this form for one prediction on raw sums: Cgg = sum g^2 - n mean_g^2, ...)
    NaN where min g == max g or pp <= 0; an mse below 0 (rounding, at a fit that is exact) counts as 0: +inf dB.
    ``t_star``: the continuous maximiser over p = t p1 + (1 - t) p2, u = S^-1 c
    with S = [[C11, C12], [C12, C22]], c = (Cg1, Cg2), t* = u0 / (u0 + u1); NaN when S is singular or u0 + u1 == 0, not
    clamped to [0, 1]."""
    m = torch.as_tensor(moments, dtype=torch.float64)
    a = torch.as_tensor(a, dtype=torch.float64, device=m.device).reshape(1, -1)
    b = torch.as_tensor(b, dtype=torch.float64, device=m.device).reshape(1, -1)
    n, lo, hi = m[:, 0:1], m[:, 1:2], m[:, 2:3]
    Cgg, C11, C22, Cg1, Cg2, C12 = (m[:, k:k + 1] for k in range(6, 12))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=m.device)
    var = Cgg / (n - 1)
    gp = a * Cg1 + b * Cg2
    pp = a * a * C11 + 2 * a * b * C12 + b * b * C22
    mse = torch.clamp(((n - 1) - gp * gp / (var * pp)) / n, min=0)
    curve = 10 * torch.log10((hi - lo) ** 2 / var / mse)
    curve = torch.where((hi == lo) | ~(pp > 0), nan, curve)
    det = C11 * C22 - C12 * C12
    u0, u1 = C22 * Cg1 - C12 * Cg2, C11 * Cg2 - C12 * Cg1           # det * S^-1 c: det cancels in the ratio
    t_star = torch.where((det == 0) | (u0 + u1 == 0), nan, u0 / (u0 + u1))
    return curve, t_star[:, 0]
