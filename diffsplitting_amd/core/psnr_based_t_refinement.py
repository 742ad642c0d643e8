"""TimePredictor-driven refinement (core/psnr_based_t_refinement.py of the reference; notebook
EvaluateJointIndi.ipynb cells 42-62), batched on the MI355X:

  1. the time classifier predicts the mixing time of every tile            (one batched TimePredictor forward)
  2. indi_1 / indi_2 turn the input into the two channel estimates, each tile started at ITS predicted time
     (one batched loop per sampler with per-sample step tables; the reference loops over the batch with batch 1)
  3. optional MMSE: the mean over ``mmse_count`` independent repeats         (cells 60-62)
  4. the mixing time is re-estimated by scanning t in [0, 1) for the best RangeInvariantPsnr of
     t * ch1 + (1 - t) * ch2 against the input                             (:41-57)
     -- by the reference's loop of 20 metric calls, or (``estimate_time_from_estimates``, ``fused=True``) from ONE HIP
     pass over the three planes and the closed-form curve (``core.psnr.comoments``, include/dsx.h: dsx_comoments)

Function names and return values follow the reference module; the reference's own file cannot be imported anywhere
(it imports the external ``disentangle`` package, :10) and calls ``p_sample_loop`` — the old name of ``inference``.
"""
import numpy as np
import torch

from .psnr import RangeInvariantPsnr


@torch.no_grad()
def get_time_prediction_from_classifier(inp, time_classifier):
    return time_classifier(inp.cuda())                                # :14-17


@torch.no_grad()
def get_channel_estimates(inp, indi_1, indi_2, time_classifier, num_timesteps=1, mmse_count=1, as_numpy=True):
    """:20-39.  for classifier input = t * c1 + (1 - t) * c2; indi_1 (target c1 at time 0) starts at 1 - t."""
    inp = inp.cuda().float()
    pred_t_2 = get_time_prediction_from_classifier(inp, time_classifier)
    pred_t_1 = 1 - pred_t_2
    acc1 = acc2 = None
    for _ in range(int(mmse_count)):
        indi_1.inference(inp, continuous=False, num_timesteps=num_timesteps, t_float_start=pred_t_1)
        ch1 = indi_1.last_full_batch.clone()
        indi_2.inference(inp, continuous=False, num_timesteps=num_timesteps, t_float_start=pred_t_2)
        ch2 = indi_2.last_full_batch.clone()
        acc1 = ch1 if acc1 is None else acc1 + ch1
        acc2 = ch2 if acc2 is None else acc2 + ch2
    pred1, pred2 = acc1 / mmse_count, acc2 / mmse_count               # MMSE estimate: mean over the repeats
    if as_numpy:
        return pred1.cpu().numpy(), pred2.cpu().numpy()
    return pred1, pred2


def _nanmean_argmax(curves):
    """argmax over the grid of the nanmean over the rows of ``curves`` (rows, G); -1 when every row is NaN there."""
    ok = ~torch.isnan(curves)
    mean = torch.where(ok, curves, torch.zeros_like(curves)).sum(dim=0) / ok.sum(dim=0)     # 0 / 0 = NaN: no row
    if bool(torch.isnan(mean).all()):
        return -1
    return int(torch.where(torch.isnan(mean), torch.full_like(mean, float("-inf")), mean).argmax())


@torch.no_grad()
def estimate_time_from_estimates(inp, pred1, pred2, t_list=np.arange(0, 1.0, 0.05)):
    """The scan of :41-57 from ONE pass over the three planes of every sample (``core.psnr.comoments``, one kernel call)
    and the closed-form curve (``core.psnr.range_invariant_psnr_curve``): ``pred1 * t + pred2 * (1 - t)`` scored
    against ``inp[:, 0]`` for every t of ``t_list``.  ``inp``, ``pred1``, ``pred2``: (B, 1, H, W) (or (B, H, W)) CUDA
    fp32.  Returns ``(per_sample_t (B,) numpy, concensus_t, curves (B, G) float64 CUDA, t_star (B,) float64 CUDA)``:
    the per-sample argmax, the argmax of the nanmean over the samples (NaN when every curve is NaN), and the
    continuous maximiser, not clamped.  A sample whose curve is all NaN (a constant input) has per_sample_t NaN."""
    from .psnr import comoments, range_invariant_psnr_curve
    t_list = np.asarray(t_list, dtype=np.float64)
    g = inp[:, 0] if inp.dim() == 4 else inp
    curves, t_star = range_invariant_psnr_curve(comoments(g, pred1, pred2), t_list, 1 - t_list)
    dead = torch.isnan(curves).all(dim=1)
    idx = torch.where(torch.isnan(curves), torch.full_like(curves, float("-inf")), curves).argmax(dim=1)
    per_sample_t = np.where(dead.cpu().numpy(), np.nan, t_list[idx.cpu().numpy()])
    best = _nanmean_argmax(curves)
    return per_sample_t, (float("nan") if best < 0 else t_list[best]), curves, t_star


@torch.no_grad()
def estimate_time_using_PSNR(inp, indi_1, indi_2, time_classifier, num_timesteps=1, mmse_count=1, fused=False):
    """:41-57.  inp: (B, 1, H, W) normalised input.  Returns (per_sample_t, concensus_t).  ``fused=True`` scores the
    same channel estimates through ``estimate_time_from_estimates``: one kernel pass instead of the loop below."""
    pred1, pred2 = get_channel_estimates(inp, indi_1, indi_2, time_classifier, num_timesteps, mmse_count, as_numpy=False)
    if fused:
        return estimate_time_from_estimates(inp.cuda().float(), pred1.float(), pred2.float())[:2]
    gt = inp.cuda().float()[:, 0]
    t_list = np.arange(0, 1.0, 0.05)
    psnr_list = []
    for t in t_list:
        pred = pred1 * float(t) + pred2 * float(1 - t)
        psnr_list.append(RangeInvariantPsnr(gt, pred[:, 0]))
    psnr_matrix = torch.stack(psnr_list).cpu()
    per_sample_t = t_list[psnr_matrix.argmax(dim=0).numpy()]
    concensus_t = t_list[int(psnr_matrix.mean(dim=1).argmax())]
    return per_sample_t, concensus_t
