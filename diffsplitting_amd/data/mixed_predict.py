"""The mixed-input drivers of tiled prediction (BASELINE C5: JointIndi + TimePredictor): the classifier sweep
(``evaluate_time_predictor``), the split of tiles mixed at a given ratio with per-tile start times (``predict_tiled_mixed``)
and the same with the start times re-estimated from the split itself (``predict_tiled_refined``, ``choose_times``)."""
import numpy as np
import torch

from .. import parallel
from .._lib import DsxError
from .tile_predict import TileExchange, _batches, store_kept


@torch.no_grad()
def evaluate_time_predictor(val_set, time_predictor, num_timesteps=20, batch_tiles=16):
    """The classifier sweep of notebooks/time_prediction_evaluation.ipynb cells 3-7: for every mixing ratio of
    ``np.arange(0, 1.01, 1 / num_timesteps)`` the TimePredictor's estimate on every tile of ``val_set`` (a
    ``SplitDatasetTiledPred``), fed ``target0 * t + target1 * (1 - t)`` min-max-normalised with row
    ``int(t * num_timesteps)`` of the range table (the 'cls' channel 1 of ``mixed_tiles``).  One fused gather launch
    and one batched TimePredictor forward per (ratio, batch); the last short batch overlaps the one before it, so the
    whole sweep runs on one executor.  Returns ``(all_pred (n + 1, n_tiles) float32 numpy, rmse)`` with the RMSE of
    cell 7.  One rank (the sweep is not sharded)."""
    from .time_predictor_dataset import compute_input_normalization_dict
    n = int(num_timesteps)
    table = compute_input_normalization_dict(val_set._data_dict, n, val_set._mean_target, val_set._std_target)
    gt = np.arange(0, 1.01, 1 / n)[:n + 1]
    assert len(gt) == n + 1
    ids = range(len(val_set))
    all_pred = torch.empty((n + 1, len(ids)), dtype=torch.float32, device=val_set.device)
    for k, t in enumerate(gt):
        for chunk, keep in _batches(ids, batch_tiles):
            cls = val_set.mixed_tiles(chunk, float(t), table, want=("cls",))["cls"]
            store_kept(all_pred[k], time_predictor(cls[:, 1:2]), chunk, keep)
    all_pred = all_pred.cpu().numpy()
    mse = ((all_pred - gt.reshape(-1, 1)) ** 2).mean(axis=1)          # cell 7
    return all_pred, float(np.sqrt(mse.mean()))


def _set_rows(pred_t, chunk, world, t1, t2):
    """The start times of a batch into the rows of its tiles (``chunk``: ids of one shard, ``world`` apart)."""
    rows = slice(chunk[0], chunk[-1] + 1, world)
    if isinstance(t1, torch.Tensor):
        pred_t[rows] = torch.stack([t1, t2], dim=1).to(pred_t.dtype)
    else:
        pred_t[rows, 0], pred_t[rows, 1] = float(t1), float(t2)


def _mixed_setup(netG, val_set, classify, table, table_timesteps):
    """The opening of both mixed-input drivers -> (device, plan, range table): a ``noise_source`` of the joint sampler goes
    down to its children; the table is computed (``table_timesteps`` rows) where the classifier needs one and none came."""
    if getattr(netG, "noise_source", None) is not None:
        netG.indi1.noise_source = netG.indi2.noise_source = netG.noise_source
    if classify and table is None:
        from .time_predictor_dataset import compute_input_normalization_dict
        table = compute_input_normalization_dict(val_set._data_dict, table_timesteps, val_set._mean_target,
                                                 val_set._std_target)
    return val_set.device, val_set.plan, table


def _mixed_batches(netG, time_predictor, val_set, ids, mixing_t, start, table, num_timesteps, mmse_count, batch_tiles,
                   seed, draw_base=0):
    """The batch loop of the mixed-input drivers: for every batch of the shard ``ids`` the mixed tiles at ``mixing_t``,
    the start times, and the MMSE mean of ``netG.indi1`` on ``mix[:, 0]`` and ``netG.indi2`` on ``mix[:, 1]``.  Yields
    ``(chunk, mix (b, 2, p, p), (t1, t2), est (b, 2, p, p))``.  ``start``: "classifier" (``pred_t_0 = 1 - TP(cls[:, 0])``,
    ``pred_t_1 = TP(cls[:, 1])``, normalised with ``table``), a number (both samplers of every tile), or a
    (n_tiles, 2) tensor of per-tile times.  With ``seed``, repeat ``r`` of tile ``k`` draws from sample id
    ``k + (draw_base + r) * plan.total`` (``indi2`` from the same id with bit 39 set)."""
    i1, i2 = netG.indi1, netG.indi2
    plan = val_set.plan
    world = parallel.world_size()
    classify = isinstance(start, str)
    want = ("mix", "cls") if classify else ("mix",)
    for i in range(0, len(ids), batch_tiles):
        chunk = ids[i:i + batch_tiles]
        out = val_set.mixed_tiles(chunk, mixing_t, table if classify else None, want=want)
        in1, in2 = out["mix"][:, 0:1].contiguous(), out["mix"][:, 1:2].contiguous()
        if classify:
            t1 = 1 - time_predictor(out["cls"][:, 0:1])
            t2 = time_predictor(out["cls"][:, 1:2])
        elif isinstance(start, torch.Tensor):
            rows = start[chunk[0]:chunk[-1] + 1:world]
            t1, t2 = rows[:, 0].contiguous(), rows[:, 1].contiguous()
        else:
            t1 = t2 = start
        acc1 = acc2 = None
        for r in range(int(mmse_count)):                              # as core/psnr_based_t_refinement.py:26-39
            k1 = k2 = {}
            if seed is not None:
                rep_ids = [k + (draw_base + r) * plan.total for k in chunk]
                k1, k2 = dict(seed=seed, sample_ids=rep_ids), dict(seed=seed, sample_ids=netG.second_ids(rep_ids))
            i1.inference(in1, continuous=False, num_timesteps=num_timesteps, t_float_start=t1, **k1)
            acc1 = i1.last_full_batch.clone() if acc1 is None else acc1 + i1.last_full_batch
            i2.inference(in2, continuous=False, num_timesteps=num_timesteps, t_float_start=t2, **k2)
            acc2 = i2.last_full_batch.clone() if acc2 is None else acc2 + i2.last_full_batch
        yield chunk, out["mix"], (t1, t2), torch.cat([acc1, acc2], dim=1) / mmse_count


@torch.no_grad()
def predict_tiled_mixed(netG, time_predictor, val_set, mixing_t, num_timesteps=1, mmse_count=1, batch_tiles=8,
                        t_from="classifier", table=None, table_timesteps=100, group=None, lpips=None, seed=None):
    """The out-of-distribution split of notebooks/EvaluateJointIndiIterative.ipynb cells 59-64, batched: the two
    channels of every tile of ``val_set`` (a ``SplitDatasetTiledPred``) mixed at ``mixing_t`` -> the TimePredictor's
    estimate of the mixing time per tile (``pred_t_0 = 1 - TP(cls[:, 0])``, ``pred_t_1 = TP(cls[:, 1])``, cell 40) ->
    ``netG.indi1`` on ``mix[:, 0]`` started at pred_t_0 and ``netG.indi2`` on ``mix[:, 1]`` at pred_t_1 (per-sample
    step tables, one batched loop per sampler) -> mean over ``mmse_count`` repeats -> stitched, with RangeInvariantPsnr
    accumulated while pasting.

    ``t_from="given"`` skips the classifier and starts both samplers at ``mixing_t`` (the reference's scalar
    ``t_float_start``).  ``table``: the range table (computed with ``table_timesteps`` rows when not given; cell 40
    uses 100).  Returns ``((canvas (N,H,W,2), psnr (N,2)), pred_t (n_tiles, 2))``.

    The score is taken in normalised space against ``val_set.normalized_target_frames()``: the notebook de-normalises
    prediction and target first, a positive affine map per channel, under which RangeInvariantPsnr does not change --
    no extra pass.  A sampler's own ``noise_source`` is used (set ``netG.noise_source`` to give both the same).
    Several ranks: tiles are sharded through ``TileExchange`` as in ``predict_tiled``; ``pred_t`` then holds this
    rank's tiles only (NaN elsewhere); ``gather_pred_t`` completes it on every rank.

    ``lpips``: a ``core.lpips.LPIPS``; with it the first element is ``(canvas, psnr, lpips_dict)``, the per-frame LPIPS of
    every channel against the same normalised target (``core.metrics.calculate_lpips``; its min-max map makes it
    invariant under the de-normalisation too).

    ``seed``: per-sample noise streams; MMSE repeat ``r`` of tile ``k`` draws from sample id ``k + r * plan.total``
    (``indi2`` from the same id with bit 39 set), whatever batch or rank it runs in."""
    if t_from not in ("classifier", "given"):
        raise ValueError("t_from must be 'classifier' or 'given'")
    dev, plan, table = _mixed_setup(netG, val_set, t_from == "classifier", table, table_timesteps)
    gt = val_set.normalized_target_frames()
    ex = TileExchange(plan, 2, dev, group, gt=gt)
    ids = parallel.shard_ids(plan.total, ex.rank, ex.world)
    pred_t = torch.full((plan.total, 2), float("nan"), dtype=torch.float32, device=dev)
    start = "classifier" if t_from == "classifier" else mixing_t
    for chunk, _, (t1, t2), est in _mixed_batches(netG, time_predictor, val_set, ids, mixing_t, start, table,
                                                  num_timesteps, mmse_count, batch_tiles, seed):
        _set_rows(pred_t, chunk, ex.world, t1, t2)
        ex.add(est, chunk)
    if lpips is None:
        return ex.finish(), pred_t
    from ..core.metrics import calculate_lpips
    canvas, psnr = ex.finish()
    return (canvas, psnr, calculate_lpips(gt, canvas, lpips)), pred_t


def gather_pred_t(pred_t, group=None):
    """``pred_t`` (n_tiles, 2) of a sharded ``predict_tiled_mixed`` -- rank q holds the rows of its tiles q, q + W, ...
    and NaN elsewhere -- completed on every rank: one all-gather of the small table, row i taken from its owner
    i % W.  One rank: returned as it is.  Any per-tile table (n_tiles, columns) of any dtype is completed the same way
    (the per-round table of ``predict_tiled_refined``)."""
    world = parallel.world_size()
    if world == 1:
        return pred_t
    full = parallel.all_gather_flat(pred_t.reshape(-1).contiguous(), group).view(world, -1, pred_t.shape[1])
    ids = torch.arange(pred_t.shape[0], device=pred_t.device)
    return full[ids % world, ids].contiguous()


REFINE_SCOPES = ("tile", "frame", "set")


def choose_times(curves, units, t_list, previous):
    """The argmax rule of ``predict_tiled_refined`` on the host: ``curves`` (tiles, G) float64, ``units`` (tiles,) the
    scope unit of every tile, ``previous`` (tiles, 2) the start times in force.  For every unit the nanmean of its tiles'
    curves over the tiles, then ``t_list[argmax]`` for both samplers of its tiles; a unit whose mean curve is all NaN keeps
    ``previous``.  Only grid points > 0 can be chosen: a sampler cannot start at 0 (InDI's step weighs its prediction
    with delta / t: 0 / 0), and an input that scores best there needs no splitting; the curves keep the whole grid.
    -> (start times (tiles, 2) float32, chosen (units,) float64 with NaN for a kept unit, mean curves
    (units, G))."""
    curves, units = np.asarray(curves, dtype=np.float64), np.asarray(units)
    startable = np.asarray(t_list, dtype=np.float64) > 0
    out = np.array(previous, dtype=np.float32, copy=True)
    n_units = int(units.max()) + 1 if units.size else 0
    chosen, means = np.full(n_units, np.nan), np.full((n_units, curves.shape[1]), np.nan)
    for u in range(n_units):
        rows = curves[units == u]
        ok = ~np.isnan(rows)
        cnt = ok.sum(axis=0)
        mean = np.where(cnt > 0, np.where(ok, rows, 0.0).sum(axis=0) / np.maximum(cnt, 1), np.nan)
        means[u] = mean
        if np.isnan(mean[startable]).all():
            continue
        chosen[u] = t_list[int(np.nanargmax(np.where(startable, mean, np.nan)))]
        out[units == u] = np.float32(chosen[u])
    return out, chosen, means


@torch.no_grad()
def predict_tiled_refined(netG, time_predictor, val_set, mixing_t, num_timesteps=1, mmse_count=1, batch_tiles=8, rounds=1,
                          scope="frame", t_list=None, table=None, table_timesteps=100, group=None, seed=None,
                          keep_tiles=False):
    """``predict_tiled_mixed`` with the start times re-estimated from the split itself (the scan of
    core/psnr_based_t_refinement.py:41-57, EvaluateJointIndiIterative.ipynb cells 44-54, which needs no ground truth).

    Round 0 starts every tile at the TimePredictor's estimate, exactly as ``t_from="classifier"``, or -- without a
    TimePredictor -- at 0.5 (``JointIndi.inference``'s default).  Every round scores each tile k from its own inputs
    ``in1 = mix[:, 0]``, ``in2 = mix[:, 1]`` and its MMSE estimates c1, c2, for every tau of ``t_list`` (default
    ``np.arange(0, 1, 0.05)``):

        curve_k(tau) = 1/2 [RIPSNR(in1, (1 - tau) c1 + tau c2) + RIPSNR(in2, (1 - tau) c2 + tau c1)]

    (``mixed_tiles``' definition of the two inputs), on the device: one ``core.psnr.comoments`` call per batch and the
    closed-form curve; nothing of tile size leaves the GPU.  Round r + 1 starts both samplers of a tile at
    ``t_list[argmax]`` (over the grid points > 0: no sampler starts at 0) of a nanmean curve: the tile's own (``scope="tile"``), that of its frame's tiles ("frame", the
    reference's consensus taken per frame) or of all tiles ("set"); a unit whose curve is all NaN keeps its time
    (``choose_times``).  The tiles of the last round (round ``rounds``) are stitched and scored as ``predict_tiled_mixed``
    does: ``rounds=0`` returns its canvas, PSNR and ``pred_t`` bit for bit.

    Returns ``((canvas, psnr), pred_t, report)``: ``pred_t`` (tiles, 2) float32, the last round's start times;
    ``report`` = ``{"t_list", "units", "rounds": [{"start" (tiles, 2), "moments" (tiles, 2, 12), "curves" (tiles, G),
    "t_star" (tiles, 2), "chosen" (units,), "mean_curves" (units, G)}, ...]}`` as numpy arrays (``t_star``: the
    continuous maximiser in tau per input, not clamped; ``chosen``: what the round's curves select, NaN for a kept
    unit), plus ``"tiles"`` / ``"mix"`` (tiles, 2, p, p) of the last round with ``keep_tiles`` (one rank).

    Several ranks: tiles are sharded as in ``predict_tiled_mixed``; per round ONE all-gather completes the small
    (tiles, G + 28) table on every rank (``gather_pred_t``), so every rank derives the same times and holds the same
    report.  ``seed``: repeat ``r`` of tile ``k`` in round ``q`` draws from sample id
    ``k + (q * mmse_count + r) * plan.total``: rounds do not reuse noise, and any number of ranks stitches the same bits."""
    from ..core.psnr import comoments, range_invariant_psnr_curve
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError(f"predict_tiled_refined: rounds = {rounds}: 0 or more")
    if scope not in REFINE_SCOPES:
        raise ValueError(f"predict_tiled_refined: scope = {scope!r}: one of {', '.join(REFINE_SCOPES)}")
    t_list = np.arange(0, 1.0, 0.05) if t_list is None else np.asarray(t_list, dtype=np.float64).reshape(-1)
    if t_list.size < 1 or not np.isfinite(t_list).all():
        raise ValueError("predict_tiled_refined: t_list: at least one finite mixing time")
    rank, world = parallel.rank(), parallel.world_size()
    if keep_tiles and world > 1:
        raise DsxError("predict_tiled_refined: keep_tiles holds every tile on one rank; not with several ranks")
    dev, plan, table = _mixed_setup(netG, val_set, time_predictor is not None, table, table_timesteps)
    units = {"tile": np.arange(plan.total), "frame": plan.patch_start[:, 0].copy(),
             "set": np.zeros(plan.total, dtype=np.int64)}[scope]
    G = len(t_list)
    gt = val_set.normalized_target_frames()
    ids = parallel.shard_ids(plan.total, rank, world)
    start = "classifier" if time_predictor is not None else 0.5
    report = {"t_list": t_list, "units": units, "rounds": []}
    ex = None
    for q in range(rounds + 1):
        last = q == rounds
        if last:
            ex = TileExchange(plan, 2, dev, group, gt=gt)
            if keep_tiles:
                shape = (plan.total, 2) + plan.patch_shape[1:]
                report["tiles"], report["mix"] = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
        # this round's small table: {start (2), curve (G), moments (24), t_star (2)} per tile, NaN for other ranks' tiles
        tab = torch.full((plan.total, G + 28), float("nan"), dtype=torch.float64, device=dev)
        for chunk, mix, (t1, t2), est in _mixed_batches(netG, time_predictor, val_set, ids, mixing_t, start, table,
                                                        num_timesteps, mmse_count, batch_tiles, seed,
                                                        draw_base=q * int(mmse_count)):
            rows = slice(chunk[0], chunk[-1] + 1, world)
            b, pp = len(chunk), plan.patch_shape[1:]
            _set_rows(tab[:, 0:2], chunk, world, t1, t2)
            # planes (k, 0): g = in1, p1 = c1, p2 = c2;  (k, 1): g = in2, p1 = c2, p2 = c1
            m = comoments(mix.reshape((2 * b,) + pp), est.reshape((2 * b,) + pp), est.flip(1).reshape((2 * b,) + pp))
            c, ts = range_invariant_psnr_curve(m, 1 - t_list, t_list)
            tab[rows, 2:2 + G] = 0.5 * (c[0::2] + c[1::2])
            tab[rows, 2 + G:26 + G] = m.view(b, 24)
            tab[rows, 26 + G:] = (1 - ts).view(b, 2)             # t* weighs p1: tau = 1 - t*
            if last:
                ex.add(est, chunk)
                if keep_tiles:
                    report["tiles"][rows], report["mix"][rows] = est, mix
        full = gather_pred_t(tab, group).cpu().numpy()                # the round's one collective
        begun = full[:, 0:2].astype(np.float32)
        nxt, chosen, means = choose_times(full[:, 2:2 + G], units, t_list, begun)
        report["rounds"].append({"start": begun, "curves": full[:, 2:2 + G].copy(),
                                 "moments": full[:, 2 + G:26 + G].reshape(-1, 2, 12).copy(),
                                 "t_star": full[:, 26 + G:].copy(), "chosen": chosen, "mean_curves": means})
        start = torch.from_numpy(nxt).to(dev)
    pred_t = torch.from_numpy(report["rounds"][-1]["start"]).to(dev)
    return ex.finish(), pred_t, report
