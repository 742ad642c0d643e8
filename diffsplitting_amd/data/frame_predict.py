"""The frame-state drivers of tiled prediction: every frame is ONE state, a row is one UNet forward per batch of tiles
cut out of it and a blend back onto the frame canvas.  Per-step frame fusion for the Gaussian few-step solvers
(``predict_stack(fuse=True)``, ``fused_sample``) and frame diffusion for the InDI family (``predict_stack_frames``,
``frame_sample``: a row is one ``TilePlan.blend_step`` launch and, over several ranks, one all-gather of x0 tiles)."""
import torch

from .. import parallel
from .._lib import DsxError
from .tile_predict import (FrameDisagreement, _apply_consistency, _batches, _check_consistency, _check_disagreement, _check_field_ids, _check_frame_map, _check_quantile_bytes, _check_quantiles, _check_rank_gt,
                           _check_samples, _check_stitch, _is_gaussian, _mean_and_spread, _mean_spread_quantiles,
                           _scorable_gt, store_kept)


def _frame_outputs(netG, dataset, samples, return_std, draw, q=None, ranks=False):
    """What both frame-state drivers return: the frame states ``draw(r)`` (N,H,W,C) of the posterior samples are the stitched
    frames -- 'mean', with ``return_std`` 'std', and 'psnr' from a paste of the mean's own tiles against the ground truth.
    ``q`` / ``ranks`` (checked by the caller): the states are kept, 'quantiles' (Q,N,H,W,C) and 'rank' (N,H,W,C) are
    taken over them per pixel."""
    plan, C_out = dataset.plan, netG.prediction_channels
    gt = _scorable_gt(dataset, C_out)
    quant = rank = None
    if q is not None or ranks:
        _check_rank_gt("predict_stack" if _is_gaussian(netG) else "predict_stack_frames", ranks, gt)
        states = torch.empty((samples,) + tuple(plan.data_shape) + (C_out,), dtype=torch.float32, device=dataset.device)
        X, spread, quant, rank = _mean_spread_quantiles(samples, return_std, draw, states, q,
                                                        gt.contiguous() if ranks else None)
    else:
        X, spread = _mean_and_spread(samples, return_std, draw)
    out = {"mean": X}
    if gt is not None and X.shape[-1] == C_out:
        out["psnr"] = plan.stitch_with_psnr(plan.gather_canvas(X), gt)[1]
    if return_std:
        out["std"] = spread
    if quant is not None:
        out["quantiles"] = quant
    if rank is not None:
        out["rank"] = rank
    return out


def fused_sample(netG, dataset, table, batch_tiles, seed, id_base, order=None, keep_tiles=None, measure=None):
    """One posterior sample of per-step frame fusion -> the frame state (N,H,W,C) after the last row of ``table`` (a
    ``SolverTableHost``).  The state starts as draw 0 of the noise fields ``id_base + n``; per row and batch of tiles:
    ``gather_canvas`` -> ``denoise_fn`` -> ``engine.solver_step`` -> two resident (total, C, p, p) buffers; after the
    row's last batch the x tiles are blended into the state, the x0 tiles into the history when the next row reads it.
    The last short batch is moved back to end at the last tile (one executor, one batch size).  ``order``: a permutation
    of the batches (the result does not depend on it).  ``keep_tiles``: a list that receives the x tiles of every row
    before their blend (a copy per row).  ``measure``: a ``FrameDisagreement`` that takes the x tiles of the last row,
    what ``keep_tiles[-1]`` holds."""
    from .. import engine
    plan = dataset.plan
    N, H, W = plan.data_shape
    Cn, dev = int(netG.channels), netG.betas.device
    X = engine.randn_samples((N, Cn, H, W), seed, [id_base + n for n in range(N)], draw=0, device=dev)
    X = X.permute(0, 2, 3, 1).contiguous()
    X0 = None
    shape = (plan.total, Cn) + plan.patch_shape[1:]
    xt, x0t = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
    batches = [(list(chunk), keep) for chunk, keep in _batches(range(plan.total), batch_tiles)]
    if order is not None:
        batches = [batches[i] for i in order]
    K = table.n_steps
    for s in range(K):
        for chunk, keep in batches:
            B = len(chunk)
            col = lambda name: torch.full((B,), float(getattr(table, name)[s]), device=dev)
            x = plan.gather_canvas(X, chunk)
            inp = torch.cat([dataset.tiles(chunk)["input"], x], dim=1) if netG.conditional else x
            time = col("tcond").view(B, 1) if netG.kind == "sr3" else col("tcond")
            net = netG.denoise_fn(inp, time)
            z = plan.randn_field(chunk, Cn, seed, draw=s + 1, id_base=id_base, device=dev) if table.sigma[s] != 0 else None
            hist = table.cp[s] != 0
            x0, xo = engine.solver_step(x, net, col("a"), col("b"), col("cx"), col("c0"), col("sigma"),
                                        cp=col("cp") if hist else None,
                                        x0_prev=plan.gather_canvas(X0, chunk) if hist else None, clip=table.clip, z=z)
            store_kept(xt, xo, chunk, keep)
            store_kept(x0t, x0, chunk, keep)
        if keep_tiles is not None:
            keep_tiles.append(xt.clone())
        if measure is not None and s == K - 1:
            measure.child(xt, 1, Cn)
        X = plan.blend(xt)
        if s + 1 < K and table.cp[s + 1] != 0:
            X0 = plan.blend(x0t)
    return X


def _predict_stack_fused(netG, dataset, batch_tiles, samples, return_std, seed, solver, window, q=None, ranks=False,
                         measure=None):
    """``predict_stack(fuse=True)`` after its checks: the frame states of the posterior samples (``fused_sample``),
    sample ``r`` with the field ids ``r * frames + n``.  ``measure``: a ``FrameDisagreement`` or None."""
    dataset.plan.set_window(window)
    frames, table = dataset.plan.data_shape[0], netG.solver_table(**solver)

    def draw(r):
        X = fused_sample(netG, dataset, table, batch_tiles, seed, r * frames, measure=measure)
        if measure is not None:
            measure.end_sample()
        return X
    out = _frame_outputs(netG, dataset, samples, return_std, draw, q, ranks)
    if measure is not None:
        out["disagreement"] = measure.result()
    return out


# ---- frame diffusion for the InDI family ----------------------------------------------------------------------------
def _indi_children(netG, t_float_start):
    """[(InDI sampler, its start time, the bit its field ids carry)]: the sampler itself, or the two children of a joint
    sampler (indi1 at t, indi2 at 1 - t under ``STREAM2_BIT``; ``JointIndiSampler.inference``'s defaults)."""
    if hasattr(netG, "indi1"):
        t = 0.5 if t_float_start is None else t_float_start
        return [(netG.indi1, t, 0), (netG.indi2, 1 - t, netG.STREAM2_BIT)]
    return [(netG, 1.0 if t_float_start is None else t_float_start, 0)]


def input_frames(dataset, batch_tiles=8):
    """The normalised input of every frame, (N,H,W,Cin): the crop-paste (a copy) of the dataset's own input tiles.  Every
    rank holds the frames, so every rank cuts all tiles: no collective."""
    plan = dataset.plan
    batch = max(1, int(batch_tiles))
    canvas = None
    for i in range(0, plan.total, batch):
        chunk = list(range(i, min(i + batch, plan.total)))
        canvas = plan.stitch(dataset.tiles(chunk)["input"], chunk, canvas)
    return canvas


def frame_sample(child, dataset, x_in, num_timesteps, t_float_start, batch_tiles, seed, id_base, group=None,
                 keep_tiles=None, measure=None):
    """One posterior sample of frame diffusion with the InDI sampler ``child`` -> the frame state (N,H,W,C) after the
    last row of ``engine.indi_step_table``.  ``x_in`` (N,H,W,Cin): the normalised input frames.  The state starts as
    ``x_in`` (repeated to the sampler's channels) ``+ Z0 * (e * t)``, Z0 draw 0 of the noise fields ``id_base + n``; per
    row ``s`` and batch of this rank's tiles: ``gather_canvas`` -> ``denoise_fn`` -> a resident (local tiles, C, p, p) x0
    buffer, the rank's slot of the exchange buffer; after the row's last batch one all-gather of the slots (several
    ranks) and one ``TilePlan.blend_step`` with draw ``s + 1``: the whole InDI update of the row, on the canvas.  A short
    last batch is moved back (one executor).  ``keep_tiles``: a list that receives the x0 tiles of every row before
    their blend (a copy per row; one rank).  ``measure``: a ``FrameDisagreement`` that takes the x0 tiles of the last row
    in the layout the row's ``blend_step`` reads, gathered or not."""
    from .. import engine
    plan = dataset.plan
    N, H, W = plan.data_shape
    dev = x_in.device
    rank, world = parallel.rank(), parallel.world_size()
    X = torch.cat([x_in] * child._copies(x_in.permute(0, 3, 1, 2)), dim=-1)
    Cn = int(X.shape[-1])
    z0 = engine.randn_samples((N, Cn, H, W), seed, [id_base + n for n in range(N)], draw=0, device=dev).permute(0, 2, 3, 1)
    scale = (child.e * torch.Tensor([t_float_start])).to(dev)          # InDISampler._start's two operations
    X = (X + z0 * scale).contiguous()
    table = engine.indi_step_table(num_timesteps, t_float_start, child.e)
    flat = torch.zeros(plan.blend_rank_stride(world, Cn), dtype=torch.float32, device=dev)
    x0t = flat.view((-1, Cn) + plan.patch_shape[1:])
    batches = list(_batches(parallel.shard_ids(plan.total, rank, world), batch_tiles))
    for s in range(table.n_steps):
        time = torch.Tensor([float(table.tcond[s])]).to(dev)
        for chunk, keep in batches:
            store_kept(x0t, child.denoise_fn(plan.gather_canvas(X, chunk), time), chunk, keep, world)
        if keep_tiles is not None:
            keep_tiles.append(x0t.clone())
        row = (float(table.c1[s]), float(table.c2[s]), float(table.sigma[s]), seed, s + 1, id_base)
        last = measure is not None and s == table.n_steps - 1
        if world == 1:
            if last:
                measure.child(x0t, 1, Cn)
            plan.blend_step(x0t, X, *row)
        else:
            full = parallel.all_gather_flat(flat, group)              # the row's one collective, of whole x0 tiles
            if last:
                measure.child(full, world, Cn)
            plan.blend_step(full, X, *row, world=world, Cn=Cn)
    return X


@torch.no_grad()
def predict_stack_frames(netG, dataset, batch_tiles=8, num_timesteps=None, t_float_start=None, samples=1,
                         return_std=False, seed=None, group=None, window="triangle", quantiles=None, ranks=False,
                         quantile_bytes=8 << 30, disagreement=False, seam_band=8, consistency=False,
                         consistency_noise=0.0, consistency_weights=None):
    """``predict_stack`` for the InDI family (``InDISampler`` and its subclasses, ``JointIndiSampler``) with every frame
    diffused as ONE state: frame diffusion.  The InDI update ``x <- (d/t) x0 + (1 - d/t) x + e (t - d) z`` is affine in
    the UNet output with coefficients shared by the batch, so a row of a frame is ``X <- c_x0 * blend(x0 tiles) +
    c_xt * X + sigma * Z`` on the canvas, ``Z`` the frame's noise field: one ``TilePlan.blend_step`` launch per row --
    no per-tile step launch and no per-tile noise tensors (``frame_sample``).  Overlapping tiles are cut from one
    state, so they agree after every row, not only in the last blend.

    Returns ``(out, plan)`` with ``predict_stack``'s keys, on every rank.  Posterior sample ``r`` takes the field ids
    ``r * frames + n``; a joint sampler's second child adds ``STREAM2_BIT``, its two children run one after the other
    and their states are joined along the channels.  ``t_float_start``: one start time for every frame (default: 1.0,
    0.5 for a joint sampler, whose second child starts at ``1 - t``).  Tiles are sharded over the ranks: one collective
    per row and child, every rank holds the same state.  ``samples > 1``: mean and spread over the frame states
    (``engine.moments_update``).  With one tile per frame this is ``predict_stack(seed=, noise="field")`` bit for bit.

    ``quantiles=`` / ``ranks=True`` (``samples`` in 2..64): ``out['quantiles']`` (Q,N,H,W,C) and ``out['rank']`` (N,H,W,C)
    as ``predict_stack`` describes them; a draw is the whole frame state here, so both are exact per pixel.  The
    ``samples`` states are kept: more than ``quantile_bytes`` of them is refused before any launch.

    ``disagreement=True`` / ``"sums"`` with ``seam_band``: ``out['disagreement']`` as ``predict_stack`` describes it, of
    the x0 tiles of the last row before their blend (a joint sampler's two children joined along the channels), per
    posterior sample: counts and sums are added in sample order, min / max folded; a map needs ``samples == 1``.

    ``consistency=`` / ``consistency_noise=`` / ``consistency_weights=``: as ``predict_stack`` describes them, through the
    same helper on the finished canvases."""
    from ..model.samplers import InDISampler, JointIndiSampler
    what = "predict_stack_frames"
    if _is_gaussian(netG):
        raise DsxError(f"{what}: {type(netG).__name__} is a Gaussian sampler (sr3 / ddpm): its per-step frame fusion is "
                       "predict_stack(fuse=True)")
    if not isinstance(netG, (InDISampler, JointIndiSampler)):
        raise DsxError(f"{what}: {type(netG).__name__} is no InDI or JointIndi sampler")
    if seed is None:
        raise DsxError(f"{what} needs seed=: a frame's noise field is named by (seed, frame, draw)")
    if torch.is_tensor(t_float_start) or isinstance(t_float_start, (list, tuple)) or \
            (hasattr(t_float_start, "shape") and getattr(t_float_start, "ndim", 0) > 0):
        raise DsxError(f"{what}: a per-sample t_float_start: a frame has one time; give one number")
    samples = _check_samples(what, samples, DsxError)
    children = _indi_children(netG, t_float_start)
    for child, _, _ in children:
        if child._noise_mode == "brownian":
            raise DsxError(f"{what}: noise mode 'brownian' is not built (only 'gaussian')")
    plan, N = dataset.plan, dataset.plan.data_shape[0]
    _check_field_ids(what, samples, N)
    _check_stitch(what, "blend", window)
    measure = _check_disagreement(what, disagreement, seam_band, max(c.out_channel for c, _, _ in children) if disagreement
                                  else None)
    _check_frame_map(what, "the frame-state path", measure, samples)
    measure = FrameDisagreement(plan, measure, seam_band) if measure else None
    q, ranks = _check_quantiles(what, samples, quantiles, ranks, dataset)
    if q is not None or ranks:
        _check_quantile_bytes(what, samples, plan, netG.prediction_channels, quantile_bytes)
    cons = _check_consistency(what, consistency, consistency_noise, consistency_weights, dataset, netG.prediction_channels,
                              q, ranks)
    plan.set_window(window)
    x_in = input_frames(dataset, batch_tiles)

    def draw(r):
        parts = [frame_sample(child, dataset, x_in, int(child.num_timesteps if num_timesteps is None else num_timesteps),
                              t0, batch_tiles, seed, r * N + bit, group, measure=measure) for child, t0, bit in children]
        if measure is not None:
            measure.end_sample()
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
    out = _frame_outputs(netG, dataset, samples, return_std, draw, q, ranks)
    if measure is not None:
        out["disagreement"] = measure.result()
    return _apply_consistency(out, dataset, cons), plan
