"""Batched tiled prediction: the notebook loop of the reference
(notebooks/EvaluateJointIndi.ipynb cells 23-26: one tile per ``test()`` call,
490 strictly serial calls, numpy stitch on the host) as a device-resident
pipeline: gather tiles on the GPU -> batches of tiles through the sampler ->
(multi-GPU: one all-gather) -> HIP stitch into the (N,H,W,C) canvas.

Beyond the paste: blended stitching (``TileExchange(blend=True)``), per-step frame fusion for the Gaussian few-step
solvers (``predict_stack(fuse=True)``, ``fused_sample``) and frame diffusion for the InDI family
(``predict_stack_frames``, ``frame_sample``): every frame is one state, a row is one UNet forward per batch of tiles cut
out of it and one ``TilePlan.blend_step`` launch -- blend of the x0 tiles, InDI update and the frame's noise field in one
kernel --, over any number of ranks with one all-gather of whole x0 tiles per row."""
import torch

from .. import parallel
from .._lib import DsxError
from .tiling import PSNR_MAX_CHANNELS, TilePlan


class TileExchange:
    """The stitched output of a sharded run.  One rank: every batch is pasted straight into the canvas.  Several ranks:
    every batch's VALID REGIONS are packed into this rank's run of the exchange buffer (the crop of
    tile_stitcher.py:38-56 before the collective), one all-gather of the equal-sized runs (RCCL over xGMI) moves
    canvas bytes + padding instead of whole (C, p, p) tiles, and every rank pastes from the packed layout.

    ``blend=True``: blended stitching (``TilePlan.blend``) under ``window``.  This rank's WHOLE predicted tiles stay in a
    resident buffer -- its slot of the exchange buffer, tile ``id`` at index ``id // world`` --, ``add`` copies a batch
    in, and ``finish`` is one all-gather of the equal-sized slots (several ranks) and one blend of all tiles."""

    def __init__(self, plan, channels, device, group=None, gt=None, blend=False, window="triangle"):
        self.plan, self.C, self.group, self.gt = plan, int(channels), group, gt
        self.rank, self.world = parallel.rank(), parallel.world_size()
        self.canvas = self.part = self.flat = None
        self.blend = bool(blend)
        if self.blend:
            plan.set_window(window)
            self.flat = torch.zeros(plan.blend_rank_stride(self.world, self.C), dtype=torch.float32, device=device)
            self.tiles = self.flat.view((-1, self.C) + plan.patch_shape[1:])
        elif self.world == 1:
            self.canvas = torch.zeros(plan.data_shape + (self.C,), dtype=torch.float32, device=device)
            if gt is not None:
                self.part = plan.new_psnr_partials(self.C, device)
        else:
            self.flat = torch.zeros(plan.rank_stride(self.world, self.C), dtype=torch.float32, device=device)

    def add(self, tiles, ids):
        """``tiles`` (b, C, p, p): predictions of this rank's tile ids ``ids`` (a batch of its shard, in order)."""
        if len(ids) == 0:
            return
        if self.blend:
            j = int(ids[0]) // self.world
            self.tiles[j:j + len(ids)].copy_(tiles)
        elif self.world == 1:
            if self.gt is not None:
                self.plan.stitch_psnr_into(tiles, ids, self.canvas, self.gt, self.part)
            else:
                self.plan.stitch(tiles, ids, self.canvas)
        else:
            self.plan.pack(tiles, self.world, ids[0], self.flat)

    def gathered_bytes(self):
        """Bytes every rank receives from the collective (world * rank_stride * 4)."""
        return 0 if self.world == 1 else self.world * self.flat.numel() * 4

    def finish(self):
        """-> canvas (N,H,W,C), or (canvas, psnr (N,C)) when a ground truth was given."""
        if self.blend:
            if self.world == 1:
                return self.plan.blend(self.tiles, gt=self.gt)
            full = parallel.all_gather_flat(self.flat, self.group)   # one collective per canvas, of whole tiles
            return self.plan.blend(full, world=self.world, gt=self.gt, Cn=self.C)
        if self.world == 1:
            return self.canvas if self.gt is None else (self.canvas, self.plan.psnr_from_partials(self.part))
        full = parallel.all_gather_flat(self.flat, self.group)       # the path's only collective
        return self.plan.paste_packed(full, self.C, self.world, self.gt)


@torch.no_grad()
def predict_tiled(netG, frames_input, patch_size, grid_size=None, batch_tiles=8, sampler_kwargs=None,
                  group=None, lpips=None, target_frames=None, seed=None, stitch="crop", window="triangle"):
    """``frames_input``: (N,H,W) fp32 CUDA tensor, already normalised (the network input channel).
    Returns the stitched prediction (N,H,W,C) on every rank and the ``TilePlan``.

    ``lpips``: a ``core.lpips.LPIPS``; with it (and ``target_frames`` (N,H,W,C), the ground truth of the prediction
    channels) the first element is ``(canvas, lpips_dict)``, ``lpips_dict`` = ``core.metrics.calculate_lpips(
    target_frames, canvas, lpips)``: per channel the LPIPS of every frame, computed on the device.

    ``netG`` is what ``define_G`` returns (InDI / JointIndi sampler); its full-batch
    output (``last_full_batch``) is used, not the single element the reference API returns.

    ``seed``: per-sample noise streams (include/dsx.h) with a tile's id as its sample id: a tile's noise then does not
    depend on ``batch_tiles``, on the order of the batches or on the number of ranks, and neither does its prediction
    as long as the batch size is the same (the planner may pick other kernels for another).

    ``stitch``: ``"crop"`` pastes every tile's inner region (the reference's stitch); ``"blend"`` overlap-adds the whole
    tiles under the separable ``window`` (``TilePlan.blend``)."""
    _check_stitch("predict_tiled", stitch, window)
    if grid_size is None:
        grid_size = patch_size // 2                                   # split_dataset_tiledpred.py:13-14
    N, H, W = frames_input.shape
    plan = TilePlan((N, H, W), (1, grid_size, grid_size), (1, patch_size, patch_size))
    rank, world = parallel.rank(), parallel.world_size()
    ids = parallel.shard_ids(plan.total, rank, world)
    kw = dict(sampler_kwargs or {})
    ex = TileExchange(plan, netG.prediction_channels, frames_input.device, group, blend=stitch == "blend", window=window)
    for i in range(0, len(ids), batch_tiles):
        chunk = ids[i:i + batch_tiles]
        tiles = plan.gather(frames_input, chunk).unsqueeze(1)         # (b,1,p,p)
        if seed is not None:
            kw.update(seed=seed, sample_ids=chunk)
        netG.inference(tiles, continuous=False, **kw)
        ex.add(netG.last_full_batch, chunk)
    canvas = ex.finish()
    if lpips is None:
        return canvas, plan
    if target_frames is None:
        raise ValueError("predict_tiled(lpips=...) needs target_frames (N,H,W,C) to compare the prediction with")
    from ..core.metrics import calculate_lpips
    return (canvas, calculate_lpips(target_frames, canvas, lpips)), plan


def _check_stitch(what, stitch, window):
    from .tiling import WINDOWS
    if stitch not in ("crop", "blend"):
        raise DsxError(f"{what}: stitch = {stitch!r}: 'crop' or 'blend'")
    if stitch == "blend" and isinstance(window, str) and window not in WINDOWS:
        raise DsxError(f"{what}: window = {window!r}: one of {', '.join(WINDOWS)}, or a pair of arrays (wy, wx)")


def _is_gaussian(netG):
    from ..model.samplers import GaussianSampler
    return isinstance(netG, GaussianSampler)


@torch.no_grad()
def sample_tiles(netG, x, num_timesteps=None, solver=None, **noise):
    """One batch of input tiles ``x`` (b, 1, p, p) through whatever sampler ``define_G`` returned -> its full-batch
    prediction (b, C, p, p).  InDI family: ``inference`` (``num_timesteps`` steps).  A ``GaussianSampler`` (sr3 / ddpm):
    ``solver_sample_loop(x, **solver)`` with a solver -- the dict ``DDPM.set_solver`` keeps -- else ``super_resolution``,
    the full ancestral loop.  ``noise``: ``seed`` / ``sample_ids`` of the per-sample streams, or nothing."""
    if _is_gaussian(netG):
        if solver:
            netG.solver_sample_loop(x, **solver, **noise)
        else:
            netG.super_resolution(x, **noise)
    else:
        if solver:
            raise DsxError(f"solver: {type(netG).__name__} is not a Gaussian sampler (sr3 / ddpm); InDI's loop already "
                           "takes num_timesteps")
        netG.inference(x, continuous=False, **({} if num_timesteps is None else dict(num_timesteps=num_timesteps)),
                       **noise)
    return netG.last_full_batch


def _stochastic_rows(netG, num_timesteps, solver):
    """(rows, C): how many rows of one batch's loop add noise -- each is one materialised (B, C, p, p) draw under
    noise='field' -- and the channels C of the sampler's state."""
    if _is_gaussian(netG):
        if solver:
            sigma = netG.solver_table(**solver).sigma
            return sum(1 for s in range(len(sigma)) if sigma[s] != 0), int(netG.channels)
        netG._need_schedule()
        return (netG.num_timesteps - 1 if netG.kind == "sr3" else netG.num_timesteps), int(netG.channels)
    children = [netG.indi1, netG.indi2] if hasattr(netG, "indi1") else [netG]
    rows = sum(int(num_timesteps if num_timesteps is not None else c.num_timesteps) for c in children)
    return rows, int(children[0].out_channel)


@torch.no_grad()
def predict_stack(netG, dataset, batch_tiles=8, num_timesteps=None, samples=1, return_std=False, seed=None, group=None,
                  solver=None, noise="samples", field_noise_bytes=2 << 30, stitch=None, window="triangle", fuse=False):
    """The tiled prediction of a dataset that cuts its own normalised tiles -- an ``InputStackTiledPred`` (one
    superimposed acquisition, no ground truth) or a ``SplitDatasetTiledPred`` -- with ``samples`` posterior samples per
    tile: their mean and, with ``return_std``, the unbiased per-pixel spread, accumulated by one fused launch per sample
    (``engine.moments_update``, Welford in double) and one to finish.  ``samples == 1``: the prediction itself, spread 0.

    Returns ``(out, plan)``, ``out = {'mean': (N,H,W,C)}`` plus ``'std'`` (N,H,W,C) with ``return_std`` and, for a
    ``SplitDatasetTiledPred`` whose target has the prediction's channels, ``'psnr'`` (N,C): the RangeInvariantPsnr of the
    mean against the normalised ground truth, accumulated while pasting.  Everything in normalised units, on every rank.

    ``seed``: per-sample noise streams; sample ``r`` of tile ``k`` draws from sample id ``k + r * plan.total`` (the rule
    of ``predict_tiled_mixed``), whatever batch or rank it runs in.  Tiles are sharded over the ranks and exchanged
    through ``TileExchange``: one collective per output canvas.

    ``solver``: the dict ``DDPM.set_solver`` keeps (``solver``, ``steps``, ``eta``, ``spacing``): a Gaussian sampler
    (sr3 / ddpm) then runs that few-step solver per batch instead of its full ancestral loop; refused for any other.

    ``noise="field"`` (needs ``seed``): every draw is cut from a noise field keyed by the FRAME position
    (``TilePlan.randn_field``): a function of (seed, frame, draw ordinal, channel, y, x), so overlapping tiles start from
    -- and, in a stochastic row, receive -- the same noise where they overlap; posterior sample ``r`` takes
    ``id_base = r * frames``.  The draws travel in the loop's injected form, one (B, C, p, p) tensor per stochastic
    row; more than ``field_noise_bytes`` of them per batch is refused.  ``noise="samples"``: the streams above.

    ``stitch``: ``"crop"`` (the default) pastes every tile's inner region; ``"blend"`` overlap-adds the whole tiles under
    the separable ``window`` (``TilePlan.blend``: "triangle", "hann" or a pair of arrays) -- 'mean', 'std' and 'psnr'
    then each come from a blend.

    ``fuse=True`` (a Gaussian sampler with ``solver``, ``noise="field"`` and ``seed``, one rank; ``stitch`` is then
    "blend"): per-step frame fusion.  Every posterior sample diffuses each frame as ONE state (N,H,W,C), started from the
    noise field's draw 0: for every solver row the tiles are cut out of the state (``TilePlan.gather_canvas``), go
    through one UNet forward and one ``engine.solver_step`` per batch -- with the crops of the field's draw ``s + 1``
    where the row adds noise and the tiles of the blended x0 of the row before where it has a history term --, and are
    blended back into the state.  The state after the last row is the sample; with one tile per frame this is the
    unfused chain bit for bit."""
    from .. import engine
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"predict_stack: samples = {samples}: a positive count")
    plan = dataset.plan
    if solver and not _is_gaussian(netG):
        raise DsxError(f"predict_stack: solver: {type(netG).__name__} is not a Gaussian sampler (sr3 / ddpm); InDI's "
                       "loop already takes num_timesteps")
    if noise not in ("samples", "field"):
        raise DsxError(f"predict_stack: noise = {noise!r}: 'samples' or 'field'")
    if fuse:
        if stitch == "crop":
            raise DsxError("predict_stack: fuse with stitch='crop': a fused frame is a blend of its tiles; leave stitch "
                           "out or give 'blend'")
        if not _is_gaussian(netG):
            raise DsxError(f"predict_stack: fuse: {type(netG).__name__} is not a Gaussian sampler (sr3 / ddpm); frame "
                           "diffusion for the InDI family is predict_stack_frames")
        if not solver:
            raise DsxError("predict_stack: fuse needs solver=: the rows of a few-step solver are fused; the ancestral "
                           "loop is not")
        if noise != "field" or seed is None:
            raise DsxError("predict_stack: fuse needs noise='field' and seed=: overlapping tiles must receive the same "
                           "noise, or the blend would shrink its variance")
        if parallel.world_size() > 1:
            raise DsxError("predict_stack: fuse runs on one rank: a collective after every solver row is not provided")
        stitch = "blend"
    stitch = "crop" if stitch is None else stitch
    _check_stitch("predict_stack", stitch, window)
    blend = stitch == "blend"
    field = noise == "field"
    if fuse:
        if samples * plan.data_shape[0] > (1 << 39):
            raise DsxError("predict_stack: samples * frames exceeds the 2^39 field ids of one sampler")
        return _predict_stack_fused(netG, dataset, batch_tiles, samples, return_std, seed, solver, window), plan
    if field:
        if seed is None:
            raise DsxError("predict_stack: noise='field' needs seed=: a noise field is named by (seed, frame, draw)")
        rows, C_state = _stochastic_rows(netG, num_timesteps, solver)
        B = max(1, min(int(batch_tiles), plan.total))
        need = rows * B * C_state * plan.patch_shape[1] * plan.patch_shape[2] * 4
        if need > field_noise_bytes:
            raise DsxError(f"predict_stack: noise='field' materialises one (B, C, p, p) draw per stochastic row: {rows} "
                           f"rows x {B} tiles need {need} bytes, field_noise_bytes = {field_noise_bytes}; use a solver "
                           "(ddim with eta = 0 and dpmpp2m draw once per batch), fewer rows, or a smaller batch")
        joint_bit = getattr(netG, "STREAM2_BIT", 1 << 39)
        if samples * plan.data_shape[0] > joint_bit:
            raise DsxError("predict_stack: samples * frames exceeds the 2^39 field ids of one sampler")
    C_out = netG.prediction_channels
    gt = None
    if hasattr(dataset, "normalized_target_frames"):
        gt = dataset.normalized_target_frames()                       # every rank holds the frames: no collective
        if gt.shape[-1] != C_out or C_out > PSNR_MAX_CHANNELS:
            gt = None
    ex = ex_std = None
    ids = parallel.shard_ids(plan.total, parallel.rank(), parallel.world_size())
    kept_field = getattr(netG, "noise_field", None)
    try:
        for i in range(0, len(ids), batch_tiles):
            chunk = ids[i:i + batch_tiles]
            x = dataset.tiles(chunk)["input"]
            if ex is None:
                ex = TileExchange(plan, C_out, x.device, group, gt=gt, blend=blend, window=window)
                ex_std = TileExchange(plan, C_out, x.device, group, blend=blend, window=window) if return_std else None
            mean = m2 = None
            for r in range(samples):
                kw = {}
                if field:
                    # (shape, draw[, id_bit]): the crops of this batch's tiles out of the fields of sample r; a joint
                    # sampler's second child adds its bit to the field ids
                    netG.noise_field = lambda shape, draw, id_bit=0, chunk=chunk, r=r: plan.randn_field(
                        chunk, shape[1], seed, draw, id_base=r * plan.data_shape[0] + id_bit, device=x.device)
                elif seed is not None:
                    kw = dict(seed=seed, sample_ids=[k + r * plan.total for k in chunk])
                last = sample_tiles(netG, x, num_timesteps, solver, **kw)
                if samples > 1:
                    mean, m2 = engine.moments_update(last.contiguous(), mean, m2, r)
            if samples == 1:
                tiles, spread = netG.last_full_batch, None
                if return_std:
                    spread = torch.zeros_like(tiles)
            else:
                tiles, spread = engine.moments_finish(mean, m2, samples, want_std=return_std)
            ex.add(tiles, chunk)
            if return_std:
                ex_std.add(spread, chunk)
    finally:
        if field:
            netG.noise_field = kept_field
            for child in (getattr(netG, "indi1", None), getattr(netG, "indi2", None)):
                if child is not None:                                 # a joint sampler hands its field down per call
                    child.noise_field = None
    if ex is None:                                                    # a rank without tiles still joins the collectives
        dev = torch.device("cuda", torch.cuda.current_device())
        ex = TileExchange(plan, C_out, dev, group, gt=gt, blend=blend, window=window)
        ex_std = TileExchange(plan, C_out, dev, group, blend=blend, window=window) if return_std else None
    res = ex.finish()
    out = {"mean": res[0], "psnr": res[1]} if gt is not None else {"mean": res}
    if return_std:
        out["std"] = ex_std.finish()
    return out, plan


def fused_sample(netG, dataset, table, batch_tiles, seed, id_base, order=None, keep_tiles=None):
    """One posterior sample of per-step frame fusion -> the frame state (N,H,W,C) after the last row of ``table`` (a
    ``SolverTableHost``).  The state starts as draw 0 of the noise fields ``id_base + n``; per row and batch of tiles:
    ``gather_canvas`` -> ``denoise_fn`` -> ``engine.solver_step`` -> two resident (total, C, p, p) buffers; after the
    row's last batch the x tiles are blended into the state, the x0 tiles into the history when the next row reads it.
    The last short batch is moved back to end at the last tile (one executor, one batch size).  ``order``: a permutation
    of the batches (the result does not depend on it).  ``keep_tiles``: a list that receives the x tiles of every row
    before their blend (a copy per row)."""
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
            last = chunk[-1] + 1
            xt[last - keep:last] = xo[B - keep:]
            x0t[last - keep:last] = x0[B - keep:]
        if keep_tiles is not None:
            keep_tiles.append(xt.clone())
        X = plan.blend(xt)
        if s + 1 < K and table.cp[s + 1] != 0:
            X0 = plan.blend(x0t)
    return X


def _predict_stack_fused(netG, dataset, batch_tiles, samples, return_std, seed, solver, window):
    """``predict_stack(fuse=True)`` after its checks: the frame states of the posterior samples (``fused_sample``) are the
    stitched frames -- their mean and spread come from ``engine.moments_update`` over whole frames, and 'psnr' from a
    paste of the mean's own tiles (a copy) against the ground truth."""
    from .. import engine
    plan = dataset.plan
    plan.set_window(window)
    table = netG.solver_table(**solver)
    mean = m2 = X = None
    for r in range(samples):
        X = fused_sample(netG, dataset, table, batch_tiles, seed, r * plan.data_shape[0])
        if samples > 1:
            mean, m2 = engine.moments_update(X, mean, m2, r)
    spread = None
    if samples > 1:
        X, spread = engine.moments_finish(mean, m2, samples, want_std=return_std)
    elif return_std:
        spread = torch.zeros_like(X)
    out = {"mean": X}
    C_out = netG.prediction_channels
    if hasattr(dataset, "normalized_target_frames"):
        gt = dataset.normalized_target_frames()
        if gt.shape[-1] == C_out and C_out <= PSNR_MAX_CHANNELS and X.shape[-1] == C_out:
            out["psnr"] = plan.stitch_with_psnr(plan.gather_canvas(X), gt)[1]
    if return_std:
        out["std"] = spread
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
    canvas = None
    for i in range(0, plan.total, max(1, int(batch_tiles))):
        chunk = list(range(i, min(i + max(1, int(batch_tiles)), plan.total)))
        canvas = plan.stitch(dataset.tiles(chunk)["input"], chunk, canvas)
    return canvas


def frame_sample(child, dataset, x_in, num_timesteps, t_float_start, batch_tiles, seed, id_base, group=None,
                 keep_tiles=None):
    """One posterior sample of frame diffusion with the InDI sampler ``child`` -> the frame state (N,H,W,C) after the
    last row of ``engine.indi_step_table``.  ``x_in`` (N,H,W,Cin): the normalised input frames.  The state starts as
    ``x_in`` (repeated to the sampler's channels) ``+ Z0 * (e * t)``, Z0 draw 0 of the noise fields ``id_base + n``; per
    row ``s`` and batch of this rank's tiles: ``gather_canvas`` -> ``denoise_fn`` -> a resident (local tiles, C, p, p) x0
    buffer, the rank's slot of the exchange buffer; after the row's last batch one all-gather of the slots (several
    ranks) and one ``TilePlan.blend_step`` with draw ``s + 1``: the whole InDI update of the row, on the canvas.  A short
    last batch is moved back (one executor).  ``keep_tiles``: a list that receives the x0 tiles of every row before
    their blend (a copy per row; one rank)."""
    from .. import engine
    plan = dataset.plan
    N, H, W = plan.data_shape
    dev = x_in.device
    rank, world = parallel.rank(), parallel.world_size()
    copies = child._copies(x_in.permute(0, 3, 1, 2))
    X = torch.cat([x_in] * copies, dim=-1)
    Cn = int(X.shape[-1])
    fids = [id_base + n for n in range(N)]
    z0 = engine.randn_samples((N, Cn, H, W), seed, fids, draw=0, device=dev).permute(0, 2, 3, 1)
    scale = (child.e * torch.Tensor([t_float_start])).to(dev)          # InDISampler._start's two operations
    X = (X + z0 * scale).contiguous()
    table = engine.indi_step_table(num_timesteps, t_float_start, child.e)
    flat = torch.zeros(plan.blend_rank_stride(world, Cn), dtype=torch.float32, device=dev)
    x0t = flat.view((-1, Cn) + plan.patch_shape[1:])
    batches = list(_batches(parallel.shard_ids(plan.total, rank, world), batch_tiles))
    for s in range(table.n_steps):
        time = torch.Tensor([float(table.tcond[s])]).to(dev)
        for chunk, keep in batches:
            x0 = child.denoise_fn(plan.gather_canvas(X, chunk), time)
            last = chunk[-1] // world + 1
            x0t[last - keep:last] = x0[len(chunk) - keep:]
        if keep_tiles is not None:
            keep_tiles.append(x0t.clone())
        row = (float(table.c1[s]), float(table.c2[s]), float(table.sigma[s]), seed, s + 1, id_base)
        if world == 1:
            plan.blend_step(x0t, X, *row)
        else:
            full = parallel.all_gather_flat(flat, group)              # the row's one collective, of whole x0 tiles
            plan.blend_step(full, X, *row, world=world, Cn=Cn)
    return X


@torch.no_grad()
def predict_stack_frames(netG, dataset, batch_tiles=8, num_timesteps=None, t_float_start=None, samples=1,
                         return_std=False, seed=None, group=None, window="triangle"):
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
    (``engine.moments_update``).  With one tile per frame this is ``predict_stack(seed=, noise="field")`` bit for bit."""
    from .. import engine
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
    samples = int(samples)
    if samples < 1:
        raise DsxError(f"{what}: samples = {samples}: a positive count")
    children = _indi_children(netG, t_float_start)
    for child, _, _ in children:
        if child._noise_mode == "brownian":
            raise DsxError(f"{what}: noise mode 'brownian' is not built (only 'gaussian')")
    plan = dataset.plan
    N = plan.data_shape[0]
    if samples * N > (1 << 39):
        raise DsxError(f"{what}: samples * frames exceeds the 2^39 field ids of one sampler")
    _check_stitch(what, "blend", window)
    plan.set_window(window)
    x_in = input_frames(dataset, batch_tiles)
    mean = m2 = X = None
    for r in range(samples):
        parts = [frame_sample(child, dataset, x_in, int(child.num_timesteps if num_timesteps is None else num_timesteps),
                              t0, batch_tiles, seed, r * N + bit, group) for child, t0, bit in children]
        X = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
        if samples > 1:
            mean, m2 = engine.moments_update(X, mean, m2, r)
    spread = None
    if samples > 1:
        X, spread = engine.moments_finish(mean, m2, samples, want_std=return_std)
    elif return_std:
        spread = torch.zeros_like(X)
    out = {"mean": X}
    C_out = netG.prediction_channels
    if hasattr(dataset, "normalized_target_frames"):
        gt = dataset.normalized_target_frames()
        if gt.shape[-1] == C_out and C_out <= PSNR_MAX_CHANNELS and X.shape[-1] == C_out:
            out["psnr"] = plan.stitch_with_psnr(plan.gather_canvas(X), gt)[1]
    if return_std:
        out["std"] = spread
    return out, plan


# ---- mixed-input evaluation (BASELINE C5: JointIndi + TimePredictor) -----------------------------------------------
def _batches(ids, batch):
    """Batches of ``batch`` consecutive entries of the arithmetic id list ``ids``; the last short batch is moved back
    to end at the last id (still arithmetic, same batch size: no second executor) -> (chunk, entries to keep)."""
    batch = max(1, min(int(batch), len(ids)))
    for i in range(0, len(ids), batch):
        if i + batch <= len(ids):
            yield ids[i:i + batch], batch
        else:
            yield ids[len(ids) - batch:], len(ids) - i


@torch.no_grad()
def evaluate_time_predictor(val_set, time_predictor, num_timesteps=20, batch_tiles=16):
    """The classifier sweep of notebooks/time_prediction_evaluation.ipynb cells 3-7: for every mixing ratio of
    ``np.arange(0, 1.01, 1 / num_timesteps)`` the TimePredictor's estimate on every tile of ``val_set`` (a
    ``SplitDatasetTiledPred``), fed ``target0 * t + target1 * (1 - t)`` min-max-normalised with row
    ``int(t * num_timesteps)`` of the range table (the 'cls' channel 1 of ``mixed_tiles``).  One fused gather launch
    and one batched TimePredictor forward per (ratio, batch); the last short batch overlaps the one before it, so the
    whole sweep runs on one executor.  Returns ``(all_pred (n + 1, n_tiles) float32 numpy, rmse)`` with the RMSE of
    cell 7.  One rank (the sweep is not sharded)."""
    import numpy as np
    from .time_predictor_dataset import compute_input_normalization_dict
    n = int(num_timesteps)
    table = compute_input_normalization_dict(val_set._data_dict, n, val_set._mean_target, val_set._std_target)
    gt = np.arange(0, 1.01, 1 / n)[:n + 1]
    assert len(gt) == n + 1
    ids = range(len(val_set))
    all_pred = torch.empty((n + 1, len(ids)), dtype=torch.float32, device=val_set._dev[0].device)
    for k, t in enumerate(gt):
        for chunk, keep in _batches(ids, batch_tiles):
            cls = val_set.mixed_tiles(chunk, float(t), table, want=("cls",))["cls"]
            pred = time_predictor(cls[:, 1:2])
            all_pred[k, chunk[-1] + 1 - keep:chunk[-1] + 1] = pred[len(chunk) - keep:]
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
    i1, i2 = netG.indi1, netG.indi2
    if getattr(netG, "noise_source", None) is not None:
        i1.noise_source = i2.noise_source = netG.noise_source
    dev = val_set._dev[0].device
    plan = val_set.plan
    if t_from == "classifier" and table is None:
        from .time_predictor_dataset import compute_input_normalization_dict
        table = compute_input_normalization_dict(val_set._data_dict, table_timesteps, val_set._mean_target,
                                                 val_set._std_target)
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
    import numpy as np
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
    import numpy as np
    from ..core.psnr import comoments, range_invariant_psnr_curve
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError(f"predict_tiled_refined: rounds = {rounds}: 0 or more")
    if scope not in REFINE_SCOPES:
        raise ValueError(f"predict_tiled_refined: scope = {scope!r}: one of {', '.join(REFINE_SCOPES)}")
    t_list = np.arange(0, 1.0, 0.05) if t_list is None else np.asarray(t_list, dtype=np.float64).reshape(-1)
    if t_list.size < 1 or not np.isfinite(t_list).all():
        raise ValueError("predict_tiled_refined: t_list: at least one finite mixing time")
    i1, i2 = netG.indi1, netG.indi2
    if getattr(netG, "noise_source", None) is not None:
        i1.noise_source = i2.noise_source = netG.noise_source
    dev = val_set._dev[0].device
    plan = val_set.plan
    rank, world = parallel.rank(), parallel.world_size()
    if keep_tiles and world > 1:
        raise DsxError("predict_tiled_refined: keep_tiles holds every tile on one rank; not with several ranks")
    if time_predictor is not None and table is None:
        from .time_predictor_dataset import compute_input_normalization_dict
        table = compute_input_normalization_dict(val_set._data_dict, table_timesteps, val_set._mean_target,
                                                 val_set._std_target)
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
