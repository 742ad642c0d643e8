"""The per-tile drivers ``predict_tiled`` / ``predict_stack`` -- every tile runs its own chain, the stitch comes last -- and
what every driver shares: ``TileExchange``, the batching of an id list (``_batches``, ``store_kept``), the refusals."""
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
    in, and ``finish`` is one all-gather of the equal-sized slots (several ranks) and one blend of all tiles.

    ``disagreement=True`` (or ``"sums"``: no map): ``finish`` also measures how far the whole tiles differ where they
    overlap (``TilePlan.disagreement`` with ``band = seam_band``) and leaves the result in ``self.disagreement``.  Under
    ``blend=True`` the kernel reads the buffer the blend reads, gathered or not.  Under crop the exchange additionally
    keeps this rank's whole tiles in a slot of ``blend_rank_stride`` elements and, with several ranks, does ONE MORE
    all-gather, of those slots -- only when asked; the canvas still comes from the cropped exchange, bit for bit."""

    def __init__(self, plan, channels, device, group=None, gt=None, blend=False, window="triangle", disagreement=False,
                 seam_band=8):
        self.plan, self.C, self.group, self.gt = plan, int(channels), group, gt
        self.rank, self.world = parallel.rank(), parallel.world_size()
        self.canvas = self.part = self.flat = self.whole = self.disagreement = None
        self.blend = bool(blend)
        self.measure, self.seam_band = _check_disagreement("TileExchange", disagreement, seam_band, self.C), int(seam_band)
        if self.measure and not self.blend:
            self.whole = torch.zeros(plan.blend_rank_stride(self.world, self.C), dtype=torch.float32, device=device)
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
        if self.whole is not None:
            j = int(ids[0]) // self.world
            self.whole.view((-1, self.C) + self.plan.patch_shape[1:])[j:j + len(ids)].copy_(tiles)
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
                self._measure(self.tiles)
                return self.plan.blend(self.tiles, gt=self.gt)
            full = parallel.all_gather_flat(self.flat, self.group)   # one collective per canvas, of whole tiles
            self._measure(full)
            return self.plan.blend(full, world=self.world, gt=self.gt, Cn=self.C)
        if self.whole is not None:                                    # crop: the whole tiles travel only for the measure
            self._measure(self.whole.view((-1, self.C) + self.plan.patch_shape[1:]) if self.world == 1 else
                          parallel.all_gather_flat(self.whole, self.group))
        if self.world == 1:
            return self.canvas if self.gt is None else (self.canvas, self.plan.psnr_from_partials(self.part))
        full = parallel.all_gather_flat(self.flat, self.group)       # the path's only collective
        return self.plan.paste_packed(full, self.C, self.world, self.gt)

    def _measure(self, tiles):
        if self.measure:
            self.disagreement = self.plan.disagreement(tiles, world=self.world, Cn=self.C, band=self.seam_band,
                                                       want_map=self.measure is True)


def _batches(ids, batch):
    """Batches of ``batch`` consecutive entries of the arithmetic id list ``ids``; the last short batch is moved back
    to end at the last id (still arithmetic, same batch size: no second executor) -> (chunk, entries to keep)."""
    batch = max(1, min(int(batch), len(ids)))
    for i in range(0, len(ids), batch):
        if i + batch <= len(ids):
            yield ids[i:i + batch], batch
        else:
            yield ids[len(ids) - batch:], len(ids) - i


def store_kept(buf, out, chunk, keep, world=1):
    """The last ``keep`` entries of ``out``, the output of a batch ``(chunk, keep)`` of ``_batches`` -- the ones before them
    belong to the batch it was moved back over --, into the resident buffer ``buf`` at local index ``id // world``."""
    last = chunk[-1] // world + 1
    buf[last - keep:last] = out[len(chunk) - keep:]


# ---- refusals that several drivers share, each worded once: ``what`` names the caller, ``error`` is its exception class
def _check_stitch(what, stitch, window):
    from .tiling import WINDOWS
    if stitch not in ("crop", "blend"):
        raise DsxError(f"{what}: stitch = {stitch!r}: 'crop' or 'blend'")
    if stitch == "blend" and isinstance(window, str) and window not in WINDOWS:
        raise DsxError(f"{what}: window = {window!r}: one of {', '.join(WINDOWS)}, or a pair of arrays (wy, wx)")


def _check_disagreement(what, disagreement, seam_band, channels=None):
    """-> False, "sums" or True: what ``disagreement=`` asks for; the refusals that need no launch"""
    if disagreement is None or disagreement is False:
        return False
    if disagreement is not True and disagreement != "sums":
        raise DsxError(f"{what}: disagreement = {disagreement!r}: False, 'sums' or True")
    if isinstance(seam_band, bool) or int(seam_band) != seam_band or not 1 <= int(seam_band) <= 65535:
        raise DsxError(f"{what}: seam_band = {seam_band!r}: an integer in 1..65535")
    if channels is not None and not 1 <= int(channels) <= PSNR_MAX_CHANNELS:
        raise DsxError(f"{what}: disagreement: {int(channels)} prediction channels, the measure takes 1..{PSNR_MAX_CHANNELS}")
    return disagreement


def _check_frame_map(what, path, disagreement, samples):
    if disagreement is True and samples > 1:
        raise DsxError(f"{what}: disagreement=True on {path} with samples = {samples}: the x0 tiles of every posterior "
                       "sample have a map of their own; give disagreement='sums', or samples=1")


class FrameDisagreement:
    """The measure on the frame-state paths: ``child`` takes the x0 tiles of a sampler's last row (one call per child of
    a joint sampler, joined along the channels), ``end_sample`` closes a posterior sample: counts and sums are added
    in sample order, min / max folded (``fold_disagreement``).  A map is kept for a single sample only."""

    def __init__(self, plan, mode, band):
        self.plan, self.mode, self.band, self.parts, self.total, self.samples = plan, mode, int(band), [], None, 0

    def child(self, tiles, world, Cn):
        self.parts.append(self.plan.disagreement(tiles, world=world, Cn=Cn, band=self.band, want_map=self.mode is True))

    def end_sample(self):
        from .tiling import fold_disagreement
        parts, self.parts = self.parts, []
        one = parts[0] if len(parts) == 1 else {
            k: None if parts[0][k] is None else torch.cat([p[k] for p in parts], dim={"map": -1, "partials": 2}.get(k, 1))
            for k in parts[0]}
        self.total = one if self.samples == 0 else fold_disagreement(self.total, one)   # the fold carries no map
        self.samples += 1

    def result(self):
        return None if self.total is None else dict(self.total, map=self.total.get("map"))


def _check_samples(what, samples, error):
    if int(samples) < 1:
        raise error(f"{what}: samples = {int(samples)}: a positive count")
    return int(samples)


def _check_field_ids(what, samples, frames, limit=1 << 39):
    if samples * frames > limit:
        raise DsxError(f"{what}: samples * frames exceeds the 2^39 field ids of one sampler")


def _check_solver(what, netG, solver):
    if solver and not _is_gaussian(netG):                             # what = None: sample_tiles never named itself
        raise DsxError(f"{what + ': ' if what else ''}solver: {type(netG).__name__} is not a Gaussian sampler (sr3 / ddpm); "
                       "InDI's loop already takes num_timesteps")


def _is_gaussian(netG):
    from ..model.samplers import GaussianSampler
    return isinstance(netG, GaussianSampler)


def _scorable_gt(dataset, C_out):
    """The normalised ground truth (N,H,W,C) a stitched prediction of ``C_out`` channels is scored against (every rank
    holds the frames: no collective), or None: the dataset has none, other channels, or more than the PSNR sums take."""
    gt = dataset.normalized_target_frames() if hasattr(dataset, "normalized_target_frames") else None
    return gt if gt is not None and gt.shape[-1] == C_out and C_out <= PSNR_MAX_CHANNELS else None


def _mean_and_spread(samples, return_std, draw):
    """``draw(r)`` for r = 0 .. samples - 1 -> (mean, unbiased spread or None without ``return_std``): one fused
    ``engine.moments_update`` launch per sample and one ``moments_finish``.  One sample: the draw itself, spread 0."""
    from .. import engine
    mean = m2 = x = None
    for r in range(samples):
        x = draw(r)
        if samples > 1:
            mean, m2 = engine.moments_update(x.contiguous(), mean, m2, r)
    if samples > 1:
        return engine.moments_finish(mean, m2, samples, want_std=return_std)
    return x, (torch.zeros_like(x) if return_std else None)


MAX_QUANTILE_SAMPLES, MAX_QUANTILES = 64, 8                           # dsx_sample_quantiles: n <= 64, nq <= 8


def _check_quantiles(what, samples, quantiles, ranks, dataset, blend=False):
    """The refusals of ``quantiles=`` / ``ranks=`` that need no launch -> (q as a tuple of floats or None, ranks).
    ``blend``: the maps would be blended tile maps.  A dataset without target frames is refused here; one whose
    target has other channels by ``_check_rank_gt``, once the frames are at hand."""
    q = None
    if quantiles is not None:
        try:
            q = tuple(float(v) for v in (quantiles if hasattr(quantiles, "__iter__") else (quantiles,)))
        except (TypeError, ValueError):
            raise DsxError(f"{what}: quantiles = {quantiles!r}: 1 to {MAX_QUANTILES} numbers in [0, 1]")
        if not 1 <= len(q) <= MAX_QUANTILES or any(not 0.0 <= v <= 1.0 for v in q):   # a NaN fails both comparisons
            raise DsxError(f"{what}: quantiles = {quantiles!r}: 1 to {MAX_QUANTILES} numbers in [0, 1]")
    ranks = bool(ranks)
    if q is None and not ranks:
        return None, False
    if samples < 2:
        raise DsxError(f"{what}: quantiles= and ranks= are taken over the posterior samples: samples = {samples}, give 2 "
                       "or more")
    if samples > MAX_QUANTILE_SAMPLES:
        raise DsxError(f"{what}: quantiles= and ranks= sort the samples in registers: samples = {samples}, at most "
                       f"{MAX_QUANTILE_SAMPLES}")
    if ranks and blend:
        raise DsxError(f"{what}: ranks=True with stitch='blend': a blend of per-tile ranks is not a rank; use stitch='crop' "
                       "or a frame-state path (fuse=True, predict_stack_frames), where ranks are exact per pixel")
    if ranks and not hasattr(dataset, "normalized_target_frames"):
        _check_rank_gt(what, ranks, None)
    return q, ranks


def _check_rank_gt(what, ranks, gt):
    if ranks and gt is None:
        raise DsxError(f"{what}: ranks=True: the dataset holds no ground truth with the prediction's channels to rank "
                       "among the samples")


def _check_quantile_bytes(what, samples, plan, channels, quantile_bytes):
    N, H, W = plan.data_shape
    need = samples * N * H * W * channels * 4
    if need > quantile_bytes:
        raise DsxError(f"{what}: quantiles= / ranks= keep the {samples} frame states of {N} x {H} x {W} x {channels}: {need} "
                       f"bytes, quantile_bytes = {quantile_bytes}; draw fewer samples, split fewer frames per call or raise "
                       "quantile_bytes")


def _check_consistency(what, consistency, noise, weights, dataset, channels, q=None, ranks=False):
    """The refusals of ``consistency=`` that need no launch -> None (not asked for) or the checked
    ``(project, rho, weights)``.  The arguments that go with it are refused without it."""
    if consistency is False or consistency is None:
        if noise or weights is not None:
            raise DsxError(f"{what}: consistency_noise= / consistency_weights= without consistency=True or 'project'")
        return None
    if consistency is not True and consistency != "project":
        raise DsxError(f"{what}: consistency = {consistency!r}: False, True (report) or 'project'")
    from ..core.consistency import check_noise, check_weights
    if not hasattr(dataset, "acquisition"):
        raise DsxError(f"{what}: consistency= compares the prediction with the acquisition it was made from: "
                       f"{type(dataset).__name__} does not expose one (an InputStackTiledPred does: its resident stack, "
                       "pixel type and input_clip)")
    if getattr(dataset, "_target_channel_idx", None) is not None:
        raise DsxError(f"{what}: consistency= with target_channel_idx = {dataset._target_channel_idx}: the prediction "
                       "holds one of the summands, the sum cannot be formed")
    n_w = channels if weights is None else len(list(weights))
    if n_w != channels:
        raise DsxError(f"{what}: consistency=: {n_w} channel weights for a prediction of {channels} channels (a "
                       "target_channel_idx config predicts one of the two summands: the sum cannot be formed)")
    project = consistency == "project"
    if project and (q is not None or ranks):
        raise DsxError(f"{what}: consistency='project' with quantiles= / ranks=: quantile and rank maps are not "
                       "projected; ask for them in a run of their own, or use consistency=True")
    return project, check_noise(noise), check_weights(weights, channels)


def _apply_consistency(out, dataset, checked):
    """The shared post-processing of ``consistency=``, on the stitched canvases, on every rank (each holds the canvases
    and the resident stack: no collective).  Adds ``out['consistency']``, the report of the prediction as it was made;
    under 'project' the conditioned mean and spread replace ``out['mean']`` / ``out['std']`` and the unprojected mean
    stays under ``out['mean_raw']``."""
    if checked is None:
        return out
    from ..core.consistency import consistency as run
    project, rho, w = checked
    stack, pix, _, clip = dataset.acquisition()
    rep = run(out["mean"], stack, dataset.get_normalization_dict(), weights=w, std=out.get("std"), clip=clip, noise=rho,
              project=project, pix=pix)
    if project:
        out["mean_raw"], out["mean"] = out["mean"], rep.pop("mean")
        if "std" in rep:
            out["std"] = rep.pop("std")
    out["consistency"] = rep
    return out


def _mean_spread_quantiles(samples, return_std, draw, buf, q, target):
    """``_mean_and_spread`` for ``samples >= 2`` that also keeps the draws: ``draw(r)`` is copied into ``buf[r]`` (the
    samplers reuse their output buffer), feeds the Welford launch from there, and one ``engine.sample_quantiles`` launch
    reads the whole of ``buf`` -> (mean, spread or None, quantiles (len(q), ...) or None, rank (...) or None)."""
    from .. import engine
    mean = m2 = None
    for r in range(samples):
        buf[r].copy_(draw(r))
        mean, m2 = engine.moments_update(buf[r], mean, m2, r)
    mean, spread = engine.moments_finish(mean, m2, samples, want_std=return_std)
    quant, rank = engine.sample_quantiles(buf, q, target)
    return mean, spread, quant, rank


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


@torch.no_grad()
def sample_tiles(netG, x, num_timesteps=None, solver=None, **noise):
    """One batch of input tiles ``x`` (b, 1, p, p) through whatever sampler ``define_G`` returned -> its full-batch
    prediction (b, C, p, p).  InDI family: ``inference`` (``num_timesteps`` steps).  A ``GaussianSampler`` (sr3 / ddpm):
    ``solver_sample_loop(x, **solver)`` with a solver -- the dict ``DDPM.set_solver`` keeps -- else ``super_resolution``,
    the full ancestral loop.  ``noise``: ``seed`` / ``sample_ids`` of the per-sample streams, or nothing."""
    _check_solver(None, netG, solver)
    if not _is_gaussian(netG):
        netG.inference(x, continuous=False, **({} if num_timesteps is None else dict(num_timesteps=num_timesteps)),
                       **noise)
    elif solver:
        netG.solver_sample_loop(x, **solver, **noise)
    else:
        netG.super_resolution(x, **noise)
    return netG.last_full_batch


def _stochastic_rows(netG, num_timesteps, solver):
    """(rows, C): how many rows of one batch's loop add noise -- each is one materialised (B, C, p, p) draw under
    noise='field' -- and the channels C of the sampler's state."""
    if _is_gaussian(netG):
        return len(netG.noise_rows(netG.solver_table(**solver) if solver else None)), int(netG.channels)
    children = [netG.indi1, netG.indi2] if hasattr(netG, "indi1") else [netG]
    rows = sum(len(c.noise_rows(int(num_timesteps if num_timesteps is not None else c.num_timesteps))) for c in children)
    return rows, int(children[0].out_channel)


@torch.no_grad()
def predict_stack(netG, dataset, batch_tiles=8, num_timesteps=None, samples=1, return_std=False, seed=None, group=None,
                  solver=None, noise="samples", field_noise_bytes=2 << 30, stitch=None, window="triangle", fuse=False,
                  quantiles=None, ranks=False, quantile_bytes=8 << 30, disagreement=False, seam_band=8,
                  consistency=False, consistency_noise=0.0, consistency_weights=None):
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
    unfused chain bit for bit.

    ``quantiles=(q1, ..)`` (1 to 8 values in [0, 1]) and ``ranks=True`` (both need ``samples`` in 2..64) add
    ``out['quantiles']`` (Q,N,H,W,C), the per-pixel quantiles of the samples (``np.quantile`` in float64, linear, bit for
    bit), and ``out['rank']`` (N,H,W,C), the number of samples strictly below the normalised ground truth (0..samples,
    as float32; ``core.calibration.rank_histogram`` counts them).  The draws of a batch are then kept in one
    (samples, B, C, p, p) buffer and one ``engine.sample_quantiles`` launch per batch sorts them per element; every map
    is stitched like 'std', through an exchange of its own.  With ``stitch="blend"`` a quantile map is a BLEND OF THE
    PER-TILE QUANTILES -- not the quantile of blended samples --, and ``ranks=True`` is refused: a blend of ranks is not a
    rank.  With ``fuse=True`` a draw is the whole frame state, quantiles and ranks are exact per pixel, and the
    ``samples`` states are kept: more than ``quantile_bytes`` of them is refused.  ``ranks=True`` needs a dataset whose
    ground truth has the prediction's channels.  Without either argument nothing changes.

    ``disagreement=True`` (or ``"sums"``: no map) adds ``out['disagreement']``, the dict of ``TilePlan.disagreement`` with
    ``band = seam_band``: how far the tiles that predicted a pixel differ, over every overlap and over the band around
    the crop lines -- a quality signal that needs no ground truth.  It measures the tiles the 'mean' exchange receives:
    with ``samples = N`` the per-tile means of N samples (independent per-tile streams alone make those differ by about
    ``std * sqrt(2 / N)`` pairwise).  Under ``stitch="crop"`` with several ranks the whole tiles take one more all-gather;
    'mean', 'std' and 'psnr' keep their bits either way.  With ``fuse=True`` the x tiles of the last solver row are
    measured, before their blend, per posterior sample: counts and sums are added in sample order, min / max folded, and
    a map needs ``samples == 1``.  At most 4 prediction channels.

    ``consistency=True`` (an ``InputStackTiledPred``) adds ``out['consistency']``: how far the stitched mean is from adding
    back up to the acquisition, ``r = x - sum_c w_c p_c`` in raw counts, per frame and in total
    (``core.consistency.consistency``: rms, bias, relative residual, saturated pixels and, with ``return_std``, the
    ``chi2`` of the spread), with ``consistency_weights`` (w_c, default ones) and ``consistency_noise`` (rho in counts).
    ``consistency="project"`` also replaces ``out['mean']`` and, where present, ``out['std']`` by the posterior
    conditioned on that observation, keeps the unprojected mean under ``out['mean_raw']`` and reports the residual before
    the projection.  One pass over the stitched canvases on every rank, no collective: any number of ranks gives the
    same bits.  Quantile and rank maps are NOT projected: asking for them together with "project" is refused.  Refused
    too: a dataset that exposes no acquisition, a ``target_channel_idx`` prediction, weights of another length.
    Without the argument nothing changes."""
    samples = _check_samples("predict_stack", samples, ValueError)
    plan = dataset.plan
    measure = _check_disagreement("predict_stack", disagreement, seam_band, netG.prediction_channels if disagreement else None)
    _check_solver("predict_stack", netG, solver)
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
    blend, field = stitch == "blend", noise == "field"
    q, ranks = _check_quantiles("predict_stack", samples, quantiles, ranks, dataset, blend=blend and not fuse)
    cons = _check_consistency("predict_stack", consistency, consistency_noise, consistency_weights, dataset,
                              netG.prediction_channels, q, ranks)
    if fuse:
        from .frame_predict import _predict_stack_fused
        _check_field_ids("predict_stack", samples, plan.data_shape[0])
        if q is not None or ranks:
            _check_quantile_bytes("predict_stack", samples, plan, netG.prediction_channels, quantile_bytes)
        _check_frame_map("predict_stack", "fuse=True", measure, samples)
        out = _predict_stack_fused(netG, dataset, batch_tiles, samples, return_std, seed, solver, window, q, ranks,
                                   FrameDisagreement(plan, measure, seam_band) if measure else None)
        return _apply_consistency(out, dataset, cons), plan
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
        _check_field_ids("predict_stack", samples, plan.data_shape[0], getattr(netG, "STREAM2_BIT", 1 << 39))
    C_out = netG.prediction_channels
    gt = _scorable_gt(dataset, C_out)
    _check_rank_gt("predict_stack", ranks, gt)
    ids = parallel.shard_ids(plan.total, parallel.rank(), parallel.world_size())
    # a rank without tiles still joins the collectives, on the device it is bound to
    dev = dataset.device if len(ids) else torch.device("cuda", torch.cuda.current_device())
    ex = TileExchange(plan, C_out, dev, group, gt=gt, blend=blend, window=window, disagreement=measure,
                      seam_band=seam_band)
    ex_std = TileExchange(plan, C_out, dev, group, blend=blend, window=window) if return_std else None
    ex_q = [TileExchange(plan, C_out, dev, group, blend=blend, window=window) for _ in q or ()]
    ex_rank = TileExchange(plan, C_out, dev, group) if ranks else None
    draws = None                                                      # (samples, B, C, p, p): the draws of one batch
    if (q is not None or ranks) and len(ids):
        draws = torch.empty((samples, min(int(batch_tiles), len(ids)), C_out) + tuple(plan.patch_shape[1:]),
                            dtype=torch.float32, device=dev)
    kept_field = getattr(netG, "noise_field", None)
    try:
        for i in range(0, len(ids), batch_tiles):
            chunk = ids[i:i + batch_tiles]
            x = dataset.tiles(chunk)["input"]

            def sample(r):
                kw = {}
                if field:
                    # (shape, draw[, id_bit]): the crops of this batch's tiles out of the fields of sample r; a joint
                    # sampler's second child adds its bit to the field ids
                    netG.noise_field = lambda shape, draw, id_bit=0: plan.randn_field(
                        chunk, shape[1], seed, draw, id_base=r * plan.data_shape[0] + id_bit, device=x.device)
                elif seed is not None:
                    kw = dict(seed=seed, sample_ids=[k + r * plan.total for k in chunk])
                return sample_tiles(netG, x, num_timesteps, solver, **kw)
            if draws is None:
                tiles, spread = _mean_and_spread(samples, return_std, sample)
            else:
                tiles, spread, quant, rank = _mean_spread_quantiles(
                    samples, return_std, sample, draws[:, :len(chunk)], q,
                    plan.gather_canvas(gt, chunk) if ranks else None)
                for k, e in enumerate(ex_q):
                    e.add(quant[k], chunk)
                if ranks:
                    ex_rank.add(rank, chunk)
            ex.add(tiles, chunk)
            if return_std:
                ex_std.add(spread, chunk)
    finally:
        if field:
            netG.noise_field = kept_field
            for child in (getattr(netG, "indi1", None), getattr(netG, "indi2", None)):
                if child is not None:                                 # a joint sampler hands its field down per call
                    child.noise_field = None
    res = ex.finish()
    out = {"mean": res[0], "psnr": res[1]} if gt is not None else {"mean": res}
    if return_std:
        out["std"] = ex_std.finish()
    if q is not None:
        out["quantiles"] = torch.stack([e.finish() for e in ex_q])
    if ranks:
        out["rank"] = ex_rank.finish()
    if measure:
        out["disagreement"] = ex.disagreement
    return _apply_consistency(out, dataset, cons), plan
