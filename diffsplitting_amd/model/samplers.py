"""The reverse-sampling loops behind the reference's sampler classes.

Each class keeps the reference's constructor / method signatures and return
shapes and drives ``UNetEngine.sample_loop`` (a captured
hipGraph per step).  ``forward`` / ``p_losses`` evaluate the training objective's forward half on the device
(one noising launch, one UNet forward, one reduction) under ``torch.no_grad()``: the UNet always runs with eval
semantics (dropout is identity), so the value is the validation objective and carries no graph.
Training itself (backward, optimiser) stays out of scope.  The single reverse steps (``p_mean_variance``, ``p_sample``,
``inference_one_step``) and ``interpolate`` let a caller drive the loop: one UNet forward and one
``dsx_posterior_step`` launch per step.

Noise: where a call's normals come from is decided once, by the ``Draws`` object (``model/draws.py``) every public
sampling entry builds first -- it refuses what does not go together before anything is drawn -- and asks for the
initial state, for the loop's ``noise`` / ``seed`` / ``sample_ids`` keywords or for a single step's.  Which rows of a
loop add noise is each sampler's ``noise_rows``.  By default the per-step noise is drawn on the device (Philox, seeded
from torch's generator); set ``noise_source`` to a ``randn(shape)`` callable to inject host draws in the reference's
draw order (parity mode, Q4).

Per-sample noise streams (opt-in, include/dsx.h): the sampling loops take ``seed=`` and ``sample_ids=`` (B integers);
the single steps keep the reference's signatures and have the siblings ``p_sample_seeded`` /
``inference_one_step_seeded``.
Every draw of sample ``b`` -- the initial state, draw 0, and step ``s``, draw ``s + 1`` -- then is a function of
``(seed, sample_ids[b], draw, element)`` alone: the same whatever batch, batch position or rank the sample runs in.
torch's generator is not touched, and a ``noise_source`` together with ids is refused.

Draws by ordinal: ``noise_field``, a callable ``(shape, draw) -> CUDA fp32 tensor``, is asked for the initial state
(draw 0) and for the noise of step ``s`` (draw ``s + 1``) of every sampling loop, which then runs on these draws in the
injected form; a step that adds no noise keeps its ordinal.  Tiled prediction sets it to noise cut from a frame-keyed
field (``TilePlan.randn_field``).  Together with ``noise_source`` or ``sample_ids`` it is refused; torch's generator is
not touched.  The single steps, the objective and ``interpolate`` do not consult it (a known gap).

Few-step sampling (Gaussian samplers only): ``solver_sample_loop`` runs a sub-sequence of the trained schedule with
DDIM(eta) or DPM-Solver++(2M) rows (``model/solvers.py``) through ``UNetEngine.solver_loop``; ``p_sample_loop`` and
the other methods keep their parameter lists.
"""
import numpy as np
import torch
from torch import nn

from .. import engine
from .._lib import DsxError
from . import solvers
from .draws import Draws


class _SamplerBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.noise_source = None      # callable(shape) -> CPU/GPU tensor; None = device RNG
        self.noise_field = None       # callable(shape, draw ordinal) -> CUDA fp32 tensor; None = the sources above
        self.use_graph = True
        self.last_full_batch = None   # final state of the whole batch (Q1 keeps only one element)

    STREAM2_BIT = 1 << 39            # JointIndi: the second sampler's ids carry this bit, callers' ids stay below it

    def _draws(self, B, seed=None, sample_ids=None, field=True):
        """The ``Draws`` of one call on a batch of ``B``, built -- and everything refused -- before anything is drawn.
        ``field=False``: a call that does not consult ``noise_field`` (single steps, the objective, ``interpolate``)."""
        return Draws(self.noise_source, self.noise_field if field else None, seed, sample_ids, B)

    def forward(self, x, *args, **kwargs):
        """The objective's forward evaluation (``p_losses``); no gradients, eval semantics."""
        return self.p_losses(x, *args, **kwargs)

    def get_current_log(self):
        return {}

    # ---- the objective's forward half (dsx_q_sample / dsx_loss) ---------------------------
    @staticmethod
    def _need_cuda(*tensors, what=None):
        for t in tensors:
            if not t.is_cuda:
                raise DsxError("the objective runs on the MI355X only; pass CUDA tensors (no CPU fallback)" if what is None
                               else f"{what} runs on the MI355X only; pass a CUDA tensor (no CPU fallback)")

    def _set_loss(self, device, reduction):
        if self.loss_type not in ("l1", "l2"):
            raise NotImplementedError("loss_type {!r}: only 'l1' and 'l2' exist".format(self.loss_type))
        if reduction not in ("sum", "mean"):
            raise NotImplementedError("loss reduction {!r}: only 'sum' and 'mean' are built".format(reduction))
        self._device, self._reduction = device, reduction

    def _loss(self, a, b):
        """nn.L1Loss / nn.MSELoss(reduction)(a, b) as a 0-dim fp32 device tensor: per-sample sums in double on the
        device (dsx_loss), added in double, divided by the element count for 'mean', rounded to fp32 once."""
        if getattr(self, "_reduction", None) is None:
            raise DsxError("set_loss() first")
        if a.shape != b.shape:       # torch's losses broadcast (a 1-channel noise against a wider UNet output)
            a, b = torch.broadcast_tensors(a, b)
        a, b = a.float().contiguous(), b.float().contiguous()      # no copy for what the samplers themselves produce
        total = engine.loss_per_sample(a, b, squared=self.loss_type == "l2").sum()
        if self._reduction == "mean":
            total = total / a.numel()
        return total.to(torch.float32)

    def _q_args(self, x_start, coef, noise):
        """What engine.q_sample takes: x_start as contiguous float32 (a copy only when the caller's is not), the
        coefficients (c0, c1, c2) on the device, and the draws (z, seed): ``noise``, or a single step's."""
        dev = x_start.device
        x_start = x_start.float().contiguous()
        zkw = self._draws(x_start.shape[0], field=False).step(x_start.shape, dev, noise=noise)
        c0, c1, c2 = (None if c is None else c.to(dev).contiguous() for c in coef)
        return x_start, c0, c2, dict(c1=c1, **zkw)

    def _q_sample(self, x_start, coef, noise, x_end=None):
        """The public q_sample of the three families: one dsx_q_sample launch."""
        x_start, c0, c2, kw = self._q_args(x_start, coef, noise)
        xe = None if x_end is None else x_end.float().contiguous()
        return engine.q_sample(x_start, c0, c2, xe=xe, **kw)[0]

    @staticmethod
    def _unet_input(cond, x):
        """The buffer of cat([cond, x], 1) with ``cond`` written and x's channels left to the caller, and where those
        begin; (None, 0) without a condition."""
        if cond is None:
            return None, 0
        cc = cond.shape[1]
        inp = torch.empty((x.shape[0], cc + x.shape[1]) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        inp[:, :cc] = cond
        return inp, cc

    def _noised_forward(self, x_start, coef, time, noise, cond=None, xe=None, want_noise=True):
        """x_noisy = q_sample(x_start) written straight into the UNet's input (behind ``cond``'s channels when the
        model is conditional), then the UNet forward.  ``coef`` = (c0, c1, c2), (B,) each (c1 None: two terms).
        Returns (x_recon, the normals used or None)."""
        x_start, c0, c2, kw = self._q_args(x_start, coef, noise)
        inp, coff = self._unet_input(cond, x_start)
        inp, z = engine.q_sample(x_start, c0, c2, xe=xe, dst=inp, coff=coff, want_z=want_noise, **kw)
        return self.denoise_fn(inp, time.to(x_start.device)), z

    @property
    def prediction_channels(self):
        """Channels of ``last_full_batch`` (what tiled prediction stitches)."""
        return int(getattr(self, "out_channel", None) or self.channels)


class GaussianSampler(_SamplerBase):
    """SR3 / DDPM ancestral sampling (sr3 diffusion.py:141-213, ddpm diffusion.py:194-247)."""

    kind = "sr3"

    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", conditional=True,
                 schedule_opt=None, **unused):
        # `unused` swallows out_channel / lr_reduction / val_schedule_opt that define_G always
        # passes (networks.py:159-170, rot R1)
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.conditional = conditional
        self.num_timesteps = None
        self._table = {}

    def set_loss(self, device):
        self._set_loss(device, "sum")                                # sr3 diffusion.py:84-90: always reduction='sum'

    def set_new_noise_schedule(self, schedule_opt, device):
        bufs, gamma = engine.gaussian_buffers(schedule_opt)
        self.sqrt_alphas_cumprod_prev = gamma                    # float64 numpy, as in the reference
        self.num_timesteps = int(bufs["betas"].shape[0])
        for k, v in bufs.items():                                # same buffer names as diffusion.py:104-139
            if hasattr(self, k):
                delattr(self, k)
            self.register_buffer(k, v.to(device))
        self._bufs_cpu, self._table = bufs, {}
        self._ac64 = solvers.alphas_cumprod_f64(schedule_opt)    # float64: the few-step solvers' rows start from it

    def _step_table(self, clip):
        if clip not in self._table:
            self._table[clip] = engine.gaussian_step_table(self._bufs_cpu, self.sqrt_alphas_cumprod_prev,
                                                           self.kind, clip)
        return self._table[clip]

    def _need_schedule(self):
        if self.num_timesteps is None:
            raise DsxError("set_new_noise_schedule() first")

    @torch.no_grad()
    def p_sample_loop(self, x_in, clip_denoised=True, continous=False, seed=None, sample_ids=None):
        """``seed`` / ``sample_ids``: per-sample noise streams -- the initial state is ``randn_samples(draw=0)``, step
        ``s`` takes draw ``s + 1``; torch's generator is not touched."""
        self._need_schedule()
        table = self._step_table(bool(clip_denoised))
        snaps = engine.gaussian_snapshot_steps(self.num_timesteps) if continous else []
        return self._run("sample_loop", table, self.noise_rows(), snaps, x_in, continous, seed, sample_ids)

    def noise_rows(self, table=None):
        """The rows of a loop that add noise.  The ancestral loop follows the reference's draw order: one draw per row,
        none at t == 0 for sr3 (its last row; ddpm draws there and masks it).  The rows of a solver ``table``: those
        with sigma != 0 -- none for dpmpp2m and ddim with eta = 0, every row but the last for eta > 0."""
        if table is not None:
            return [s for s in range(table.n_steps) if table.sigma[s] != 0]
        self._need_schedule()
        return range(self.num_timesteps - 1 if self.kind == "sr3" else self.num_timesteps)

    def _run(self, loop, table, rows, snaps, x_in, continous, seed, sample_ids):
        """The reverse loop ``loop`` of the engine over ``table``, of which ``rows`` add noise, from draw 0, and what
        the reference returns of it."""
        dev = self.betas.device
        if not self.conditional:
            shape, cond = tuple(x_in), None
        else:
            cond = x_in.to(dev).float()
            shape = (cond.shape[0], self.channels) + tuple(cond.shape[2:])
        draws = self._draws(shape[0], seed, sample_ids)
        img = draws.initial(shape, dev)
        # the loop updates `img` in place: keep a copy of the initial noise for ret_img[0] (sr3 diffusion.py:183-185)
        first = (img.clone() if continous else None) if cond is None else cond.repeat((1, self.channels // cond.shape[1], 1, 1))
        x, sn = getattr(self.denoise_fn.engine(), loop)(table, img, cond=cond, snapshot_steps=snaps,
                                                        use_graph=self.use_graph,
                                                        **draws.loop(shape, table.n_steps, rows, dev))
        self.last_full_batch = x
        if self.kind == "ddpm" and not self.conditional:
            return x                                                 # ddpm diffusion.py:222
        if continous:
            return torch.cat([first] + [s for s in sn], dim=0)
        return x[-1]                                                 # diffusion.py:200-203: ret_img[-1]

    def solver_table(self, steps=50, solver="dpmpp2m", eta=0.0, spacing=None, timesteps=None, clip_denoised=True):
        """The rows ``solver_sample_loop`` runs (``model/solvers.py``): a ``SolverTableHost`` with its ``timesteps``."""
        self._need_schedule()
        return solvers.solver_table(self._bufs_cpu, self.sqrt_alphas_cumprod_prev, self.kind, self._ac64, solver=solver,
                                    steps=None if timesteps is not None else steps, eta=eta, spacing=spacing,
                                    timesteps=timesteps, clip_denoised=bool(clip_denoised))

    @torch.no_grad()
    def solver_sample_loop(self, x_in, steps=50, solver="dpmpp2m", eta=0.0, spacing=None, timesteps=None,
                           clip_denoised=True, continous=False, seed=None, sample_ids=None):
        """Few-step sampling over a sub-sequence of the trained schedule: ``solver`` "ddim" (deterministic, or stochastic
        with ``eta`` in (0, 1]) or "dpmpp2m" (DPM-Solver++(2M), second order).  The run is ``timesteps`` (strictly
        descending) or ``steps`` timesteps spaced by ``spacing`` ("uniform" / "logsnr"; default: logsnr for dpmpp2m,
        uniform for ddim).  Initial state, ``noise_source``, ``seed`` / ``sample_ids`` and the return value as
        ``p_sample_loop``; ``continous=True`` returns the start followed by the state after every row."""
        table = self.solver_table(steps, solver, eta, spacing, timesteps, clip_denoised)
        if self.conditional:
            self._need_cuda(x_in, what="solver_sample_loop")
        snaps = range(table.n_steps) if continous else ()
        return self._run("solver_loop", table, self.noise_rows(table), snaps, x_in, continous, seed, sample_ids)

    @torch.no_grad()
    def sample(self, batch_size=1, continous=False, seed=None, sample_ids=None):
        return self.p_sample_loop((batch_size, self.channels, self.image_size, self.image_size),
                                  continous=continous, seed=seed, sample_ids=sample_ids)

    @torch.no_grad()
    def super_resolution(self, x_in, clip_denoised=True, continous=False, seed=None, sample_ids=None):
        return self.p_sample_loop(x_in, clip_denoised=clip_denoised, continous=continous, seed=seed,
                                  sample_ids=sample_ids)

    predict = super_resolution                                       # ddpm diffusion.py:245-247

    # ---- caller-driven reverse steps (sr3 diffusion.py:141-175, ddpm diffusion.py:163-203) ------------------
    def _rows(self, t, B, dev):
        """The step-table rows of ``t`` (an integer, or (B,) integers) as (B,) fp32 device tensors per column."""
        self._need_schedule()
        if torch.is_tensor(t):
            t = t.detach().reshape(-1).cpu()
            if t.numel() != B:
                raise DsxError(f"t must hold B = {B} timesteps, got {t.numel()}")
        rows = engine.gaussian_step_rows(self._bufs_cpu, self.sqrt_alphas_cumprod_prev, self.kind, t)
        return {k: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,)))).to(dev) for k, v in rows.items()}

    def _reverse(self, x, t, clip_denoised, condition_x, want, repeat_noise=False, **noise):
        """One UNet forward and one dsx_posterior_step launch: ``want`` = (x_recon, model_mean, sample) flags, the
        wanted ones are returned as new tensors, the others as None.  ``noise``: the keywords of ``Draws.step``."""
        self._need_cuda(x, *(() if condition_x is None else (condition_x,)))
        x = x.float().contiguous()
        B = x.shape[0]
        r = self._rows(t, B, x.device)
        time = r["tcond"].view(B, 1) if self.kind == "sr3" else r["tcond"]
        inp, cc = self._unet_input(condition_x, x)
        if inp is None:
            inp = x
        else:
            inp[:, cc:] = x
        net = self.denoise_fn(inp, time)
        outs = [torch.empty_like(x) if w else None for w in want]
        return engine.posterior_step(x, net, r["c1"], r["c2"], r["sigma"], a=r["a"], b=r["b"], predict_eps=True,
                                     clip=bool(clip_denoised), repeat_noise=repeat_noise, x_recon_out=outs[0],
                                     mean_out=outs[1], x_out=outs[2], **noise)

    def _step_draw(self, t, draw):
        """The draw ordinal of the reverse step at timestep ``t``: ``T - t``, what the loop uses there (its step
        ``s = T - 1 - t`` takes draw ``s + 1``), unless the caller names one."""
        if draw is not None:
            return int(draw)
        self._need_schedule()
        if torch.is_tensor(t):
            ts = set(int(v) for v in t.detach().reshape(-1).cpu().tolist())
            if len(ts) != 1:
                raise DsxError("sample_ids with differing timesteps: pass draw=, one ordinal serves the whole call")
            t = ts.pop()
        return self.num_timesteps - int(t)

    @torch.no_grad()
    def predict_start_from_noise(self, x_t, t, noise):
        self._need_cuda(x_t, noise)
        x_t = x_t.float().contiguous()
        r = self._rows(t, x_t.shape[0], x_t.device)
        return engine.posterior_step(x_t, noise.float().contiguous(), r["c1"], r["c2"], r["sigma"], a=r["a"], b=r["b"],
                                     predict_eps=True, x_recon_out=torch.empty_like(x_t))[0]

    @torch.no_grad()
    def q_posterior(self, x_start, x_t, t):
        self._need_cuda(x_start, x_t)
        x_t = x_t.float().contiguous()
        r = self._rows(t, x_t.shape[0], x_t.device)
        mean = engine.posterior_step(x_t, x_start.float().contiguous(), r["c1"], r["c2"], r["sigma"],
                                     mean_out=torch.empty_like(x_t))[1]
        return mean, self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_mean_variance(self, x, t, clip_denoised: bool, condition_x=None):
        mean = self._reverse(x, t, clip_denoised, condition_x, (False, True, False))[1]
        return mean, self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, condition_x=None):
        """One draw per call, none at t == 0 (sr3 diffusion.py:174)."""
        self._need_cuda(x)
        noise = self._draws(x.shape[0], field=False).step(x.shape, x.device) if t > 0 else {}
        return self._reverse(x, t, clip_denoised, condition_x, (False, False, True), **noise)[2]

    @torch.no_grad()
    def p_sample_seeded(self, x, t, seed, sample_ids, clip_denoised=True, condition_x=None, draw=None):
        """``p_sample`` with per-sample noise streams (``p_sample`` itself keeps the reference's signature): the draw
        the loop takes at this timestep from the streams (seed, sample_ids[b]) -- ``draw`` = T - t unless given -- so
        the caller's loop from ``randn_samples(draw=0)`` reproduces ``p_sample_loop`` with the same ids bit for bit.
        ``t``: an integer, or (B,) equal integers (ddpm)."""
        self._need_cuda(x)
        draws = self._draws(x.shape[0], seed, sample_ids, field=False)
        if draws.streams is None:
            raise DsxError("p_sample_seeded needs sample_ids (p_sample draws without them)")
        return self._reverse(x, t, clip_denoised, condition_x, (False, False, True),
                             **draws.step(x.shape, x.device, draw=self._step_draw(t, draw)))[2]

    # ---- objective (sr3 diffusion.py:215-249) -----------------------------------------------
    def q_coefficients(self, continuous_sqrt_alpha_cumprod):
        """(c0, c2) of q_sample for the (B,) fp32 noise levels: the reference's own torch expressions."""
        c = continuous_sqrt_alpha_cumprod.reshape(-1).to(torch.float32)
        return c, (1 - c ** 2).sqrt()

    @torch.no_grad()
    def q_sample(self, x_start, continuous_sqrt_alpha_cumprod, noise=None):
        """c*x_start + sqrt(1 - c^2)*noise in one launch; ``noise`` None draws on the device (Philox)."""
        self._need_cuda(x_start)
        c0, c2 = self.q_coefficients(continuous_sqrt_alpha_cumprod)
        return self._q_sample(x_start, (c0, None, c2), noise)

    def _sample_gamma(self, b, t=None):
        """The host draws of p_losses in the reference's order (sr3 diffusion.py:227-234): (t, (b,) fp32 levels)."""
        if t is None:
            t = np.random.randint(1, self.num_timesteps + 1)
        g = self.sqrt_alphas_cumprod_prev
        return t, torch.FloatTensor(np.random.uniform(g[t - 1], g[t], size=b))

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, *, t=None, continuous_sqrt_alpha_cumprod=None):
        """The objective on ``x_in`` = {'target', 'input'}: loss(noise, UNet(q_sample(target))) with eval semantics
        (dropout is identity: the validation objective), no graph.  ``t`` / ``continuous_sqrt_alpha_cumprod``
        override the host draws (a superset of the reference's signature)."""
        self._need_cuda(x_in["target"])
        b = x_in["target"].shape[0]
        c = continuous_sqrt_alpha_cumprod
        if c is None:
            c = self._sample_gamma(b, t)[1]
        return self._objective(x_in, noise, c.reshape(b, -1).to(torch.float32))

    def _objective(self, x_in, noise, time):
        """loss(noise, UNet(q_sample(target), time)): ``time`` -- noise levels (sr3) or integer steps (ddpm) -- is what
        q_coefficients reads and what the UNet is conditioned on."""
        x_start = x_in["target"]
        c0, c2 = self.q_coefficients(time)
        cond = x_in["input"].to(x_start.device).float() if self.conditional else None
        x_recon, z = self._noised_forward(x_start, (c0, None, c2), time, noise, cond=cond)
        return self._loss(z, x_recon)


class GaussianSamplerDdpm(GaussianSampler):
    kind = "ddpm"

    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", lr_reduction=None,
                 conditional=True, schedule_opt=None, **unused):
        super().__init__(denoise_fn, image_size, channels, loss_type, conditional, schedule_opt)
        self.lr_reduction = lr_reduction or "sum"

    def set_loss(self, device):
        self._set_loss(device, self.lr_reduction)                    # ddpm diffusion.py:96-107

    # ---- forward process (ddpm diffusion.py:156-177, 266-300): gathers from the registered buffers --------------
    @staticmethod
    def _extract(a, t, x_shape):
        out = a.gather(-1, t.to(a.device))
        return out.reshape(t.shape[0], *((1,) * (len(x_shape) - 1)))

    def q_mean_variance(self, x_start, t):
        mean = self._extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = self._extract(1. - self.alphas_cumprod, t, x_start.shape)
        log_variance = self._extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def predict_start_from_noise(self, x_t, t, noise):
        return (self._extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t -
                self._extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        posterior_mean = (self._extract(self.posterior_mean_coef1, t, x_t.shape) * x_start +
                          self._extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = self._extract(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = self._extract(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    # ---- caller-driven reverse steps (ddpm diffusion.py:179-264): t is a (B,) long tensor, entries may differ ----
    @torch.no_grad()
    def p_mean_variance(self, x, t, clip_denoised: bool, condition_x=None):
        mean = self._reverse(x, t, clip_denoised, condition_x, (False, True, False))[1]
        return (mean, self._extract(self.posterior_variance, t, x.shape),
                self._extract(self.posterior_log_variance_clipped, t, x.shape))

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, repeat_noise=False, condition_x=None):
        """The draw is taken on every call -- (1, C, H, W) under ``repeat_noise`` -- and a sample at t == 0 gets none of
        it (the reference's nonzero_mask, ddpm diffusion.py:199-203)."""
        self._need_cuda(x)
        shape = ((1,) + tuple(x.shape[1:])) if repeat_noise else tuple(x.shape)
        return self._reverse(x, t, clip_denoised, condition_x, (False, False, True), repeat_noise=bool(repeat_noise),
                             **self._draws(x.shape[0], field=False).step(shape, x.device))[2]

    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5):
        """(1 - lam)*q_sample(x1, t) + lam*q_sample(x2, t) in one launch, then the steps i = t-1 .. 0 through the
        engine's loop; returns the whole batch.  Draws: x1's, x2's, then one per step."""
        if self.conditional:
            raise DsxError("interpolate: the reference steps without a condition (ddpm diffusion.py:260-262); a "
                           "conditional sampler cannot interpolate")
        self._need_cuda(x1, x2)
        self._need_schedule()
        t = self.num_timesteps - 1 if t is None else int(t)
        assert x1.shape == x2.shape
        if not 0 <= t < self.num_timesteps:
            raise DsxError(f"interpolate: t must lie in 0..{self.num_timesteps - 1}, got {t}")
        dev = x1.device
        b = x1.shape[0]
        c0, c2 = self.q_coefficients(torch.full((b,), t, dtype=torch.long))
        draws = self._draws(b, field=False)                          # noise_field is not consulted
        start = draws.step(x1.shape, dev)                            # x1's draw, or the seed of both
        z1 = start["z"]
        z2 = None if z1 is None else draws.normal(x1.shape, dev).contiguous()
        img = engine.interp_start(x1.float().contiguous(), x2.float().contiguous(), c0.to(dev).contiguous(),
                                  c2.to(dev).contiguous(), lam, z1=z1, z2=z2, seed=start["seed"])
        if t == 0:
            return img
        table = engine.gaussian_step_table(self._bufs_cpu, self.sqrt_alphas_cumprod_prev, self.kind, True, start=t)
        x, _ = self.denoise_fn.engine().sample_loop(table, img, use_graph=self.use_graph,
                                                    **draws.loop(x1.shape, t, range(t), dev))
        self.last_full_batch = x
        return x

    def q_coefficients(self, t):
        """(c0, c2) of q_sample for integer ``t`` (B,): gathered from the schedule buffers."""
        t = t.reshape(-1).long().to(self.betas.device)
        return self.sqrt_alphas_cumprod.gather(-1, t), self.sqrt_one_minus_alphas_cumprod.gather(-1, t)

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None):
        self._need_cuda(x_start)
        c0, c2 = self.q_coefficients(t)
        return self._q_sample(x_start, (c0, None, c2), noise)

    def _sample_t(self, b):
        """ddpm diffusion.py:288: drawn from torch's CPU generator."""
        return torch.randint(0, self.num_timesteps, (b,)).long()

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, *, t=None):
        """loss(noise, UNet(q_sample(target, t), t)) with eval semantics (the validation objective), no graph.
        ``t`` (B,) integer overrides the host draw."""
        self._need_cuda(x_in["target"])
        if t is None:
            t = self._sample_t(x_in["target"].shape[0])
        return self._objective(x_in, noise, t.reshape(-1).long())


class InDISampler(_SamplerBase):
    """InDI.inference (ddpm_modules/indi.py:62-110)."""

    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", out_channel=2, lr_reduction=None,
                 conditional=True, schedule_opt=None, val_schedule_opt=None, e=0.01, **unused):
        super().__init__()
        self.denoise_fn = denoise_fn
        self.image_size, self.channels, self.loss_type = image_size, channels, loss_type
        self.out_channel = out_channel
        self.conditional = conditional
        self.lr_reduction = lr_reduction or "sum"
        self.e = e
        self._t_sampling_mode = "linear_indi"                        # indi.py:32-39
        self._linear_indi_a = 1.0
        self._noise_mode = "gaussian"
        self.num_timesteps = None
        self.val_num_timesteps = val_schedule_opt["n_timestep"] if val_schedule_opt else None

    def set_loss(self, device):
        self._set_loss(device, self.lr_reduction)                    # ddpm diffusion.py:96-107

    def set_new_noise_schedule(self, schedule_opt, device):
        self.num_timesteps = schedule_opt["n_timestep"]              # indi.py:46-47

    # ---- objective (indi.py:98-175) -----------------------------------------------------------
    def _gaussian_noise_mode(self):
        if self._noise_mode not in ("gaussian", "none"):
            raise NotImplementedError("noise mode {!r} is not built (only 'gaussian'): 'brownian' is refused"
                                      .format(self._noise_mode))

    def get_e(self, t):
        self._gaussian_noise_mode()
        return self.e if self._noise_mode == "gaussian" else 0.0

    def get_t_times_e(self, t):
        return self.get_e(t) * t

    def q_coefficients(self, t):
        """(c0, c1, c2) = (1 - t, t, e*t) of q_sample for the (B,) fp32 times: the reference's own expressions."""
        t = t.reshape(-1).to(torch.float32)
        return 1 - t, t, self.get_t_times_e(t)

    @torch.no_grad()
    def q_sample(self, x_start, x_end, t, noise=None):
        """(1-t)*x_start + t*x_end + noise*(e*t) in one launch.  ``x_end`` (B, Ce, H, W) with C % Ce == 0 stands
        for its channel-wise repetition to C channels (indi.py:157)."""
        assert 0 < t.min(), "t > 0"
        assert t.max() <= 1, "t <= 1. but t is {}".format(t.max())
        self._need_cuda(x_start, x_end)
        if x_start.shape[1] % x_end.shape[1] != 0:
            raise DsxError("x_end has {} channels, x_start {}: C % Ce != 0".format(x_end.shape[1], x_start.shape[1]))
        return self._q_sample(x_start, self.q_coefficients(t), noise, x_end=x_end)

    def _draw_t_linear_indi(self, batch_size, hi, maxv):
        """randint(1, hi), then with probability 1 - 1/(a + 1) the value maxv (indi.py:141-147)."""
        t = torch.randint(1, hi, (batch_size,)).long()
        alpha = 1 / (self._linear_indi_a + 1)
        probab = torch.rand(t.shape)
        t[probab > alpha] = maxv
        return t

    def _draw_t(self, batch_size):
        n = self.num_timesteps
        mode = self._t_sampling_mode
        if mode in ("linear_ramp", "quadratic_ramp"):
            p = torch.arange(n) if mode == "linear_ramp" else torch.arange(n) ** 2   # P(t = 0) = 0
            return torch.multinomial(p / torch.sum(p), batch_size, replacement=True).long()
        if mode == "uniform":
            return torch.randint(1, n + 1, (batch_size,)).long()
        if mode == "uniform_in_range":
            return torch.randint((2 * n) // 3, n + 1, (batch_size,)).long()
        if mode == "linear_indi":
            return self._draw_t_linear_indi(batch_size, n, n)
        raise NotImplementedError("t sampling mode {!r}".format(mode))

    def sample_t(self, batch_size, device):
        """indi.py:126-150: drawn from torch's CPU generator (pure host logic), then moved to ``device``."""
        return (self._draw_t(batch_size) / self.num_timesteps).to(device)

    @torch.no_grad()
    def get_prediction_during_training(self, x_in, noise=None, *, t=None):
        """UNet(q_sample(target, input, t), t) with eval semantics (dropout is identity), no graph.  ``t`` (B,)
        overrides the host draw."""
        x_start, x_end = x_in["target"], x_in["input"]
        self._need_cuda(x_start, x_end)
        assert self.conditional is False
        if x_end.shape[1] * self._copies(x_end) != x_start.shape[1]:
            raise DsxError("input has {} channels, repeated to out_channel {} != target's {}".format(
                x_end.shape[1], self.out_channel, x_start.shape[1]))
        t_float = self.sample_t(x_start.shape[0], "cpu") if t is None else t.reshape(-1).to(torch.float32)
        assert 0 < t_float.min(), "t > 0"
        assert t_float.max() <= 1, "t <= 1. but t is {}".format(t_float.max())
        x_recon, _ = self._noised_forward(x_start, self.q_coefficients(t_float), t_float, noise,
                                          xe=x_end.float().contiguous(), want_noise=False)
        return x_recon

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, *, t=None):
        """loss(target, get_prediction_during_training(x_in)): the validation objective, no graph."""
        x_recon = self.get_prediction_during_training(x_in, noise=noise, t=t)
        return self._loss(x_in["target"], x_recon)

    # ---- the Gaussian methods InDI overrides away (indi.py:50-60,112-114) -----------------------------------
    def q_mean_variance(self, x_start, t):
        raise NotImplementedError("This is not needed.")

    def predict_start_from_noise(self, x_t, t, noise):
        raise NotImplementedError("This is not needed.")

    def q_posterior(self, x_start, x_t, t):
        raise NotImplementedError("This is not needed.")

    def p_mean_variance(self, x, t, clip_denoised: bool, condition_x=None):
        raise NotImplementedError("This is not needed.")

    def interpolate(self, x1, x2, t=None, lam=0.5):
        raise NotImplementedError("This is not needed.")

    @torch.no_grad()
    def inference_one_step(self, x_t, delta_t, t_cur):
        """indi.py:62-69: delta/t * UNet(x_t, t) + (1 - delta/t) * x_t + z * e (t - delta), one UNet forward and one
        dsx_posterior_step launch; the coefficients are one row of ``engine.indi_step_table``.  One draw per call."""
        return self._one_step(x_t, delta_t, t_cur, self._draws(x_t.shape[0], field=False), None)

    @torch.no_grad()
    def inference_one_step_seeded(self, x_t, delta_t, t_cur, seed, sample_ids, draw):
        """``inference_one_step`` with per-sample noise streams (``inference_one_step`` itself keeps the reference's
        signature): ``draw`` = s + 1 at the caller's step ``s`` is the draw ``inference`` takes there with the same
        ``seed`` and ``sample_ids``, so the caller's loop reproduces it bit for bit."""
        draws = self._draws(x_t.shape[0], seed, sample_ids, field=False)
        if draws.streams is None:
            raise DsxError("inference_one_step_seeded needs sample_ids (inference_one_step draws without them)")
        return self._one_step(x_t, delta_t, t_cur, draws, draw)

    def _one_step(self, x_t, delta_t, t_cur, draws, draw):
        assert delta_t <= t_cur, "delta_t should be less than or equal to t_cur."
        self._gaussian_noise_mode()
        self._need_cuda(x_t, what="inference_one_step")
        dev = x_t.device
        x_t = x_t.float().contiguous()
        B = x_t.shape[0]
        tc, c1, c2, sg = engine.indi_step_row(delta_t, t_cur, self.get_e(t_cur))
        col = lambda v: torch.full((B,), v, dtype=torch.float32, device=dev)
        x_0 = self.denoise_fn(x_t, torch.Tensor([tc]).to(dev))
        return engine.posterior_step(x_t, x_0, col(c1), col(c2), col(sg), predict_eps=False,
                                     x_out=torch.empty_like(x_t), **draws.step(x_t.shape, dev, draw=draw))[2]

    def _copies(self, x_in):
        """How often the input is repeated along the channels: to ``out_channel`` channels in all.  indi.py:80,157
        repeat ``out_channel`` times, which is the same for the one-channel inputs the reference runs on; on a colour
        input (3 planes, CIFAR's C1: UNet 6 -> 6, target 6 planes) that literal count gives 18 channels and the
        reference stops in its first conv with a shape error."""
        cin = x_in.shape[1]
        if self.out_channel % cin != 0:
            raise DsxError("out_channel {} is no multiple of the input's {} channels".format(self.out_channel, cin))
        return self.out_channel // cin

    def _repeated(self, x_in):
        return torch.cat([x_in.float()] * self._copies(x_in), dim=1)   # indi.py:80

    def _perturbed(self, x, d0, t_starts):
        """``x + d0 * e * t``, t the one start time or one per sample: get_t_times_e (indi.py:106-110), indi.py:82."""
        scale = torch.stack([self.e * torch.Tensor([t]) for t in t_starts]).to(x.device).view(-1, 1, 1, 1)
        return x + d0 * scale

    def _start(self, x_in, t_float_start, streams=None):
        """What ``inference`` starts from, for a caller that drives the steps itself: the input repeated to
        ``out_channel`` channels and perturbed by draw 0.  ``streams``: ``(seed, sample_ids)`` or None."""
        x = self._repeated(x_in)
        draws = self._draws(x.shape[0], *(streams or (None, None)))
        return self._perturbed(x, draws.initial(x.shape, x.device), [t_float_start])

    @staticmethod
    def _per_sample_t(t_float_start, batch):
        """None for the reference's scalar start time; else the B per-sample start times as python floats."""
        if torch.is_tensor(t_float_start):
            t = t_float_start.detach().reshape(-1).to("cpu", torch.float64).tolist()
        elif isinstance(t_float_start, (list, tuple)) or (hasattr(t_float_start, "shape") and getattr(t_float_start, "ndim", 0) > 0):
            t = [float(v) for v in t_float_start]
        else:
            return None
        if len(t) == 1:
            t = t * batch
        if len(t) != batch:
            raise DsxError(f"t_float_start has {len(t)} entries for a batch of {batch}")
        return t

    def noise_rows(self, n_steps):
        """The rows of a loop that add noise: every one (indi.py:62-69 draws on each step)."""
        return range(n_steps)

    @torch.no_grad()
    def inference(self, x_in, continuous=False, num_timesteps=None, t_float_start=1.0, eps=1e-8,
                  stream=None, seed=None, sample_ids=None):
        """``seed`` / ``sample_ids``: per-sample noise streams -- the start perturbation is draw 0 of every sample's
        stream, step ``s`` takes draw ``s + 1``; torch's generator is not touched.

        ``t_float_start`` with one start time per batch element runs one batched loop on per-sample step tables:
        equivalent to calling ``inference`` on every sample alone, as core/psnr_based_t_refinement.py:26-34 does; with a
        ``noise_source`` the draws are taken sample by sample in that order (start draw, then one draw per step)."""
        n = self.num_timesteps if num_timesteps is None else num_timesteps
        assert self.conditional is False
        self._need_cuda(x_in, what="inference")
        draws = self._draws(x_in.shape[0], seed, sample_ids)
        t_list = self._per_sample_t(t_float_start, x_in.shape[0])
        x = self._repeated(x_in)
        if t_list is None:
            d0, loop_kw = draws.initial(x.shape, x.device), draws.loop(x.shape, n, self.noise_rows(n), x.device)
            table = engine.indi_step_table(n, t_float_start, self.e)   # no drift assert (R3)
        else:                                                        # two tables: they select different captured steps
            d0, loop_kw = draws.per_sample(x.shape, n, x.device)
            table = engine.indi_step_table_per_sample(n, t_list, self.e)
        x_t = self._perturbed(x, d0, t_list or [t_float_start])
        # the engine's loop updates x_t in place: `first` keeps the start
        snaps = engine.indi_snapshot_steps(n) if continuous else []
        first = x_t.clone() if continuous else None
        x, sn = self.denoise_fn.engine().sample_loop(table, x_t, snapshot_steps=snaps, use_graph=self.use_graph,
                                                     stream=stream, **loop_kw)
        self.last_full_batch = x
        if continuous:
            if stream is not None:
                stream.synchronize()
            return torch.cat([first] + [s for s in sn], dim=0)
        return x[-1:]                                                # indi.py:92-95: ret_img[-1:]


class IndiCustomT(InDISampler):
    """joint_indi.py:10-22: t in (0, 0.5]."""

    def _draw_t(self, batch_size):
        assert self._t_sampling_mode == "linear_indi"
        assert self.num_timesteps % 2 == 0, "num_timesteps should be even since we are dividing it by 2 in the next line."
        maxv = int(self.num_timesteps * 0.5)
        return self._draw_t_linear_indi(batch_size, maxv, maxv)


class IndiFullTranslation(InDISampler):
    """joint_indi.py:24-36: t over the whole range, the point mass at 0.5."""

    def _draw_t(self, batch_size):
        assert self._t_sampling_mode == "linear_indi"
        assert self.num_timesteps % 2 == 0, "num_timesteps should be even since we are dividing it by 2 in the next line."
        return self._draw_t_linear_indi(batch_size, self.num_timesteps, int(self.num_timesteps * 0.5))


class JointIndiSampler(_SamplerBase):
    """JointIndi (ddpm_modules/joint_indi.py:40-149): indi1 at t0, indi2 at 1-t0; the two
    independent loops run concurrently on two HIP streams instead of back to back."""

    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", out_channel=2, lr_reduction=None,
                 denoise_fn_ch1=None, denoise_fn_ch2=None, conditional=True, schedule_opt=None,
                 val_schedule_opt=None, w_input_loss=0.0, e=0.01, allow_full_translation=False):
        super().__init__()
        assert denoise_fn_ch1 is not None and denoise_fn_ch2 is not None and denoise_fn is None
        kw = dict(channels=channels, loss_type=loss_type, out_channel=out_channel, lr_reduction=lr_reduction,
                  conditional=conditional, schedule_opt=schedule_opt, val_schedule_opt=val_schedule_opt, e=e)
        indi_class = IndiFullTranslation if allow_full_translation else IndiCustomT   # joint_indi.py:61
        self.indi1 = indi_class(denoise_fn_ch1, image_size, **kw)
        self.indi2 = indi_class(denoise_fn_ch2, image_size, **kw)
        self.val_num_timesteps = self.indi1.val_num_timesteps
        self.alpha_param = nn.Parameter(torch.tensor(0.0))           # kept for *_gen.pth compatibility
        self.offset_param = nn.Parameter(torch.tensor(0.0))
        self.scale_param = nn.Parameter(torch.tensor(1.0))
        self.w_input_loss = w_input_loss
        self.current_log_dict = {}
        self._streams = None
        self.concurrent = True        # the two loops on two HIP streams; False: back to back on the current stream

    @property
    def prediction_channels(self):
        return self.indi1.prediction_channels + self.indi2.prediction_channels   # joint_indi.py:135 (channel cat)

    def get_offset(self):
        return self.offset_param

    def get_scale(self):
        return self.scale_param

    def get_alpha(self):
        return torch.sigmoid(self.alpha_param)

    def get_current_log(self):
        return self.current_log_dict

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, *, t=None):
        """joint_indi.py:103-120: channel 0 is indi1's target with channel 1 as its input, the reverse for indi2;
        indi1's draws come first; the loss is (l1 + l2) / 2.  Eval semantics (the validation objective), no graph.
        ``t`` = (t1, t2) overrides the two host draws."""
        target = x_in["target"]
        self._need_cuda(target)
        ch0, ch1 = target[:, 0:1].contiguous(), target[:, 1:2].contiguous()
        t1, t2 = (None, None) if t is None else t
        # the joint sampler's noise_source, when set, serves both children for this call only: their own is put back
        kept = (self.indi1.noise_source, self.indi2.noise_source)
        try:
            if self.noise_source is not None:
                self.indi1.noise_source = self.indi2.noise_source = self.noise_source
            x_recon_ch1 = self.indi1.get_prediction_during_training({"target": ch0, "input": ch1}, noise=noise, t=t1)
            x_recon_ch2 = self.indi2.get_prediction_during_training({"target": ch1, "input": ch0}, noise=noise, t=t2)
        finally:
            self.indi1.noise_source, self.indi2.noise_source = kept
        loss_splitting = (self.indi1._loss(ch0, x_recon_ch1) + self.indi2._loss(ch1, x_recon_ch2)) / 2
        loss_input = 0.0
        self.current_log_dict["loss_splitting"] = loss_splitting.item()
        self.current_log_dict["alpha"] = self.get_alpha().item()
        self.current_log_dict["offset"] = self.get_offset().item()
        self.current_log_dict["scale"] = self.get_scale().item()
        return loss_splitting + self.w_input_loss * loss_input

    def set_loss(self, device):
        self.indi1.set_loss(device)
        self.indi2.set_loss(device)

    def set_new_noise_schedule(self, schedule_opt, device):
        self.indi1.set_new_noise_schedule(schedule_opt, device)
        self.indi2.set_new_noise_schedule(schedule_opt, device)

    @torch.no_grad()
    def second_ids(self, sample_ids):
        """The ids indi2 draws from: the caller's (below 2^39) with bit 39 set, so the two channels never share a draw."""
        return None if sample_ids is None else [v | self.STREAM2_BIT for v in
                                                engine._sample_ids(sample_ids, len(sample_ids), self.STREAM2_BIT).tolist()]

    @torch.no_grad()
    def inference(self, x_in, continuous=False, num_timesteps=None, t_float_start=0.5, eps=1e-8, seed=None,
                  sample_ids=None):
        """``seed`` / ``sample_ids`` (ids < 2^39): per-sample noise streams; indi1 draws from the ids, indi2 from the
        ids with bit 39 set.  ``noise_field`` here is a callable ``(shape, draw, id_bit)``: indi1 asks with
        ``id_bit = 0``, indi2 with ``STREAM2_BIT``, which the provider adds to its field ids -- the two channels never
        share a draw."""
        # the children build the Draws of their own calls; the field's refusals are made here, before they are set up
        Draws.refuse_field_with(self.noise_source, self.noise_field, sample_ids)
        field = self.noise_field
        for s, bit in ((self.indi1, 0), (self.indi2, self.STREAM2_BIT)):
            s.noise_source, s.use_graph = self.noise_source, self.use_graph   # indi1's draws first (Q4)
            s.noise_field = None if field is None else (lambda shape, draw, bit=bit: field(shape, draw, bit))
        if sample_ids is not None and torch.is_tensor(sample_ids):
            sample_ids = sample_ids.detach().cpu().tolist()
        k1 = dict(seed=seed, sample_ids=sample_ids)
        k2 = dict(seed=seed, sample_ids=self.second_ids(sample_ids))
        if self.noise_source is not None or not self.concurrent:
            # host draws are order-dependent: finish indi1's before indi2's start
            ch1 = self.indi1.inference(x_in, continuous, num_timesteps, t_float_start, eps, **k1)
            ch2 = self.indi2.inference(x_in, continuous, num_timesteps, 1 - t_float_start, eps, **k2)
        else:
            if self._streams is None:
                self._streams = (torch.cuda.Stream(), torch.cuda.Stream())
            s1, s2 = self._streams
            ch1 = self.indi1.inference(x_in, continuous, num_timesteps, t_float_start, eps, stream=s1, **k1)
            ch2 = self.indi2.inference(x_in, continuous, num_timesteps, 1 - t_float_start, eps, stream=s2, **k2)
            torch.cuda.current_stream().wait_stream(s1)
            torch.cuda.current_stream().wait_stream(s2)
        self.last_full_batch = torch.cat([self.indi1.last_full_batch, self.indi2.last_full_batch], dim=1)
        return torch.cat([ch1, ch2], dim=1)
