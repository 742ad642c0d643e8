"""Python host of the HIP sampling engine: owns ``dsx_model`` / ``dsx_exec``
handles, maps reference state-dict keys onto the library's parameter table and
builds the per-step scalar tables (bit-exact with the reference's schedules).

torch is used for device memory, streams and host-side schedule arithmetic
only; all sampling compute happens inside ``libdsx.so``.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import DsxError, check, lib


def _as_tuple(v):
    if v is None:
        return ()
    if isinstance(v, int):
        return (v,)
    return tuple(int(x) for x in v)


def make_cfg(flavour, in_channel, out_channel, inner_channel, norm_groups, channel_mults, attn_res,
             res_blocks, image_size, with_time_emb=True):
    """Keyword names of the reference ``UNet.__init__`` (sr3 unet.py:161-174)."""
    cfg = _lib.UnetCfg()
    cfg.flavour = _lib.FLAVOUR_SR3 if flavour == "sr3" else _lib.FLAVOUR_DDPM
    cfg.in_channel = int(in_channel)
    cfg.out_channel = int(out_channel if out_channel is not None else in_channel)
    cfg.inner_channel = int(inner_channel)
    cfg.norm_groups = int(norm_groups)
    mults = _as_tuple(channel_mults)
    attn = _as_tuple(attn_res)
    if len(mults) > 8 or len(attn) > 8:
        raise DsxError("at most 8 channel_mults / attn_res entries are supported")
    cfg.n_mults = len(mults)
    for i, m in enumerate(mults):
        cfg.channel_mults[i] = m
    cfg.n_attn_res = len(attn)
    for i, a in enumerate(attn):
        cfg.attn_res[i] = a
    cfg.res_blocks = int(res_blocks)
    cfg.image_size = int(image_size)
    cfg.with_time_emb = 1 if with_time_emb else 0
    return cfg


def dtype_code(dtype):
    """'f32' | 'bf16' | 'f16' (or the torch dtypes) -> DSX_DTYPE_*: the MFMA operand / activation storage type."""
    if dtype in ("bf16", torch.bfloat16):
        return _lib.DTYPE_BF16
    if dtype in ("f16", "fp16", torch.float16):
        return _lib.DTYPE_F16
    if dtype in ("f32", "fp32", torch.float32, None):
        return _lib.DTYPE_F32
    raise DsxError(f"unknown compute dtype {dtype!r} (f32, bf16, f16)")


def plan_dry_run(cfg, dtype, B, H, W, cond_channels=0):
    """Host-only planner check (no GPU): (sizing_bytes, planning_bytes, launches) of dsx_plan_dry_run."""
    a, b, n = C.c_size_t(), C.c_size_t(), C.c_int()
    check(lib.dsx_plan_dry_run(C.byref(cfg), dtype_code(dtype), int(B), int(H), int(W), int(cond_channels),
                               C.byref(a), C.byref(b), C.byref(n)))
    return int(a.value), int(b.value), int(n.value)


class UNetEngine:
    """One UNet on the current GPU: parameter table + executors per (B,H,W,cond)."""

    def __init__(self, cfg, flavour):
        self.flavour = flavour
        self.cfg = cfg
        h = C.c_void_p()
        check(lib.dsx_model_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._execs = {}
        self._finalized_dtype = None
        self.param_names, self.param_shapes = [], []
        name = C.create_string_buffer(256)
        nd = C.c_int()
        shp = (C.c_int64 * 4)()
        for i in range(lib.dsx_model_num_params(h)):
            check(lib.dsx_model_param_info(h, i, name, 256, C.byref(nd), shp))
            self.param_names.append(name.value.decode())
            self.param_shapes.append(tuple(int(shp[k]) for k in range(nd.value)))

    def __del__(self):
        try:
            for ex in self._execs.values():
                lib.dsx_exec_destroy(ex)
            if self._h:
                lib.dsx_model_destroy(self._h)
        except Exception:
            pass

    # ---- weights -----------------------------------------------------------
    def load_state_dict(self, sd, prefix=""):
        """``sd``: reference-keyed tensors (``prefix`` + UNet key).  Missing
        ``inv_freq`` is derived; anything else missing raises."""
        for i, (n, shp) in enumerate(zip(self.param_names, self.param_shapes)):
            key = prefix + n
            if key not in sd:
                if n.endswith("inv_freq"):
                    continue
                raise DsxError(f"state dict lacks {key}")
            t = sd[key].detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shp:
                if "noise_func" in n and len(shp) >= 1 and t.shape[0] == 2 * shp[0] and tuple(t.shape[1:]) == tuple(shp[1:]):
                    raise DsxError(f"{key}: {tuple(t.shape)} is a FeatureWiseAffine with use_affine_level=True "
                                   f"((1 + gamma) x + beta, sr3 unet.py:34-50); the engine implements the additive form "
                                   f"every reference config uses (use_affine_level=False), expected {shp}")
                raise DsxError(f"{key}: shape {tuple(t.shape)} != {shp}")
            check(lib.dsx_model_set_param(self._h, i, t, t.numel()))
        if self.flavour == "sr3" and self.cfg.with_time_emb:
            # PositionalEncoding's table, computed with the same torch ops as the
            # reference (sr3 unet.py:24-28) so the host constant is bit-identical
            count = self.cfg.inner_channel // 2
            step = torch.arange(count, dtype=torch.float32) / count
            freq = torch.exp(-math.log(1e4) * step).contiguous()
            check(lib.dsx_model_set_posenc_freq(self._h, freq, count))
        self._drop_execs()
        self._finalized_dtype = None

    def _drop_execs(self):
        for ex in self._execs.values():
            lib.dsx_exec_destroy(ex)
        self._execs = {}

    def finalize(self, dtype="f32"):
        _lib.require_gpu()
        code = dtype_code(dtype)
        if self._finalized_dtype != code:
            self._drop_execs()
            check(lib.dsx_model_finalize(self._h, code))
            self._finalized_dtype = code

    # ---- packed-weight cache (N4: the repack next to `*_gen.pth`, model/model.py:153-166) -------------------
    _PACK_MAGIC = b"DSXPACK3"

    def _pack_header(self, dtype_code_, key):
        import hashlib
        cfg_bytes = bytes(memoryview(self.cfg))                      # the UNet configuration (ctypes struct)
        h = hashlib.sha256(cfg_bytes + bytes([dtype_code_, lib.dsx_abi_version()]) + str(key).encode()).digest()
        return self._PACK_MAGIC + h

    def save_packed(self, path, key):
        """Write the device image of the finalized model (fragment-ordered weights etc.) to ``path``."""
        if self._finalized_dtype is None:
            raise DsxError("finalize() before save_packed()")
        n = C.c_size_t()
        check(lib.dsx_model_packed_bytes(self._h, self._finalized_dtype, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        check(lib.dsx_model_export_packed(self._h, buf, n.value))
        import hashlib
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(self._pack_header(self._finalized_dtype, key))
            f.write(hashlib.sha256(buf.data).digest())               # of the payload: a damaged file is refused
            buf.tofile(f)
        os.replace(tmp, path)

    def finalize_from_packed(self, path, dtype, key):
        """Finalize from a cached image if ``path`` holds one for this configuration, dtype, ABI and ``key`` (the
        checkpoint's hash); returns False (and does nothing) otherwise.  No parameter needs to be set."""
        _lib.require_gpu()
        code = dtype_code(dtype)
        if not os.path.exists(path):
            return False
        n = C.c_size_t()
        check(lib.dsx_model_packed_bytes(self._h, code, C.byref(n)))
        hdr = self._pack_header(code, key)
        import hashlib
        if os.path.getsize(path) != len(hdr) + 32 + n.value:
            return False
        with open(path, "rb") as f:
            if f.read(len(hdr)) != hdr:
                return False
            digest = f.read(32)
            buf = np.fromfile(f, dtype=np.uint8, count=n.value)
        if buf.size != n.value or hashlib.sha256(buf.data).digest() != digest:
            return False
        self._drop_execs()
        check(lib.dsx_model_finalize_packed(self._h, code, buf, n.value))
        self._finalized_dtype = code
        return True

    def flops(self, H, W):
        return float(lib.dsx_model_flops(self._h, int(H), int(W)))

    # ---- execution ---------------------------------------------------------
    def executor(self, B, H, W, cond_channels=0, slot=0):
        """One executor (plan + workspace) per geometry and ``slot``; concurrent loops on
        different streams must use different slots (an executor's calls are not concurrent)."""
        if self._finalized_dtype is None:
            raise DsxError("finalize() must precede execution")
        key = (int(B), int(H), int(W), int(cond_channels), int(slot))
        ex = self._execs.get(key)
        if ex is None:
            ex = C.c_void_p()
            check(lib.dsx_exec_create(self._h, key[0], key[1], key[2], key[3], C.byref(ex)))
            self._execs[key] = ex
        return ex

    def workspace_bytes(self, B, H, W, cond_channels=0):
        return int(lib.dsx_exec_workspace_bytes(self.executor(B, H, W, cond_channels)))

    def handoff_timeouts(self):
        """Sum over this network's executors of dsx_exec_handoff_timeouts: bounded spins of the conv kernel's
        loader -> compute hand-off that gave up.  0 in every correct run (synchronises the device)."""
        total = 0
        for ex in self._execs.values():
            n = C.c_uint(0)
            check(lib.dsx_exec_handoff_timeouts(ex, C.byref(n)))
            total += int(n.value)
        return total

    def num_launches(self, B, H, W, cond_channels=0):
        return int(lib.dsx_exec_num_launches(self.executor(B, H, W, cond_channels)))

    def op_descriptions(self, B, H, W, cond_channels=0):
        """Descriptions of the plan's launches in order (dsx_exec_op_info), e.g. 'conv3x3 64->64 @128x128 tile128x64 ws'."""
        ex = self.executor(B, H, W, cond_channels)
        desc = C.create_string_buffer(256)
        kind, fl, by = C.c_int(), C.c_double(), C.c_double()
        out = []
        for i in range(int(lib.dsx_exec_num_ops(ex))):
            check(lib.dsx_exec_op_info(ex, i, desc, 256, C.byref(kind), C.byref(fl), C.byref(by)))
            out.append(desc.value.decode())
        return out

    def layer_table(self, B, H, W, cond_channels=0):
        """The plan's layer table (dsx_exec_layer_info) with the recorded tensors copied out of the workspace: call it
        after a forward of this geometry.  One dict per layer: the dsx_layer_info fields, `desc` (the description of
        its conv / attention launch), the param names, and torch tensors in their storage dtype -- `x0`, `x1`
        (B, Hs, Ws, C), `gn_scale` / `gn_shift` (B, C0 + C1), `film` (B, Cout), `resid` (B, Ho, Wo, Cout), `out`
        (B, Ho, Wo, Cout); attention: `q`, `k`, `v`, `out` (B, L, C).  Absent entries are None."""
        ex = self.executor(B, H, W, cond_channels)
        descs = self.op_descriptions(B, H, W, cond_channels)
        dts = {_lib.DTYPE_F32: torch.float32, _lib.DTYPE_BF16: torch.bfloat16, _lib.DTYPE_F16: torch.float16}
        info = _lib.LayerInfo()

        def fetch(addr, shape, dtype, ld=None):
            """rows of `shape[-1]` elements at pitch `ld` (whole rows are copied, then sliced)"""
            if not addr:
                return None
            ld = ld or shape[-1]
            n = 1
            for s in shape[:-1]:
                n *= s
            t = torch.empty(n * ld, dtype=dtype, device="cuda")
            check(lib.dsx_exec_copy_workspace(ex, addr, (n * ld - ld + shape[-1]) * t.element_size(), t, None))
            return t.view(n, ld)[:, :shape[-1]].reshape(shape)

        out = []
        for i in range(int(lib.dsx_exec_num_layers(ex))):
            check(lib.dsx_exec_layer_info(ex, i, C.byref(info)))
            d = {name: getattr(info, name) for name, _ in _lib.LayerInfo._fields_}
            d["desc"] = descs[d["op_main"]] if d["op_main"] >= 0 else ""
            for key in ("w_param", "b_param", "gn_gamma_param", "gn_beta_param"):
                d[key.replace("param", "name")] = self.param_names[d[key]] if d[key] >= 0 else None
            sdt, odt, b = dts[d["src_dtype"]], dts[d["out_dtype"]], d["B"]
            kind = d["kind"]
            if kind == _lib.LAYER_CONV:
                d["x0"] = fetch(d["src0"], (b, d["Hs"], d["Ws"], d["C0"]), sdt)
                d["x1"] = fetch(d["src1"], (b, d["Hs"], d["Ws"], d["C1"]), sdt) if d["C1"] else None
                cin = d["C0"] + d["C1"]
                d["gn_scale"] = fetch(d["gn_scale"], (b, cin), torch.float32)
                d["gn_shift"] = fetch(d["gn_shift"], (b, cin), torch.float32)
                d["film"] = (fetch(d["film"], (b, d["film_bs"]), torch.float32)[:, d["film_off"]:d["film_off"] + d["Cout"]]
                             if d["film"] else None)
                d["resid"] = fetch(d["resid"], (b, d["Ho"], d["Wo"], d["Cout"]), sdt, d["resid_ld"])
                d["out"] = fetch(d["out"], (b, d["Ho"], d["Wo"], d["Cout"]), odt, d["out_ld"])
            elif kind == _lib.LAYER_ATTN:
                L, c = d["Ho"] * d["Wo"], d["C0"]
                d["q"] = fetch(d["src0"], (b, L, c), sdt, d["ld"])
                d["k"] = fetch(d["src1"], (b, L, c), sdt, d["ld"])
                d["v"] = fetch(d["resid"], (b, L, c), sdt, d["ld"])
                d["out"] = fetch(d["out"], (b, L, c), odt, d["out_ld"])
            elif kind == _lib.LAYER_FILM:
                d["out"] = fetch(d["out"], (b, d["Cout"]), torch.float32)
            else:
                d["out"] = fetch(d["out"], (b, d["Ho"], d["Wo"], d["Cout"]), odt)
            out.append(d)
        torch.cuda.current_stream().synchronize()
        return out

    def forward(self, x, time=None, cond_channels=0):
        """denoise_fn(x, t): x (B,Cin,H,W) fp32 cuda NCHW -> (B,Cout,H,W)."""
        x = x.contiguous()
        B, _, H, W = x.shape
        ex = self.executor(B, H, W, cond_channels)
        y = torch.empty((B, self.cfg.out_channel, H, W), dtype=torch.float32, device=x.device)
        t = None                                                     # with_time_emb == 0: no time input
        if self.cfg.with_time_emb:
            t = time.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
            if t.numel() not in (1, B):
                raise DsxError(f"time must have 1 or B={B} elements, got {t.numel()}")
        check(lib.dsx_unet_forward(ex, x, t, 0 if t is None else t.numel(), y, None))
        return y

    def sample_loop(self, table, x_init, cond=None, noise=None, seed=0, snapshot_steps=(),
                    use_graph=True, stream=None, slot=0, sample_ids=None):
        """Runs ``table`` (a ``StepTableHost``) from ``x_init`` (B,C,H,W) in place.
        Returns (final_state, snapshots) with snapshots (n_snap,B,C,H,W) or None.
        Asynchronous on the current (or given) stream.

        ``sample_ids`` (B integers): per-sample noise streams (``dsx_sample_loop_streams``): step ``s`` of sample ``b``
        draws ``randn_samples(.., seed, sample_ids, draw=s + 1)[b]`` whatever the batch it sits in; not together with
        ``noise``."""
        return self._loop(False, table, x_init, cond, noise, seed, snapshot_steps, use_graph, stream, slot, sample_ids)

    def solver_loop(self, table, x_init, cond=None, noise=None, seed=0, snapshot_steps=(), use_graph=True, stream=None,
                    sample_ids=None):
        """``sample_loop`` for the rows of a few-step solver (``table``: a ``model.solvers.SolverTableHost``;
        ``dsx_solver_loop``): the previous step's predicted x0 stays on the device between the replays of the captured
        step.  Arguments and return value as ``sample_loop``; ``noise`` is (K, B, C, H, W) for K rows."""
        return self._loop(True, table, x_init, cond, noise, seed, snapshot_steps, use_graph, stream, 0, sample_ids)

    def _loop(self, solver, table, x_init, cond, noise, seed, snapshot_steps, use_graph, stream, slot, sample_ids):
        x = x_init.contiguous()
        B, Cx, H, W = x.shape
        ids = None
        if sample_ids is not None:
            if noise is not None:
                raise DsxError("sample_ids together with injected noise: the draws come from one or the other")
            ids = _sample_ids(sample_ids, B)
        cc = 0 if cond is None else cond.shape[1]
        ex = self.executor(B, H, W, cc, slot)
        if cond is not None:
            cond = cond.to(dtype=torch.float32).contiguous()
        if noise is not None:
            noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
            if tuple(noise.shape) != (table.n_steps, B, Cx, H, W):
                raise DsxError(f"noise must be {(table.n_steps, B, Cx, H, W)}, got {tuple(noise.shape)}")
        snaps = None
        steps = np.asarray(sorted(int(s) for s in snapshot_steps), dtype=np.int32)
        if len(steps):
            snaps = torch.empty((len(steps), B, Cx, H, W), dtype=torch.float32, device=x.device)
        if stream is not None:
            # the loop runs asynchronously on `stream`: tell torch's caching allocator, or a
            # tensor dropped by the caller is recycled while the kernels still read it
            stream.wait_stream(torch.cuda.current_stream())
            for t in (x, cond, noise, snaps):
                if t is not None:
                    t.record_stream(stream)
        args = (ex, C.byref(table.c_struct()), cond, x, noise, _seed64(seed),
                steps.ctypes.data_as(C.POINTER(C.c_int32)) if len(steps) else None, len(steps), snaps,
                1 if use_graph else 0, stream)
        if solver:
            check(lib.dsx_solver_loop(*args, *_ids_arg(ids)))
        elif ids is None:
            check(lib.dsx_sample_loop(*args))
        else:
            check(lib.dsx_sample_loop_streams(*args, *_ids_arg(ids)))
        return x, snaps


class StepTableHost:
    """Host-side per-step scalars handed to ``dsx_sample_loop`` (include/dsx.h)."""

    def __init__(self, tcond, c1, c2, sigma, a=None, b=None, predict_eps=False, clip=False, per_sample=0):
        """Columns of shape (n_steps,), or (n_steps, B) with ``per_sample=B`` (one schedule per batch element)."""
        f = lambda v: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        self.tcond, self.a, self.b, self.c1, self.c2, self.sigma = f(tcond), f(a), f(b), f(c1), f(c2), f(sigma)
        self.n_steps = int(self.tcond.shape[0])
        self.per_sample = int(per_sample)
        if self.per_sample and tuple(self.tcond.shape) != (self.n_steps, self.per_sample):
            raise DsxError("per-sample step tables hold (n_steps, B) values per column")
        self.predict_eps, self.clip = bool(predict_eps), bool(clip)

    def c_struct(self):
        p = lambda v: v.ctypes.data_as(C.POINTER(C.c_float)) if v is not None else None
        return _lib.StepTable(self.n_steps, int(self.predict_eps), int(self.clip), p(self.tcond), p(self.a),
                              p(self.b), p(self.c1), p(self.c2), p(self.sigma), self.per_sample)


# ---------------------------------------------------------------------------
# schedules (host arithmetic, bit-exact with the reference)
# ---------------------------------------------------------------------------
def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """model/sr3_modules/diffusion.py:19-49 (float64 numpy)."""
    if schedule == "quad":
        betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    elif schedule == "linear":
        betas = np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    elif schedule in ("warmup10", "warmup50"):
        frac = 0.1 if schedule == "warmup10" else 0.5
        betas = linear_end * np.ones(n_timestep, dtype=np.float64)
        warm = int(n_timestep * frac)
        betas[:warm] = np.linspace(linear_start, linear_end, warm, dtype=np.float64)
    elif schedule == "const":
        betas = linear_end * np.ones(n_timestep, dtype=np.float64)
    elif schedule == "jsd":
        betas = 1.0 / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    elif schedule == "cosine":
        ts = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
        alphas = torch.cos(ts / (1 + cosine_s) * math.pi / 2).pow(2)
        alphas = alphas / alphas[0]
        betas = (1 - alphas[1:] / alphas[:-1]).clamp(max=0.999).numpy()
    else:
        raise NotImplementedError(schedule)
    return betas


def gaussian_buffers(schedule_opt):
    """The buffers ``set_new_noise_schedule`` registers (sr3 diffusion.py:92-139):
    dict of fp32 torch tensors + the float64 ``sqrt_alphas_cumprod_prev`` table."""
    betas = make_beta_schedule(schedule_opt["schedule"], schedule_opt["n_timestep"],
                               schedule_opt["linear_start"], schedule_opt["linear_end"])
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)
    pv = betas * (1.0 - ac_prev) / (1.0 - ac)
    bufs = {
        "betas": t32(betas),
        "alphas_cumprod": t32(ac),
        "alphas_cumprod_prev": t32(ac_prev),
        "sqrt_alphas_cumprod": t32(np.sqrt(ac)),
        "sqrt_one_minus_alphas_cumprod": t32(np.sqrt(1.0 - ac)),
        "log_one_minus_alphas_cumprod": t32(np.log(1.0 - ac)),
        "sqrt_recip_alphas_cumprod": t32(np.sqrt(1.0 / ac)),
        "sqrt_recipm1_alphas_cumprod": t32(np.sqrt(1.0 / ac - 1)),
        "posterior_variance": t32(pv),
        "posterior_log_variance_clipped": t32(np.log(np.maximum(pv, 1e-20))),
        "posterior_mean_coef1": t32(betas * np.sqrt(ac_prev) / (1.0 - ac)),
        "posterior_mean_coef2": t32((1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac)),
    }
    return bufs, np.sqrt(np.append(1.0, ac))


STEP_COLUMNS = ("tcond", "a", "b", "c1", "c2", "sigma")


def gaussian_step_columns(bufs, gamma_table_f64, kind):
    """The six step scalars of every timestep, indexed by t = 0 .. T-1 (fp32 numpy, ``STEP_COLUMNS``).

    ``kind`` "sr3": tcond = fp32(sqrt_alphas_cumprod_prev[t+1]) (sr3 diffusion.py:153-154);
    "ddpm": tcond = float(t) (ddpm diffusion.py:216-217).  sigma = exp(0.5*logvar)
    evaluated with torch fp32 like the reference (:175); sigma = 0 at t == 0
    (no noise at t == 0: :174 / ddpm :199-203)."""
    T = bufs["betas"].shape[0]
    t = np.arange(T)
    if kind == "sr3":
        tcond = torch.tensor(gamma_table_f64[t + 1], dtype=torch.float64).to(torch.float32).numpy()
    else:
        tcond = t.astype(np.float32)
    sigma = (0.5 * bufs["posterior_log_variance_clipped"]).exp().numpy().copy()
    sigma[0] = 0.0
    g = lambda k: bufs[k].numpy()
    return dict(tcond=tcond, a=g("sqrt_recip_alphas_cumprod"), b=g("sqrt_recipm1_alphas_cumprod"),
                c1=g("posterior_mean_coef1"), c2=g("posterior_mean_coef2"), sigma=sigma)


def gaussian_step_table(bufs, gamma_table_f64, kind, clip_denoised=True, start=None):
    """Rows of ``gaussian_step_columns`` in execution order i = T-1 .. 0 (sr3 diffusion.py:196-199), or, with
    ``start`` = t, the tail i = t-1 .. 0 of it: the loop of interpolate (ddpm diffusion.py:260-262)."""
    T = bufs["betas"].shape[0]
    start = T if start is None else int(start)
    if not 1 <= start <= T:
        raise DsxError(f"a step table starts at 1 <= t <= {T}, got {start}")
    cols = gaussian_step_columns(bufs, gamma_table_f64, kind)
    order = np.arange(start - 1, -1, -1)
    g = lambda k: cols[k][order]
    return StepTableHost(g("tcond"), c1=g("c1"), c2=g("c2"), sigma=g("sigma"), a=g("a"), b=g("b"),
                         predict_eps=True, clip=clip_denoised)


def gaussian_step_rows(bufs, gamma_table_f64, kind, t):
    """The rows of the Gaussian step table for integer ``t`` (a scalar or (B,) values): a dict of ``STEP_COLUMNS`` ->
    fp32 numpy arrays of ``t``'s shape, the very numbers ``gaussian_step_table`` holds at row T-1-t."""
    T = bufs["betas"].shape[0]
    t = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    if t.dtype.kind not in "iu":
        raise DsxError(f"timesteps are integers, got {t.dtype}")
    if t.size and (t.min() < 0 or t.max() >= T):
        raise DsxError(f"timesteps must lie in 0..{T - 1}")
    cols = gaussian_step_columns(bufs, gamma_table_f64, kind)
    return {k: cols[k][t] for k in STEP_COLUMNS}


def indi_step_row(delta, cur_t, e=0.01):
    """(tcond, c1, c2, sigma) of one InDI step (indi.py:65-68) as python floats holding fp32 values: the very torch
    expressions on a (1,) fp32 tensor, so scalar promotion and rounding (e.g. python_float / tensor == reciprocal *
    scalar) match."""
    t_cur = torch.Tensor([cur_t])
    r = delta / t_cur
    return t_cur.item(), r.item(), (1 - r).item(), (e * (t_cur - delta)).item()


def indi_step_table(num_timesteps, t_float_start, e=0.01):
    """The scalars of InDI.inference (indi.py:62-69,83-88): float64 ``cur_t -= delta``
    accumulation on the host, each op rounded to fp32 as torch does for
    python-scalar (op) fp32-tensor.  The drift assert of indi.py:64 is dropped (R3)."""
    delta = t_float_start / num_timesteps
    cur_t = t_float_start
    rows = []
    for _ in range(num_timesteps):
        rows.append(indi_step_row(delta, cur_t, e))
        cur_t -= delta
    ts, c1, c2, sg = zip(*rows)
    return StepTableHost(ts, c1=c1, c2=c2, sigma=sg, predict_eps=False, clip=False)


def indi_step_table_per_sample(num_timesteps, t_starts, e=0.01):
    """One InDI schedule per batch element (``t_starts``: B floats): the columns of ``indi_step_table`` for every
    sample, stacked to (n_steps, B).  This is what the reference's refinement driver gets by looping over the batch
    one sample at a time (core/psnr_based_t_refinement.py:22-36)."""
    tabs = [indi_step_table(num_timesteps, float(t), e) for t in t_starts]
    st = lambda k: np.stack([getattr(t, k) for t in tabs], axis=1)
    return StepTableHost(st("tcond"), c1=st("c1"), c2=st("c2"), sigma=st("sigma"), predict_eps=False, clip=False,
                         per_sample=len(tabs))


def indi_snapshot_steps(num_timesteps):
    """indi.py:77,89-90: idx % (1|(n//20)) == 0 or idx == n-1."""
    inter = 1 | (num_timesteps // 20)
    return [i for i in range(num_timesteps) if i % inter == 0 or i == num_timesteps - 1]


def gaussian_snapshot_steps(T):
    """sr3 diffusion.py:180,198: i % (1|(T//10)) == 0 on the descending index i;
    returned as 0-based step ordinals (step s handles i = T-1-s)."""
    inter = 1 | (T // 10)
    return [s for s in range(T) if (T - 1 - s) % inter == 0]


def randn(shape, seed, subsequence=0, device="cuda"):
    """N(0,1) from the engine's Philox stream (perf-mode initial states)."""
    _lib.require_gpu()
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib.dsx_randn(out, out.numel(), C.c_uint64(int(seed)), C.c_uint64(int(subsequence)), None))
    return out


def _sample_ids(sample_ids, B, limit=_lib.STREAM_ID_LIMIT):
    """``sample_ids`` as B uint64 values (numpy), refused by name when the count or a value does not fit."""
    if torch.is_tensor(sample_ids):
        sample_ids = sample_ids.detach().cpu().tolist()
    ids = [int(v) for v in sample_ids]
    if len(ids) != B:
        raise DsxError(f"sample_ids must hold B = {B} ids, got {len(ids)}")
    for v in ids:
        if not 0 <= v < limit:
            raise DsxError(f"sample id {v} out of range (0 <= id < 2^{limit.bit_length() - 1})")
    return np.asarray(ids, dtype=np.uint64)


def _ids_arg(ids):
    """The ``(pointer, count)`` pair the library takes for checked ids (``_sample_ids``); ``(None, 0)`` without ids."""
    return (None, 0) if ids is None else (ids.ctypes.data_as(_lib._pu64), len(ids))


def _draw_ordinal(draw):
    draw = int(draw)
    if not 0 <= draw < _lib.STREAM_DRAW_LIMIT:
        raise DsxError(f"draw ordinal {draw} out of range (0 <= draw < 2^24)")
    return draw


def _stream_draw(sample_ids, draw, B, other_noise):
    """The noise choice of a single step: ``(ids, draw ordinal)`` for per-sample streams, None without ``sample_ids``.
    ``other_noise``: the refusal when the call names another source of draws too, else None."""
    if sample_ids is None:
        if draw is not None:
            raise DsxError("draw names a draw of a sample stream: only with sample_ids")
        return None
    if other_noise:
        raise DsxError(other_noise)
    if draw is None:
        raise DsxError("sample_ids need the draw ordinal (draw = step + 1 inside a loop)")
    return _sample_ids(sample_ids, B), _draw_ordinal(draw)


def randn_samples(shape, seed, sample_ids, draw=0, device="cuda"):
    """Per-sample noise streams (``dsx_randn_samples``): a (B, ...) tensor whose row ``b`` is
    ``randn(shape[1:], seed, subsequence=(sample_ids[b] << 24) | draw)`` -- a function of (seed, id, draw, element) only,
    not of B or of the row's position.  Draw 0 is a loop's initial state, draw ``s + 1`` belongs to its step ``s``."""
    _lib.require_gpu()
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2 or min(shape) < 1:
        raise DsxError(f"randn_samples takes a (B, ...) shape of at least two non-empty dimensions, got {shape}")
    ids = _sample_ids(sample_ids, shape[0])
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib.dsx_randn_samples(out, shape[0], out.numel() // shape[0], _seed64(seed),
                                ids.ctypes.data_as(_lib._pu64), C.c_uint32(_draw_ordinal(draw)), None))
    return out


# ---------------------------------------------------------------------------
# the forward half of the training objective (dsx_q_sample / dsx_loss, include/dsx.h)
# ---------------------------------------------------------------------------
def _f32_cuda(t, what, shape=None):
    """A contiguous float32 CUDA tensor, or a refusal: the kernels read the caller's memory as it is, nothing is
    converted or copied behind the caller's back."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise DsxError(f"{what} must be a CUDA tensor: the objective runs on the MI355X only (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise DsxError(f"{what} must be a contiguous float32 tensor, got {t.dtype}"
                       f"{'' if t.is_contiguous() else ', strided'}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise DsxError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach()


def _bchw(t, what):
    """``t`` as a contiguous float32 CUDA tensor and its dimensions (B, C, H, W)."""
    t = _f32_cuda(t, what)
    if t.dim() != 4:
        raise DsxError(f"{what} must be (B, C, H, W), got {tuple(t.shape)}")
    return (t,) + tuple(t.shape)


def _coef(c, what, B, named=True):
    c = _f32_cuda(c, what).reshape(-1)
    if c.numel() != B:
        raise DsxError(f"{what if named else 'per-sample coefficients'} must hold B = {B} values, got {c.numel()}")
    return c


def _seed64(seed):
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def q_sample(x0, c0, c2, xe=None, c1=None, z=None, seed=0, subsequence=0, dst=None, coff=0, want_z=False):
    """``dsx_q_sample``: ``dst[:, coff:coff + C] = c0*x0 (+ c1*xe) + c2*z`` in one launch, every operation rounded on
    its own.  ``c0`` / ``c1`` / ``c2``: (B,) per-sample coefficients; ``xe`` (B, Ce, H, W) is read at channel
    ``c % Ce``; ``z`` None draws the Philox normals of ``randn(x0.shape, seed, subsequence)``.  Returns
    ``(dst, z)``: ``dst`` is a new (B, C, H, W) tensor unless given, ``z`` the normals used (the injected tensor, the
    drawn ones when ``want_z``, else None).  Every tensor must be contiguous float32 on the device."""
    x0, B, Cn, H, W = _bchw(x0, "x_start")
    Ce = 1
    if xe is not None:
        xe = _f32_cuda(xe, "x_end")
        if xe.dim() != 4 or xe.shape[0] != B or tuple(xe.shape[2:]) != (H, W):
            raise DsxError(f"x_end must be ({B}, Ce, {H}, {W}), got {tuple(xe.shape)}")
        Ce = xe.shape[1]
    c0, c1, c2 = (None if c is None else _coef(c, what, B, named=False)
                  for c, what in ((c0, "c0"), (c1 if xe is not None else None, "c1"), (c2, "c2")))
    z_out = None
    if z is not None:
        z = _f32_cuda(z, "noise", x0.shape)
    elif want_z:
        z_out = torch.empty_like(x0)
    if dst is None:
        dst, coff = torch.empty_like(x0), 0
    elif not (dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() and dst.dim() == 4
              and dst.shape[0] == B and tuple(dst.shape[2:]) == (H, W)):
        raise DsxError(f"dst must be a contiguous float32 CUDA tensor ({B}, Cdst, {H}, {W})")
    check(lib.dsx_q_sample(x0, xe, B, Cn, Ce, H, W, c0, c1, c2, z, _seed64(seed), C.c_uint64(int(subsequence)), z_out,
                           dst, dst.shape[1], int(coff), None))
    return dst, (z if z is not None else z_out)


def loss_per_sample(a, b, squared):
    """``dsx_loss``: per-sample sum |a - b| (L1) or sum (a - b)^2 (L2) over (C, H, W) of two (B, C, H, W) fp32 CUDA
    tensors, accumulated in double in a fixed order: a (B,) float64 CUDA tensor, bitwise repeatable."""
    a = _f32_cuda(a, "a")
    b = _f32_cuda(b, "b", a.shape)
    if a.dim() != 4:
        raise DsxError(f"the loss takes (B, C, H, W) tensors, got {tuple(a.shape)}")
    B, Cn, H, W = a.shape
    blocks = check(lib.dsx_loss_blocks(Cn, H, W))
    part = torch.empty(B * blocks, dtype=torch.float64, device=a.device)
    out = torch.empty(B, dtype=torch.float64, device=a.device)
    check(lib.dsx_loss(a, b, B, Cn, H, W, 1 if squared else 0, part, out, None))
    return out


# ---------------------------------------------------------------------------
# the fused attention kernel on caller tensors (dsx_attention, include/dsx.h)
# ---------------------------------------------------------------------------
_STORAGE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def attention(qkv, q_col, k_col, v_col, B, L, Cn, out, col_split=False):
    """``dsx_attention``: ``out[b*L + i, :Cn] = softmax_j(q_i . k_j / sqrt(Cn)) v_j`` per image, one launch of the
    UNet's fused kernel.  ``qkv``: a contiguous 2-D CUDA tensor of at least ``B*L`` token rows (fp32, bf16 or fp16)
    whose columns ``q_col`` / ``k_col`` / ``v_col`` .. ``+ Cn`` hold q, k and v; ``out``: a contiguous 2-D CUDA tensor
    of the same type with at least ``B*L`` rows of at least ``Cn`` columns, written in place (columns past ``Cn`` and
    rows past ``B*L`` are left untouched) and returned.  Nothing is converted or copied."""
    for t, what in ((qkv, "qkv"), (out, "out")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise DsxError(f"{what} must be a CUDA tensor: attention runs on the MI355X only (no CPU fallback)")
        if t.dim() != 2 or not t.is_contiguous():
            raise DsxError(f"{what} must be a contiguous 2-D tensor (token rows), got {tuple(t.shape)}")
    if qkv.dtype not in _STORAGE or out.dtype != qkv.dtype:
        raise DsxError(f"qkv and out must share one of float32 / bfloat16 / float16, got {qkv.dtype} and {out.dtype}")
    B, L, Cn = int(B), int(L), int(Cn)
    if B < 1 or L < 1 or qkv.shape[0] < B * L or out.shape[0] < B * L:
        raise DsxError(f"B * L = {B} * {L} token rows do not fit qkv ({qkv.shape[0]} rows) and out ({out.shape[0]})")
    check(lib.dsx_attention(qkv, qkv.shape[1], int(q_col), int(k_col), int(v_col), out, out.shape[1],
                            _STORAGE[qkv.dtype], B, L, Cn, 1 if col_split else 0, None))
    return out


# ---------------------------------------------------------------------------
# caller-driven reverse sampling (dsx_posterior_step / dsx_interp_start, include/dsx.h)
# ---------------------------------------------------------------------------
def posterior_step(x, net, c1, c2, sigma, a=None, b=None, predict_eps=False, clip=False, z=None, seed=0, subsequence=0,
                   repeat_noise=False, x_recon_out=None, mean_out=None, x_out=None, sample_ids=None, draw=None):
    """``dsx_posterior_step``: one reverse update with its intermediates in one launch.  ``a`` .. ``sigma``: (B,)
    per-sample coefficients; ``z`` (B, C, H, W) -- (1, C, H, W) under ``repeat_noise`` -- or None for the Philox normals
    of ``randn(x.shape, seed, subsequence)``.  Only the outputs given are written (``x_out`` may be ``x``); every
    tensor must be contiguous float32 on the device.  Returns ``(x_recon_out, mean_out, x_out)``.

    ``sample_ids`` (B integers) with ``draw``: the normals of ``randn_samples(x.shape, seed, sample_ids, draw)``
    (``dsx_posterior_step_streams``); not together with ``z`` or ``repeat_noise``."""
    x, B, Cn, H, W = _bchw(x, "x")
    net = _f32_cuda(net, "net", x.shape)
    c1, c2, sigma = _coef(c1, "c1", B), _coef(c2, "c2", B), _coef(sigma, "sigma", B)
    if predict_eps:
        if a is None or b is None:
            raise DsxError("predict_eps needs the columns a and b")
        a, b = _coef(a, "a", B), _coef(b, "b", B)
    else:
        a = b = None
    if z is not None:
        z = _f32_cuda(z, "noise", (1, Cn, H, W) if repeat_noise else x.shape)
    outs = [None if o is None else _f32_cuda(o, what, x.shape)
            for o, what in ((x_recon_out, "x_recon_out"), (mean_out, "mean_out"), (x_out, "x_out"))]
    streams = _stream_draw(sample_ids, draw, B, (z is not None or repeat_noise) and
                           "sample_ids together with injected noise or repeat_noise: a stream belongs to one sample")
    if streams:
        ids, d = streams
        check(lib.dsx_posterior_step_streams(x, net, B, Cn, H, W, a, b, c1, c2, sigma, 1 if predict_eps else 0,
                                             1 if clip else 0, None, _seed64(seed), C.c_uint64(d), 0,
                                             *outs, None, *_ids_arg(ids)))
        return tuple(outs)
    check(lib.dsx_posterior_step(x, net, B, Cn, H, W, a, b, c1, c2, sigma, 1 if predict_eps else 0, 1 if clip else 0, z,
                                 _seed64(seed), C.c_uint64(int(subsequence)), 1 if repeat_noise else 0, *outs, None))
    return tuple(outs)


def solver_step(x, net, a, b, cx, c0, sigma, cp=None, x0_prev=None, clip=False, z=None, seed=0, subsequence=0,
                x_recon_out=None, x_out=None, sample_ids=None, draw=None):
    """``dsx_solver_step``: one update of a few-step solver (``model/solvers.py``) in one launch,
    ``x0 = clamp?(a*x - b*net)``, ``x_out = c0*x0 + cx*x (+ cp*x0_prev) (+ sigma*z)``.  ``a`` .. ``sigma``: (B,)
    per-sample coefficients; ``x0_prev`` (the previous call's ``x_recon_out``) is read only for the samples whose ``cp``
    is not 0 and may be None when there is none (``cp`` then counts as 0).  Noise as in ``posterior_step``.  Both
    outputs are written (new tensors unless given; ``x_out`` may be ``x``, ``x_recon_out`` may be ``x0_prev``).
    Returns ``(x_recon_out, x_out)``."""
    x, B, Cn, H, W = _bchw(x, "x")
    net = _f32_cuda(net, "net", x.shape)
    a, b, cx, c0, sigma = (_coef(c, what, B) for c, what in ((a, "a"), (b, "b"), (cx, "cx"), (c0, "c0"), (sigma, "sigma")))
    if x0_prev is not None:
        if cp is None:
            raise DsxError("x0_prev needs the column cp")
        x0_prev, cp = _f32_cuda(x0_prev, "x0_prev", x.shape), _coef(cp, "cp", B)
    else:
        cp = None
    if z is not None:
        z = _f32_cuda(z, "noise", x.shape)
    x_recon_out = torch.empty_like(x) if x_recon_out is None else _f32_cuda(x_recon_out, "x_recon_out", x.shape)
    x_out = torch.empty_like(x) if x_out is None else _f32_cuda(x_out, "x_out", x.shape)
    ids, d = _stream_draw(sample_ids, draw, B, z is not None and
                          "sample_ids together with injected noise: the draws come from one or the other") or (None, 0)
    check(lib.dsx_solver_step(x, net, x0_prev, B, Cn, H, W, a, b, cx, c0, cp, sigma, 1 if clip else 0, z, _seed64(seed),
                              C.c_uint64(int(subsequence)), x_recon_out, x_out, None, *_ids_arg(ids), C.c_uint32(d)))
    return x_recon_out, x_out


def interp_start(x1, x2, a0, s0, lam, z1=None, z2=None, seed=0, subsequence=0, out=None):
    """``dsx_interp_start``: ``(1 - lam)*q_sample(x1) + lam*q_sample(x2)`` in one launch, ``a0`` / ``s0`` the (B,)
    coefficients of q_sample.  ``1 - lam`` is formed in double and each scalar rounded to fp32 once, as torch does for
    a python scalar against an fp32 tensor.  ``z1`` / ``z2``: both injected, or both None for the Philox normals of
    ``randn(shape, seed, subsequence)`` and ``randn(shape, seed, subsequence + 1)``."""
    x1, B, Cn, H, W = _bchw(x1, "x1")
    x2 = _f32_cuda(x2, "x2", x1.shape)
    a0, s0 = _coef(a0, "a0", B), _coef(s0, "s0", B)
    if (z1 is None) != (z2 is None):
        raise DsxError("both draws are injected, or neither")
    if z1 is not None:
        z1, z2 = _f32_cuda(z1, "z1", x1.shape), _f32_cuda(z2, "z2", x1.shape)
    out = torch.empty_like(x1) if out is None else _f32_cuda(out, "out", x1.shape)
    check(lib.dsx_interp_start(x1, x2, B, Cn, H, W, a0, s0, C.c_float(1 - float(lam)), C.c_float(float(lam)), z1, z2,
                               _seed64(seed), C.c_uint64(int(subsequence)), out, None))
    return out


# ---------------------------------------------------------------------------
# mean and spread over repeated samples (dsx_moments_update / dsx_moments_finish, include/dsx.h)
# ---------------------------------------------------------------------------
def _f64_cuda(t, what, numel):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != numel:
        raise DsxError(f"{what} must be a contiguous float64 CUDA tensor of {numel} elements")
    return t


def moments_update(x, mean=None, m2=None, r=0):
    """``dsx_moments_update``: sample ``r`` (0-based) of a series enters the running ``mean`` / ``m2`` (float64 CUDA
    tensors of ``x``'s shape; allocated when None, which ``r == 0`` alone allows: that sample overwrites them) by
    Welford's recurrence in double, one fused launch.  Returns ``(mean, m2)``."""
    x = _f32_cuda(x, "x")
    if x.numel() < 1:
        raise DsxError("moments_update: x is empty")
    if (mean is None) != (m2 is None):
        raise DsxError("moments_update: mean and m2 are given together, or neither")
    if mean is None:
        if int(r) != 0:
            raise DsxError(f"moments_update: sample r = {r} needs the running mean and m2 of the samples before it")
        mean = torch.empty(x.shape, dtype=torch.float64, device=x.device)
        m2 = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    _f64_cuda(mean, "mean", x.numel())
    _f64_cuda(m2, "m2", x.numel())
    check(lib.dsx_moments_update(x, mean, m2, x.numel(), int(r), None))
    return mean, m2


def moments_finish(mean, m2, n, want_std=True):
    """``dsx_moments_finish`` after ``n`` samples: ``(mean as float32, std as float32 or None)``, the unbiased spread
    ``sqrt(m2 / (n - 1))`` (0 for ``n == 1``), one launch."""
    if not torch.is_tensor(mean):
        raise DsxError("moments_finish: mean must be a float64 CUDA tensor")
    _f64_cuda(mean, "mean", mean.numel())
    _f64_cuda(m2, "m2", mean.numel())
    if mean.numel() < 1:
        raise DsxError("moments_finish: mean is empty")
    mean_out = torch.empty(mean.shape, dtype=torch.float32, device=mean.device)
    std_out = torch.empty(mean.shape, dtype=torch.float32, device=mean.device) if want_std else None
    check(lib.dsx_moments_finish(mean, m2, mean.numel(), int(n), mean_out, std_out, None))
    return mean_out, std_out


# ---------------------------------------------------------------------------
# quantiles and ranks across a stack of samples (dsx_sample_quantiles, include/dsx.h)
# ---------------------------------------------------------------------------
def sample_quantiles(stack, q, target=None):
    """``dsx_sample_quantiles``: ``stack`` is (n, ...) float32 on the device, n = 1..64 samples of one shape, each
    contiguous (the whole tensor, or a view such as ``buf[:, :b]`` whose first stride exceeds a sample's size); ``q``: 0
    to 8 values in [0, 1]; ``target`` (...): a contiguous float32 CUDA tensor of a sample's shape, or None.  Returns
    ``(quantiles (len(q), ...) or None without q, rank (...) or None without target)``: per element
    ``np.quantile(stack.astype(float64), q, axis=0).astype(float32)`` bit for bit, and the number of samples strictly
    below the target as float32.  One launch; the stack is read in place."""
    address, n, count, stride = _lib.stack_view(stack, "stack")
    shape = tuple(stack.shape[1:])
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(() if q is None else q, dtype=np.float64)))
    if qs.ndim != 1:
        raise DsxError(f"q must be a sequence of quantiles, got shape {qs.shape}")
    if target is not None:
        target = _f32_cuda(target, "target", shape)
        _lib.common_device("sample_quantiles", [stack.device, target.device])
    if not len(qs) and target is None:
        raise DsxError("sample_quantiles: nq = 0 and no rank output: give q, a target or both")
    out = torch.empty((len(qs),) + shape, dtype=torch.float32, device=stack.device) if len(qs) else None
    rank = torch.empty(shape, dtype=torch.float32, device=stack.device) if target is not None else None
    # the stack goes in by address (it may be a view); out or rank names the device and the stream of the call
    check(lib.dsx_sample_quantiles(address, stride, n, count, qs if len(qs) else None, len(qs), out, target, rank, None))
    return out, rank


# ---------------------------------------------------------------------------
# data consistency of a split: residual, report rows, projection (dsx_consistency, include/dsx.h)
# ---------------------------------------------------------------------------
PIX_OF_DTYPE = {torch.uint8: _lib.PIX_U8, torch.float32: _lib.PIX_F32}
PIX_OF_DTYPE.update({d: _lib.PIX_U16 for d in _lib.DEV_DTYPES["uint16_t"]})
PIX_BYTES = {_lib.PIX_U8: 1, _lib.PIX_U16: 2, _lib.PIX_F32: 4}
CONSISTENCY_SLOTS = 10


def consistency(acquisition, mean, scale, shift, weights, std=None, clip=-1.0, noise_var=0.0, want_row=True,
                want_map=False, want_mean=False, want_std=False, out_mean=None, out_std=None, pix=None):
    """``dsx_consistency``: ``acquisition`` holds the (frames, ...) pixels of ``mean``'s leading dimensions on the device
    as the file holds them: a uint8, uint16 (or int16 storage) or float32 tensor of that shape, or, with ``pix``
    (``_lib.PIX_*``) given, the same bytes under any dtype (``InputStackTiledPred`` keeps a uint16 stack as bytes);
    ``mean`` and ``std`` (frames, ..., C) float32, channel-last, normalised; ``scale``, ``shift``, ``weights``: C host
    numbers each (std_target, mean_target, w); ``clip`` < 0: none; ``noise_var`` = rho^2.  Returns
    ``(rows, map, mean', std')``: the (frames, 10) float64 report rows, the residual map (frames, ...), and the
    conditioned canvases; each None unless wanted.  ``out_mean`` / ``out_std`` name the tensors the conditioned
    canvases go to (``mean`` / ``std`` themselves: in place; no other overlap is allowed).  Everything stays on the
    device; two launches, nothing synchronised."""
    if not torch.is_tensor(acquisition) or not acquisition.is_cuda or not acquisition.is_contiguous():
        raise DsxError("consistency: the acquisition must be a contiguous CUDA tensor")
    if pix is None:
        if acquisition.dtype not in PIX_OF_DTYPE:
            raise DsxError(f"consistency: an acquisition of {acquisition.dtype}; uint8, uint16 or float32 pixels")
        pix = PIX_OF_DTYPE[acquisition.dtype]
    if pix not in PIX_BYTES:
        raise DsxError(f"consistency: pix = {pix!r}, must be PIX_U8, PIX_U16 or PIX_F32")
    mean = _f32_cuda(mean, "consistency: mean")
    if mean.dim() < 2 or mean.numel() < 1:
        raise DsxError(f"consistency: mean of shape {tuple(mean.shape)}, expected (frames, ..., C)")
    frames = int(mean.shape[0])
    plane = mean[0].numel() // int(mean.shape[-1])
    if acquisition.numel() * acquisition.element_size() != frames * plane * PIX_BYTES[pix]:
        raise DsxError(f"consistency: mean of shape {tuple(mean.shape)} for an acquisition of "
                       f"{acquisition.numel() * acquisition.element_size()} bytes; expected {frames} x {plane} pixels of "
                       f"{PIX_BYTES[pix]} bytes")
    nch = int(mean.shape[-1])
    if std is not None:
        std = _f32_cuda(std, "consistency: std", mean.shape)
    host = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (scale, shift, weights)]
    for v, name in zip(host, ("scale", "shift", "weights")):
        if v.size != nch:
            raise DsxError(f"consistency: {v.size} values of {name} for {nch} prediction channels")
    if (want_std or out_std is not None) and std is None:
        raise DsxError("consistency: a conditioned spread needs std")
    tensors = [acquisition, mean] + ([std] if std is not None else [])
    _lib.common_device("consistency", [t.device for t in tensors])
    _lib.require_gpu()
    dev = mean.device
    rows = part = fmap = None
    if want_row:
        blocks = check(lib.dsx_consistency_blocks(plane))
        part = torch.empty((frames, blocks, CONSISTENCY_SLOTS), dtype=torch.float64, device=dev)
        rows = torch.empty((frames, CONSISTENCY_SLOTS), dtype=torch.float64, device=dev)
    if want_map:
        fmap = torch.empty(mean.shape[:-1], dtype=torch.float32, device=dev)
    if out_mean is not None:
        out_mean = _f32_cuda(out_mean, "consistency: out_mean", mean.shape)
    elif want_mean:
        out_mean = torch.empty_like(mean)
    if out_std is not None:
        out_std = _f32_cuda(out_std, "consistency: out_std", mean.shape)
    elif want_std:
        out_std = torch.empty_like(mean)
    check(lib.dsx_consistency(acquisition, pix, mean, std, frames, plane, nch, host[0], host[1],
                              host[2], float(clip), float(noise_var), fmap, out_mean, out_std, rows, part, None))
    return rows, fmap, out_mean, out_std
