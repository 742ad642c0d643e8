"""Caller-driven reverse sampling, host side (no GPU): the reference-written fixtures (tools/gen_steps_golden.py) are
self-consistent bit for bit under the reference's fp32 torch expressions -- which pins the operation order
dsx_posterior_step / dsx_interp_start follow and the rounding of interpolate's python scalars --, the truncated step
table and the per-t rows equal the full table, and the samplers carry the reference's method signatures and refusals."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import cases
from tests.bits import same_bits
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED = cases.SCHEDULES["lin_8"]


def _t(g, key):
    return torch.from_numpy(g[key])


def _bufs():
    from diffsplitting_amd import engine
    return engine.gaussian_buffers(SCHED)


def _kernel_order(x, net, r, z, predict_eps=True, clip=False):
    """dsx_posterior_step's documented arithmetic in torch fp32, per-sample rows ``r``: (x_recon, mean, out)."""
    v = lambda k: torch.as_tensor(r[k], dtype=torch.float32).reshape(-1, 1, 1, 1)
    x0 = net
    if predict_eps:
        x0 = v("a") * x - v("b") * net
        if clip:
            x0 = x0.clamp(-1.0, 1.0)
    mean = v("c1") * x0 + v("c2") * x
    out = torch.where(v("sigma") != 0, mean + z * v("sigma"), mean)
    return x0, mean, out


# ----------------------------------------------------------------------------- ABI
def test_step_symbols_declared_bound_exported():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in ("dsx_posterior_step", "dsx_interp_start"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None


def test_entry_points_refuse_bad_arguments_with_a_status():
    """Argument checks come before any device work: they run without a GPU and nothing throws."""
    from diffsplitting_amd._lib import lib
    one = 16                                                   # a non-null address that is never dereferenced
    ok = (one, one, 1, 1, 2, 2, one, one, one, one, one, 1, 0, None, 0, 0, 0)
    assert lib.dsx_posterior_step(*ok, None, None, None, None) == -1
    assert b"output" in lib.dsx_last_error()
    assert lib.dsx_posterior_step(one, one, 0, 1, 2, 2, *ok[6:], one, None, None, None) == -1
    assert lib.dsx_posterior_step(one, one, 1, 1, 2, 2, None, None, one, one, one, 1, 0, None, 0, 0, 0, one, None, None,
                                  None) == -1                  # predict_eps without a / b
    assert lib.dsx_posterior_step(one, None, *ok[2:], one, None, None, None) == -1
    assert lib.dsx_interp_start(one, one, 1, 1, 2, 2, one, one, 0.5, 0.5, one, None, 0, 0, one, None) == -1
    assert lib.dsx_interp_start(one, one, 1, 1, 2, 2, one, one, 0.5, 0.5, None, None, 0, 0, None, None) == -1
    assert lib.dsx_interp_start(one, one, 1, 1, -2, 2, one, one, 0.5, 0.5, None, None, 0, 0, one, None) == -1


# ----------------------------------------------------------------------------- fixtures: self-consistency
@pytest.mark.parametrize("t", [7, 3, 0])
@pytest.mark.parametrize("clip", [1, 0])
def test_sr3_fixture_is_self_consistent(t, clip):
    from diffsplitting_amd import engine
    g = load_golden("steps_sr3")
    bufs, gamma = _bufs()
    x, net, z = _t(g, "x"), _t(g, f"net_t{t}"), _t(g, f"noise_t{t}")
    tag = f"_t{t}_clip{clip}"
    # the reference's expressions (sr3 diffusion.py:141-175)
    x_recon = bufs["sqrt_recip_alphas_cumprod"][t] * x - bufs["sqrt_recipm1_alphas_cumprod"][t] * net
    if clip:
        x_recon.clamp_(-1., 1.)
    mean = bufs["posterior_mean_coef1"][t] * x_recon + bufs["posterior_mean_coef2"][t] * x
    logvar = bufs["posterior_log_variance_clipped"][t]
    sample = mean + z * (0.5 * logvar).exp()
    assert same_bits(x_recon, _t(g, "x_recon" + tag))
    assert same_bits(mean, _t(g, "model_mean" + tag))
    assert same_bits(sample, _t(g, "sample" + tag))
    assert same_bits(logvar, _t(g, f"log_variance_t{t}"))
    # the same through the step-table row: what the kernel is handed
    r = engine.gaussian_step_rows(bufs, gamma, "sr3", np.full(2, t))
    k0, k1, k2 = _kernel_order(x, net, r, z, clip=bool(clip))
    assert same_bits(k0, x_recon) and same_bits(k1, mean)
    assert same_bits(k2, sample) if t > 0 else torch.equal(k2, sample)     # t == 0: the reference adds 0 * sigma
    assert np.array_equal(g[f"time_t{t}"], r["tcond"].reshape(2, 1))        # the UNet's time value
    if clip:
        assert bool((_t(g, f"x_recon_t{t}_clip0").abs() > 1).any())         # the clamp did something


@pytest.mark.parametrize("tag", ["mixed", "repeat"])
def test_ddpm_fixture_is_self_consistent(tag):
    from diffsplitting_amd import engine
    g = load_golden("steps_ddpm")
    bufs, gamma = _bufs()
    x, net, z, t = _t(g, "x"), _t(g, "net_" + tag), _t(g, "noise_" + tag), _t(g, "t_" + tag)
    ext = lambda k: bufs[k].gather(-1, t).reshape(-1, 1, 1, 1)
    x_recon = ext("sqrt_recip_alphas_cumprod") * x - ext("sqrt_recipm1_alphas_cumprod") * net
    x_recon.clamp_(-1., 1.)
    mean = ext("posterior_mean_coef1") * x_recon + ext("posterior_mean_coef2") * x
    logvar = ext("posterior_log_variance_clipped")
    noise = z.repeat(2, 1, 1, 1) if tag == "repeat" else z
    assert z.shape[0] == (1 if tag == "repeat" else 2)
    mask = (1 - (t == 0).float()).reshape(2, 1, 1, 1)
    sample = mean + mask * (0.5 * logvar).exp() * noise                      # ddpm diffusion.py:203
    assert same_bits(x_recon, _t(g, "x_recon_" + tag)) and same_bits(mean, _t(g, "model_mean_" + tag))
    assert same_bits(sample, _t(g, "sample_" + tag))
    assert same_bits(ext("posterior_variance"), _t(g, "variance_" + tag))
    assert same_bits(logvar, _t(g, "log_variance_" + tag))
    r = engine.gaussian_step_rows(bufs, gamma, "ddpm", t)
    k0, k1, k2 = _kernel_order(x, net, r, noise, clip=True)
    assert same_bits(k0, x_recon) and same_bits(k1, mean)
    nz = t != 0
    assert same_bits(k2[nz], sample[nz]) and torch.equal(k2, sample)
    assert np.array_equal(g["time_" + tag].astype(np.float32), r["tcond"])   # per-sample float(t)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_indi_fixture_is_self_consistent(tag):
    from diffsplitting_amd import engine
    g = load_golden("steps_indi")
    x, net, z = _t(g, "x"), _t(g, "net_" + tag), _t(g, "noise_" + tag)
    delta, t_cur, e = float(g["delta_" + tag]), float(g["t_cur_" + tag]), float(g["e"])
    t = torch.Tensor([t_cur])
    noise = z * (e * (t - delta))                                            # indi.py:67
    sample = delta / t * net + (1 - delta / t) * x + noise
    assert same_bits(sample, _t(g, "sample_" + tag))
    tc, c1, c2, sg = engine.indi_step_row(delta, t_cur, e)
    assert np.float32(tc) == g["time_" + tag][0]
    r = {k: np.full(2, v, dtype=np.float32) for k, v in (("c1", c1), ("c2", c2), ("sigma", sg))}
    out = _kernel_order(x, net, r, z, predict_eps=False)[2]
    if tag == "b":
        assert c2 == 0.0 and sg == 0.0                                       # delta == t_cur: x_t and the noise drop out
        assert torch.equal(out, sample)
    else:
        assert same_bits(out, sample)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_interpolate_fixture_pins_the_scalar_rounding(tag):
    """(1 - lam) * xt1 + lam * xt2 with python scalars: torch rounds each scalar to fp32 once, 1 - lam being formed in
    double -- the rule dsx_interp_start's c and d follow."""
    g = load_golden("interpolate_ddpm")
    bufs, _ = _bufs()
    lam, t = float(g["lam_" + tag]), int(g["t_" + tag])
    assert t == (5 if tag == "a" else SCHED["n_timestep"] - 1)
    tb = torch.full((2,), t, dtype=torch.long)
    ext = lambda k: bufs[k].gather(-1, tb).reshape(-1, 1, 1, 1)
    xt = []
    for i in (1, 2):
        q = ext("sqrt_alphas_cumprod") * _t(g, f"x{i}") + ext("sqrt_one_minus_alphas_cumprod") * _t(g, f"noise{i}_{tag}")
        assert same_bits(q, _t(g, f"xt{i}_{tag}"))
        xt.append(q)
    start = _t(g, "start_" + tag)
    assert same_bits((1 - lam) * xt[0] + lam * xt[1], start)
    c, d = torch.tensor(np.float32(1 - lam)), torch.tensor(np.float32(lam))
    assert same_bits(c * xt[0] + d * xt[1], start)
    assert g["step_noise_" + tag].shape == (t, 2, 2, 32, 32)


# ----------------------------------------------------------------------------- step tables
@pytest.mark.parametrize("kind", ["sr3", "ddpm"])
@pytest.mark.parametrize("start", [1, 5, 8])
def test_truncated_step_table_is_the_tail_of_the_full_one(kind, start):
    from diffsplitting_amd import engine
    bufs, gamma = _bufs()
    full = engine.gaussian_step_table(bufs, gamma, kind, True)
    part = engine.gaussian_step_table(bufs, gamma, kind, True, start=start)
    assert part.n_steps == start and part.predict_eps and part.clip and part.per_sample == 0
    for k in engine.STEP_COLUMNS:
        assert np.array_equal(getattr(part, k).view(np.int32), getattr(full, k)[-start:].view(np.int32)), k
    assert part.sigma[-1] == 0.0


def test_truncated_step_table_refuses_a_start_outside_the_schedule():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    bufs, gamma = _bufs()
    for start in (0, 9, -1):
        with pytest.raises(DsxError):
            engine.gaussian_step_table(bufs, gamma, "ddpm", True, start=start)


@pytest.mark.parametrize("kind", ["sr3", "ddpm"])
def test_step_rows_equal_the_full_table(kind):
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    bufs, gamma = _bufs()
    full = engine.gaussian_step_table(bufs, gamma, kind, True)
    T = full.n_steps
    t = torch.tensor([5, 0, 7, 7, 3])
    rows = engine.gaussian_step_rows(bufs, gamma, kind, t)
    for k in engine.STEP_COLUMNS:
        assert rows[k].dtype == np.float32 and rows[k].shape == (5,)
        assert np.array_equal(rows[k].view(np.int32), getattr(full, k)[T - 1 - t.numpy()].view(np.int32)), k
    one = engine.gaussian_step_rows(bufs, gamma, kind, 3)
    assert all(np.shape(one[k]) == () and one[k] == getattr(full, k)[T - 1 - 3] for k in engine.STEP_COLUMNS)
    for bad in (8, -1, torch.tensor([0, 8]), 1.5):
        with pytest.raises(DsxError):
            engine.gaussian_step_rows(bufs, gamma, kind, bad)


def test_indi_step_row_is_a_row_of_the_table():
    from diffsplitting_amd import engine
    tab = engine.indi_step_table(4, 0.6)
    delta, cur = 0.6 / 4, 0.6
    for s in range(4):
        row = engine.indi_step_row(delta, cur, 0.01)
        assert [np.float32(v) for v in row] == [tab.tcond[s], tab.c1[s], tab.c2[s], tab.sigma[s]]
        cur -= delta


# ----------------------------------------------------------------------------- samplers: signatures and refusals
def _sr3():
    from diffsplitting_amd.model.samplers import GaussianSampler
    s = GaussianSampler(None, 32, channels=3, conditional=True)
    s.set_new_noise_schedule(SCHED, "cpu")
    return s


def _ddpm(conditional=False):
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    s = GaussianSamplerDdpm(None, 32, channels=2, conditional=conditional)
    s.set_new_noise_schedule(SCHED, "cpu")
    return s


def _indi():
    from diffsplitting_amd.model.samplers import InDISampler
    s = InDISampler(None, 32, channels=2, out_channel=2, conditional=False, val_schedule_opt={"n_timestep": 4})
    s.set_new_noise_schedule({"n_timestep": 4}, "cpu")
    return s


SIGNATURES = {
    "sr3": {"predict_start_from_noise": ["x_t", "t", "noise"], "q_posterior": ["x_start", "x_t", "t"],
            "p_mean_variance": ["x", "t", "clip_denoised", "condition_x"],
            "p_sample": ["x", "t", "clip_denoised", "condition_x"]},
    "ddpm": {"predict_start_from_noise": ["x_t", "t", "noise"], "q_posterior": ["x_start", "x_t", "t"],
             "p_mean_variance": ["x", "t", "clip_denoised", "condition_x"],
             "p_sample": ["x", "t", "clip_denoised", "repeat_noise", "condition_x"],
             "interpolate": ["x1", "x2", "t", "lam"]},
    "indi": {"inference_one_step": ["x_t", "delta_t", "t_cur"], "q_mean_variance": ["x_start", "t"],
             "predict_start_from_noise": ["x_t", "t", "noise"], "q_posterior": ["x_start", "x_t", "t"],
             "p_mean_variance": ["x", "t", "clip_denoised", "condition_x"], "interpolate": ["x1", "x2", "t", "lam"]},
}
DEFAULTS = {("sr3", "p_sample"): {"clip_denoised": True, "condition_x": None},
            ("sr3", "p_mean_variance"): {"condition_x": None},
            ("ddpm", "p_sample"): {"clip_denoised": True, "repeat_noise": False, "condition_x": None},
            ("ddpm", "p_mean_variance"): {"condition_x": None},
            ("ddpm", "interpolate"): {"t": None, "lam": 0.5},
            ("indi", "p_mean_variance"): {"condition_x": None},
            ("indi", "interpolate"): {"t": None, "lam": 0.5}}


@pytest.mark.parametrize("family", ["sr3", "ddpm", "indi"])
def test_methods_carry_the_reference_signatures(family):
    smp = {"sr3": _sr3, "ddpm": _ddpm, "indi": _indi}[family]()
    for name, params in SIGNATURES[family].items():
        sig = inspect.signature(getattr(smp, name))
        assert list(sig.parameters) == params, (family, name)
        want = DEFAULTS.get((family, name), {})
        got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
        assert got == want, (family, name)


def test_cpu_tensors_are_refused():
    from diffsplitting_amd._lib import DsxError
    x = torch.zeros(2, 3, 8, 8)
    s = _sr3()
    for call in (lambda: s.p_sample(x, 3, condition_x=x), lambda: s.p_sample(x, 0), lambda: s.p_mean_variance(x, 3, True),
                 lambda: s.predict_start_from_noise(x, 3, x), lambda: s.q_posterior(x, x, 3)):
        with pytest.raises(DsxError):
            call()
    d, x2, t = _ddpm(), torch.zeros(2, 2, 8, 8), torch.tensor([5, 0])
    for call in (lambda: d.p_sample(x2, t), lambda: d.p_sample(x2, t, repeat_noise=True),
                 lambda: d.p_mean_variance(x2, t, True), lambda: d.interpolate(x2, x2, t=5, lam=0.3)):
        with pytest.raises(DsxError):
            call()
    with pytest.raises(DsxError):
        _indi().inference_one_step(x2, 0.25, 1.0)


def test_a_conditional_sampler_refuses_interpolate_by_name():
    from diffsplitting_amd._lib import DsxError
    x = torch.zeros(2, 2, 8, 8)
    with pytest.raises(DsxError, match="interpolate"):
        _ddpm(conditional=True).interpolate(x, x)


def test_indi_refusals():
    s = _indi()
    x = torch.zeros(2, 2, 8, 8)
    for call in (lambda: s.q_mean_variance(x, 1), lambda: s.predict_start_from_noise(x, 1, x),
                 lambda: s.q_posterior(x, x, 1), lambda: s.p_mean_variance(x, 1, True), lambda: s.interpolate(x, x)):
        with pytest.raises(NotImplementedError, match="This is not needed."):
            call()
    with pytest.raises(AssertionError, match="delta_t should be less than or equal to t_cur"):
        s.inference_one_step(x, 0.5, 0.25)
    s._noise_mode = "brownian"
    with pytest.raises(NotImplementedError, match="brownian"):
        s.inference_one_step(x, 0.25, 1.0)
