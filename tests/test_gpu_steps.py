"""Caller-driven reverse sampling on the MI355X (`-m gpu`, fp32 build): dsx_posterior_step and dsx_interp_start bit-exact
against the torch fp32 expression, their Philox paths against dsx_randn, and p_mean_variance / p_sample /
inference_one_step / interpolate of the samplers against the fixtures the reference wrote
(tools/gen_steps_golden.py) and, chained, against the reference's own loops (oracle/gen_golden.py)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import cases
from tests import nets
from tests.bits import same_bits
from tests.gpu_util import maxabs
from tests.steps_util import Source, constant_unet, off
from tests.steps_util import ref_step as _ref_step
from tests.util import golden_state_dict, load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FP32_TOL = 1e-3          # the project's per-pixel fp32 bound on a UNet output (tests/test_gpu_parity.py)
SCHED = cases.SCHEDULES["lin_8"]
SENTINEL = -7.25


def _t(g, key):
    return torch.from_numpy(g[key])


# per-sample coefficients, all different; sample 1 has sigma = 0
COEF = dict(a=torch.tensor([1.0371, 2.2360679, 1.0000501]), b=torch.tensor([0.2748, 2.0, 0.0100123]),
            c1=torch.tensor([0.75623951, 0.31, 0.9990234]), c2=torch.tensor([0.1, 0.654321, 0.0123]),
            sigma=torch.tensor([0.37, 0.0, 0.81]))


def _call(x, net, co, put=lambda t: t.cuda(), **kw):
    from diffsplitting_amd import engine
    dev = {k: v.cuda() for k, v in co.items()}
    return engine.posterior_step(put(x) if not x.is_cuda else x, put(net), dev["c1"], dev["c2"], dev["sigma"],
                                 a=dev["a"], b=dev["b"], **kw)


# ----------------------------------------------------------------------------- dsx_posterior_step, injected z
@pytest.mark.parametrize("shape", [
    (2, 3, 8, 8),        # 16-byte path
    (3, 3, 5, 7),        # H*W = 35: scalar path, groups of four straddle rows and samples
    (1, 1, 1, 1),        # less than one group
    (3, 2, 64, 68),      # 16-byte path, more than one workgroup
    (3, 2, 33, 67),      # scalar path, more than one workgroup
])
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("predict_eps", [0, 1])
def test_posterior_step_bit_exact(shape, clip, predict_eps):
    """Every combination of NULL outputs; outputs not asked for keep their sentinel (they are not even passed)."""
    B = shape[0]
    co = {k: v[:B] for k, v in COEF.items()}
    x, net, z = nets.rand(shape, 1), 0.7 * nets.rand(shape, 2), nets.rand(shape, 3)
    ref = _ref_step(x, net, co, z, predict_eps, clip)
    if predict_eps and clip:
        assert bool((ref[0].abs() == 1).any()) or shape == (1, 1, 1, 1)       # the clamp is exercised
    for want in itertools.product((0, 1), repeat=3):
        if not any(want):
            continue
        bufs = [torch.full(shape, SENTINEL, device="cuda") for _ in range(3)]
        _call(x, net, co, predict_eps=predict_eps, clip=clip, z=z.cuda(),
              x_recon_out=bufs[0] if want[0] else None, mean_out=bufs[1] if want[1] else None,
              x_out=bufs[2] if want[2] else None)
        for w, got, r in zip(want, bufs, ref):
            assert same_bits(got, r) if w else bool((got == SENTINEL).all()), (want, w)


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 3, 5, 7)])
def test_posterior_step_in_place_and_unaligned(shape):
    B = shape[0]
    co = {k: v[:B] for k, v in COEF.items()}
    x, net, z = nets.rand(shape, 4), nets.rand(shape, 5), nets.rand(shape, 6)
    ref = _ref_step(x, net, co, z, 1, 1)
    # x_out aliasing x
    xg = x.cuda()
    recon = torch.empty_like(xg)
    out = _call(xg, net, co, predict_eps=1, clip=1, z=z.cuda(), x_recon_out=recon, x_out=xg)
    assert out[2].data_ptr() == xg.data_ptr() and same_bits(xg, ref[2]) and same_bits(recon, ref[0])
    # base pointers 4 bytes past a 16-byte boundary: the scalar path whatever H*W is
    n = x.numel()
    outs = [torch.full((n + 1,), SENTINEL, device="cuda")[1:].view(shape) for _ in range(3)]
    _call(x, net, co, put=off, predict_eps=1, clip=1, z=off(z), x_recon_out=outs[0], mean_out=outs[1], x_out=outs[2])
    assert all(same_bits(o, r) for o, r in zip(outs, ref))
    # only one operand misaligned
    got = _call(x, net, co, predict_eps=1, clip=1, z=off(z), x_out=torch.empty(shape, device="cuda"))[2]
    assert same_bits(got, ref[2])


@pytest.mark.parametrize("shape", [(3, 3, 8, 8), (3, 3, 5, 7)])
def test_posterior_step_repeat_noise_injected(shape):
    """An injected z of shape (1, C, H, W) serves every sample (noise_like(..., repeat=True))."""
    x, net, z = nets.rand(shape, 7), nets.rand(shape, 8), nets.rand((1,) + shape[1:], 9)
    ref = _ref_step(x, net, COEF, z, 1, 0, repeat=True)
    got = _call(x, net, COEF, predict_eps=1, clip=0, z=z.cuda(), repeat_noise=True, x_out=torch.empty(shape, device="cuda"))[2]
    assert same_bits(got, ref[2])


def test_posterior_step_refusals():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    shape = (2, 3, 8, 8)
    x = nets.rand(shape, 1).cuda()
    c = torch.ones(2, device="cuda")
    with pytest.raises(DsxError, match="output"):
        engine.posterior_step(x, x, c, c, c)
    with pytest.raises(DsxError):
        engine.posterior_step(x, x, c, c, c, predict_eps=True, x_out=torch.empty_like(x))      # no a / b
    with pytest.raises(DsxError):
        engine.posterior_step(x, x, c, c, torch.ones(3, device="cuda"), x_out=torch.empty_like(x))
    with pytest.raises(DsxError):
        engine.posterior_step(x, x, c, c, c, z=x, repeat_noise=True, x_out=torch.empty_like(x))  # z must be (1, C, H, W)
    with pytest.raises(DsxError):
        engine.posterior_step(x.cpu(), x, c, c, c, x_out=torch.empty_like(x))


# ----------------------------------------------------------------------------- dsx_posterior_step, Philox z
@pytest.mark.parametrize("shape", [(3, 3, 8, 8), (3, 3, 5, 7), (3, 1, 64, 67)])
def test_posterior_step_philox_path(shape):
    """sigma = 1 and c1 = c2 = 0 make x_out the draw itself (0 + z * 1), so it is compared with dsx_randn directly and
    never recovered by a division.  Sample 1 has sigma = 0: it gets its mean, here 0."""
    from diffsplitting_amd import engine
    B = shape[0]
    x, net = nets.rand(shape, 10), nets.rand(shape, 11)
    zero = torch.zeros(B)
    co = dict(a=zero, b=zero, c1=zero, c2=zero, sigma=torch.tensor([1.0, 0.0, 1.0]))
    run = lambda **kw: _call(x, net, co, predict_eps=0, x_out=torch.empty(shape, device="cuda"), **kw)[2]
    out = run(seed=1234, subsequence=5)
    z = engine.randn(shape, 1234, 5)
    assert same_bits(out[0], z[0]) and same_bits(out[2], z[2])
    assert bool((out[1] == 0).all())
    assert same_bits(run(seed=1234, subsequence=5), out)                       # same seed: bitwise equal
    assert not same_bits(run(seed=1235, subsequence=5), out)
    assert not same_bits(run(seed=1234, subsequence=6), out)
    rep = run(seed=1234, subsequence=5, repeat_noise=True)
    first = engine.randn((1,) + shape[1:], 1234, 5)[0]                          # sample 0's draw
    assert same_bits(rep[0], first) and same_bits(rep[2], first) and same_bits(rep[0], out[0])
    assert bool((rep[1] == 0).all())
    # with real coefficients the Philox result equals the injected one
    got = _call(x, net, COEF, predict_eps=1, clip=1, seed=77, subsequence=3, x_out=torch.empty(shape, device="cuda"))[2]
    inj = _call(x, net, COEF, predict_eps=1, clip=1, z=engine.randn(shape, 77, 3), x_out=torch.empty(shape, device="cuda"))[2]
    assert same_bits(got, inj)


# ----------------------------------------------------------------------------- dsx_interp_start
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("unaligned", [False, True])
def test_interp_start_matches_the_fixture(tag, unaligned):
    """Bitwise the reference's two q_sample results and their lerp, on the 16-byte path and (base pointers offset by
    4 bytes) on the scalar path."""
    from diffsplitting_amd import engine
    g = load_golden("interpolate_ddpm")
    bufs, _ = engine.gaussian_buffers(SCHED)
    t, lam = int(g["t_" + tag]), float(g["lam_" + tag])
    tb = torch.full((2,), t, dtype=torch.long)
    a0, s0 = bufs["sqrt_alphas_cumprod"].gather(-1, tb).cuda(), bufs["sqrt_one_minus_alphas_cumprod"].gather(-1, tb).cuda()
    put = off if unaligned else (lambda v: v.cuda())
    x1, x2, z1, z2 = (put(_t(g, k)) for k in ("x1", "x2", "noise1_" + tag, "noise2_" + tag))
    for x, z, want in ((x1, z1, "xt1_"), (x2, z2, "xt2_")):
        assert same_bits(engine.q_sample(x, a0, s0, z=z)[0], _t(g, want + tag))
    out = engine.interp_start(x1, x2, a0, s0, lam, z1=z1, z2=z2)
    assert same_bits(out, _t(g, "start_" + tag))
    # lam = 0 and 1 give the two q_sample results themselves (1 * q + 0 * q')
    assert torch.equal(engine.interp_start(x1, x2, a0, s0, 0.0, z1=z1, z2=z2).cpu(), _t(g, "xt1_" + tag))
    assert torch.equal(engine.interp_start(x1, x2, a0, s0, 1.0, z1=z1, z2=z2).cpu(), _t(g, "xt2_" + tag))


@pytest.mark.parametrize("shape", [(2, 2, 8, 8), (3, 2, 5, 7)])
def test_interp_start_philox_subsequences(shape):
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    B = shape[0]
    x1, x2 = nets.rand(shape, 12).cuda(), nets.rand(shape, 13).cuda()
    a0, s0 = COEF["c1"][:B].cuda(), COEF["c2"][:B].cuda()
    out = engine.interp_start(x1, x2, a0, s0, 0.3, seed=99, subsequence=4)
    inj = engine.interp_start(x1, x2, a0, s0, 0.3, z1=engine.randn(shape, 99, 4), z2=engine.randn(shape, 99, 5))
    assert same_bits(out, inj)
    assert not same_bits(engine.interp_start(x1, x2, a0, s0, 0.3, seed=99, subsequence=5), out)
    with pytest.raises(DsxError):
        engine.interp_start(x1, x2, a0, s0, 0.3, z1=x1)


# ----------------------------------------------------------------------------- through the UNet, against the fixtures
def _sr3(fixture):
    from diffsplitting_amd.model.samplers import GaussianSampler
    sd, g = golden_state_dict(fixture)
    net = nets.unet("sr3", cases.UNET_CASES["sr3_tiny"]["cfg"])
    smp = GaussianSampler(net, 32, channels=3, conditional=True).cuda()
    smp.set_new_noise_schedule(SCHED, "cuda")
    nets.load(smp, sd)
    return smp, net, g


def _ddpm(fixture, cfg, channels, conditional):
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    sd, g = golden_state_dict(fixture)
    net = nets.unet("ddpm", cfg)
    smp = GaussianSamplerDdpm(net, 32, channels=channels, conditional=conditional).cuda()
    smp.set_new_noise_schedule(SCHED, "cuda")
    nets.load(smp, sd)
    return smp, net, g


def _indi(fixture, n):
    from diffsplitting_amd.model.samplers import InDISampler
    sd, g = golden_state_dict(fixture)
    net = nets.unet("ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"])
    smp = InDISampler(net, 32, channels=2, out_channel=2, conditional=False, val_schedule_opt={"n_timestep": n}).cuda()
    smp.set_new_noise_schedule({"n_timestep": n}, "cuda")
    nets.load(smp, sd)
    return smp, net, g


def _within(name, got, ref, tol=FP32_TOL):
    err = maxabs(got.cpu(), ref)
    print(f"\n{name}: max|hip - reference| = {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, (name, err)


def test_sr3_steps_match_the_reference():
    smp, net, g = _sr3("steps_sr3")
    rec = {}
    net.register_forward_hook(lambda m, inp, out: rec.update(net=out))
    x, cond = _t(g, "x").cuda(), _t(g, "condition").cuda()
    for t in (7, 3, 0):
        for clip in (1, 0):
            tag = f"_t{t}_clip{clip}"
            mean, logvar = smp.p_mean_variance(x, t, bool(clip), condition_x=cond)
            _within("sr3 model_mean" + tag, mean, g["model_mean" + tag])
            assert logvar.shape == () and same_bits(logvar, smp.posterior_log_variance_clipped[t])
            assert same_bits(logvar, _t(g, f"log_variance_t{t}"))
            src = smp.noise_source = Source([_t(g, f"noise_t{t}")])
            _within("sr3 p_sample" + tag, smp.p_sample(x, t, clip_denoised=bool(clip), condition_x=cond), g["sample" + tag])
            assert src.shapes == ([tuple(x.shape)] if t > 0 else [])          # one draw per call, none at t == 0
            smp.noise_source = None
        _within(f"sr3 UNet output t{t}", rec["net"], g[f"net_t{t}"])
        scale = max(1.0, float(smp.sqrt_recipm1_alphas_cumprod[t]))            # x_recon = a x - b net: b times the net's error
        _within(f"sr3 x_recon t{t}", smp.predict_start_from_noise(x, t, rec["net"]), g[f"x_recon_t{t}_clip0"], FP32_TOL * scale)
        # on the fixture's own UNet output the two kernels' expressions are the reference's bit for bit
        assert same_bits(smp.predict_start_from_noise(x, t, _t(g, f"net_t{t}").cuda()), _t(g, f"x_recon_t{t}_clip0"))
        for clip in (1, 0):
            m, lv = smp.q_posterior(_t(g, f"x_recon_t{t}_clip{clip}").cuda(), x, t)
            assert same_bits(m, _t(g, f"model_mean_t{t}_clip{clip}")) and same_bits(lv, logvar)
    # device noise: repeatable under torch's seed, another seed gives another sample
    outs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        outs.append(smp.p_sample(x, 7, condition_x=cond))
    assert same_bits(outs[0], outs[1]) and not same_bits(outs[0], outs[2])


@pytest.mark.parametrize("tag", ["mixed", "repeat"])
def test_ddpm_steps_match_the_reference(tag):
    smp, net, g = _ddpm("steps_ddpm", cases.DDPM_COND_CASE["cfg"], 1, True)
    x, cond, t = _t(g, "x").cuda(), _t(g, "condition").cuda(), _t(g, "t_" + tag).cuda()
    repeat = tag == "repeat"
    mean, var, logvar = smp.p_mean_variance(x, t, True, condition_x=cond)
    _within(f"ddpm {tag} model_mean", mean, g["model_mean_" + tag])
    assert var.shape == logvar.shape == (2, 1, 1, 1)
    assert same_bits(var, _t(g, "variance_" + tag)) and same_bits(logvar, _t(g, "log_variance_" + tag))
    assert same_bits(var.reshape(-1), smp.posterior_variance[t])
    assert same_bits(logvar.reshape(-1), smp.posterior_log_variance_clipped[t])
    src = smp.noise_source = Source([_t(g, "noise_" + tag)])
    out = smp.p_sample(x, t, clip_denoised=True, repeat_noise=repeat, condition_x=cond)
    _within(f"ddpm {tag} p_sample", out, g["sample_" + tag])
    assert src.shapes == [(1, 1, 32, 32) if repeat else (2, 1, 32, 32)]
    if not repeat:                                                             # the sample at t == 0 is its model_mean
        assert int(t[1]) == 0 and same_bits(out[1], mean[1])
    # drawn on every call, t == 0 included
    src = smp.noise_source = Source()
    smp.p_sample(x, torch.zeros(2, dtype=torch.long, device="cuda"), condition_x=cond)
    assert src.shapes == [(2, 1, 32, 32)]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_indi_one_step_matches_the_reference(tag):
    smp, net, g = _indi("steps_indi", 4)
    x = _t(g, "x").cuda()
    src = smp.noise_source = Source([_t(g, "noise_" + tag)])
    out = smp.inference_one_step(x, float(g["delta_" + tag]), float(g["t_cur_" + tag]))
    _within(f"indi one step {tag}", out, g["sample_" + tag])
    assert src.shapes == [tuple(x.shape)]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_interpolate_matches_the_reference(tag):
    smp, net, g = _ddpm("interpolate_ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"], 2, False)
    t, lam = int(g["t_" + tag]), float(g["lam_" + tag])
    draws = [_t(g, "noise1_" + tag), _t(g, "noise2_" + tag)] + list(_t(g, "step_noise_" + tag))
    src = smp.noise_source = Source(draws)
    x1, x2 = _t(g, "x1").cuda(), _t(g, "x2").cuda()
    out = smp.interpolate(x1, x2, t=None if tag == "b" else t, lam=lam)
    assert out.shape == x1.shape                                               # the whole batch
    _within(f"interpolate {tag}", out, g["result_" + tag])
    assert src.shapes == [tuple(x1.shape)] * (2 + t) and not src.draws
    # device noise: repeatable under torch's seed
    smp.noise_source = None
    outs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        outs.append(smp.interpolate(x1, x2, t=t, lam=lam))
    assert same_bits(outs[0], outs[1]) and not same_bits(outs[0], outs[2])
    assert bool(torch.isfinite(outs[0]).all())


# ----------------------------------------------------------------------------- chaining, against the reference's loops
def test_eight_p_sample_calls_reproduce_the_reference_loop():
    smp, net, g = _sr3("loop_sr3_lin_8")
    cond = cases.make_cond("sr3_loop").cuda()
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(2, 3, 32, 32) for _ in range(8)]                     # init + T - 1 steps, reference draw order
    src = smp.noise_source = Source(draws[1:])
    img = draws[0].cuda()
    for i in reversed(range(8)):
        img = smp.p_sample(img, i, condition_x=cond)
    assert len(src.shapes) == 7 and not src.draws
    _within("sr3 chained p_sample vs loop_sr3_lin_8", img, g["ret"][-2:])
    assert maxabs(img[-1].cpu(), g["last"]) <= FP32_TOL
    smp.noise_source = Source(draws)
    smp.p_sample_loop(cond)
    print(f"sr3 loop vs chained p_sample: max|diff| = {maxabs(smp.last_full_batch.cpu(), img.cpu()):.3e}")
    assert torch.equal(smp.last_full_batch, img)                               # the loop is the single steps


def test_inference_one_step_calls_reproduce_the_reference_loop():
    n = 3
    smp, net, g = _indi(f"loop_indi_n{n}_t1.0", n)
    x_in = cases.make_cond("indi_loop")
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(3, 2, 32, 48) for _ in range(n + 1)]
    src = smp.noise_source = Source(draws[1:])
    x = (torch.cat([x_in] * 2, dim=1) + draws[0] * (0.01 * torch.Tensor([1.0]))).cuda()    # indi.py:80-82
    delta, cur = 1.0 / n, 1.0
    for _ in range(smp.num_timesteps):
        x = smp.inference_one_step(x, delta, cur)
        cur -= delta
    assert len(src.shapes) == n
    _within(f"indi chained inference_one_step vs loop_indi_n{n}_t1.0", x, g["ret"][-3:])
    smp.noise_source = Source(draws)
    smp.inference(x_in.cuda())
    print(f"indi loop vs chained inference_one_step: max|diff| = {maxabs(smp.last_full_batch.cpu(), x.cpu()):.3e}")
    assert torch.equal(smp.last_full_batch, x)                                 # the loop is the single steps


# ----------------------------------------------------------------------------- the loop's update is the single step's
# k_update and k_step share one arithmetic (step_update).  With the final conv's weights zero the UNet returns
# its bias in every executor, so the loop and the chained single steps can differ in the update alone: equal values
# (torch.equal: the loop adds z * 0 where the single step adds nothing, a difference in the sign of a zero at most).
T_EQ = 8


@pytest.mark.parametrize("clip", [True, False])
def test_ddpm_loop_equals_chained_p_sample_on_a_constant_unet(clip):
    smp, net, _ = _ddpm("interpolate_ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"], 2, False)
    shape = (2, 2, 16, 16)
    constant_unet(net, 2)
    draws = [nets.rand(shape, 100 + i) for i in range(T_EQ + 1)]                  # the start, then one per step
    smp.noise_source = Source(draws)
    loop = smp.p_sample_loop(shape, clip_denoised=clip)
    assert loop.shape == shape and not smp.noise_source.draws
    src = smp.noise_source = Source(draws[1:])
    x = draws[0].cuda()
    for i in reversed(range(T_EQ)):
        x = smp.p_sample(x, torch.full((2,), i, dtype=torch.long, device="cuda"), clip_denoised=clip)
    assert not src.draws
    assert torch.equal(loop, x)


@pytest.mark.parametrize("t_start", [1.0, (1.0, 0.5, 0.75)])
def test_indi_inference_equals_chained_one_steps_on_a_constant_unet(t_start):
    """One start time, and one per sample (binary fractions: the host's cur_t -= delta never undershoots delta).  The
    per-sample loop is compared sample by sample: inference_one_step takes one time for its whole batch."""
    n = T_EQ
    smp, net, _ = _indi("loop_indi_n3_t1.0", n)
    constant_unet(net, 3)
    x_in = nets.rand((3, 1, 16, 16), 60)
    one = (1, 2, 16, 16)
    per_sample = isinstance(t_start, tuple)
    if per_sample:                                                             # sample by sample: start, then n steps
        draws = [[nets.rand(one, 1000 * b + i) for i in range(n + 1)] for b in range(3)]
        smp.noise_source = Source([d for per in draws for d in per])
        smp.inference(x_in.cuda(), t_float_start=torch.tensor(t_start))
    else:
        flat = [nets.rand((3, 2, 16, 16), 300 + i) for i in range(n + 1)]
        draws = [[d[b:b + 1].contiguous() for d in flat] for b in range(3)]
        smp.noise_source = Source(flat)
        smp.inference(x_in.cuda(), t_float_start=t_start)
    assert not smp.noise_source.draws
    loop = smp.last_full_batch
    assert loop.shape == (3, 2, 16, 16)
    for b in range(3):
        t0 = t_start[b] if per_sample else t_start
        src = smp.noise_source = Source(draws[b][1:])
        xr = torch.cat([x_in[b:b + 1]] * 2, dim=1).cuda()
        x = xr + draws[b][0].cuda() * (smp.e * torch.Tensor([t0])).cuda()      # indi.py:80-82
        delta, cur = t0 / n, t0
        for _ in range(n):
            x = smp.inference_one_step(x, delta, cur)
            cur -= delta
        assert not src.draws
        assert torch.equal(loop[b:b + 1], x), b
