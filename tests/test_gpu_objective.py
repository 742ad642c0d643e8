"""The training objective's forward half on the MI355X (`-m gpu`): dsx_q_sample bit-exact against the reference's
torch expression, its Philox path against dsx_randn, dsx_loss against float64 numpy, and p_losses of the four sampler
families against the fixtures the reference wrote (tools/gen_objective_golden.py)."""
import numpy as np
import pytest
import torch

from oracle import cases
from tests import nets
from tests.bits import bits, same_bits
from tests.steps_util import ref_q as _ref_q
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FP32_TOL = 1e-3          # the project's per-pixel fp32 bound on a UNet output
N_INDI = 20


COEF = (torch.tensor([0.75623951, 0.31, 0.9990234]), torch.tensor([0.1, 1.0, 0.45]), torch.tensor([0.654321, 0.0123, 0.7]))


# ----------------------------------------------------------------------------- q_sample, injected z
@pytest.mark.parametrize("shape,Ce", [
    ((3, 2, 5, 7), 0),       # H*W = 35: scalar path, groups of four straddle rows
    ((3, 3, 8, 12), 0),      # vector path
    ((3, 2, 5, 7), 2),       # three terms, scalar
    ((3, 3, 8, 12), 3),      # three terms, vector
    ((3, 2, 8, 12), 1),      # Ce = 1 broadcast into C = 2, vector
    ((3, 2, 5, 7), 1),       # Ce = 1 broadcast into C = 2, scalar
    ((3, 2, 64, 67), 1),     # more than one workgroup's worth of groups
])
def test_q_sample_bit_exact(shape, Ce):
    from diffsplitting_amd import engine
    B, Cn, H, W = shape
    x0, z = nets.rand(shape, 1), nets.rand(shape, 2)
    xe = nets.rand((B, Ce, H, W), 3) if Ce else None
    c0, c1, c2 = COEF
    ref = _ref_q(x0, c0, c2, z, xe, c1 if Ce else None)
    out, z_used = engine.q_sample(x0.cuda(), c0.cuda(), c2.cuda(), xe=None if xe is None else xe.cuda(),
                                  c1=c1.cuda() if Ce else None, z=z.cuda())
    assert same_bits(out, ref) and same_bits(z_used, z)


@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)])
def test_q_sample_channel_offset_leaves_the_rest_untouched(H, W):
    """Cdst = 5, coff = 3: with H*W = 35 the destination rows are misaligned; the other three channels keep the
    sentinel."""
    from diffsplitting_amd import engine
    shape = (3, 2, H, W)
    x0, z, xe = nets.rand(shape, 4), nets.rand(shape, 5), nets.rand((3, 1, H, W), 6)
    c0, c1, c2 = COEF
    dst = torch.full((3, 5, H, W), -7.25, device="cuda")
    out, _ = engine.q_sample(x0.cuda(), c0.cuda(), c2.cuda(), xe=xe.cuda(), c1=c1.cuda(), z=z.cuda(), dst=dst, coff=3)
    assert out is dst
    assert same_bits(dst[:, 3:5], _ref_q(x0, c0, c2, z, xe, c1))
    assert bool((dst[:, :3] == -7.25).all())


def test_q_sample_unaligned_base_pointers_take_the_scalar_path():
    """H*W a multiple of 4 but the tensors start 4 bytes past a 16-byte boundary."""
    from diffsplitting_amd import engine
    shape = (3, 2, 8, 12)
    n = 3 * 2 * 8 * 12
    x0, z = nets.rand(shape, 7), nets.rand(shape, 8)
    c0, _, c2 = COEF
    off = lambda t: torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()[1:].view(t.shape)
    xo, zo = off(x0), off(z)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    dst = torch.zeros(n + 1, device="cuda")[1:].view(shape)
    engine.q_sample(xo, c0.cuda(), c2.cuda(), z=zo, dst=dst)
    assert same_bits(dst, _ref_q(x0, c0, c2, z))


@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (3, 2, 8, 12)])
def test_q_sample_two_terms_add_no_zero_term(shape):
    """x0 = -0.0 and z = -0.0 at the same places: c0*x0 + c2*z = -0.0, while a third term +0.0 would give +0.0."""
    from diffsplitting_amd import engine
    x0, z = nets.rand(shape, 9), nets.rand(shape, 10)
    x0.view(-1)[::3] = -0.0
    z.view(-1)[::3] = -0.0
    c0, _, c2 = COEF
    ref = _ref_q(x0, c0, c2, z)
    assert bool((bits(ref).view(-1)[::3] == -2 ** 31).all())           # the sign bit alone: -0.0
    out, _ = engine.q_sample(x0.cuda(), c0.cuda(), c2.cuda(), z=z.cuda())
    assert same_bits(out, ref)


# ----------------------------------------------------------------------------- q_sample, Philox z
@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (3, 3, 8, 12), (2, 1, 64, 67)])
def test_q_sample_philox_path(shape):
    from diffsplitting_amd import engine
    x0 = nets.rand(shape, 11)
    xe = nets.rand((shape[0], 1) + shape[2:], 12)
    c0, c1, c2 = (c[:shape[0]] for c in COEF)
    args = (x0.cuda(), c0.cuda(), c2.cuda())
    for kw in (dict(), dict(xe=xe.cuda(), c1=c1.cuda())):
        out, z = engine.q_sample(*args, seed=1234, subsequence=5, want_z=True, **kw)
        assert same_bits(z, engine.randn(shape, 1234, 5))               # what dsx_randn writes for (seed, subsequence)
        inj, _ = engine.q_sample(*args, z=z, **kw)
        assert same_bits(out, inj)
        assert same_bits(out, _ref_q(x0, c0, c2, z.cpu(), xe if kw else None, c1 if kw else None))
        again, z_none = engine.q_sample(*args, seed=1234, subsequence=5, **kw)
        assert z_none is None and same_bits(again, out)                  # same seed, with and without z_out
        other, _ = engine.q_sample(*args, seed=1235, subsequence=5, **kw)
        assert not same_bits(other, out)
        other, _ = engine.q_sample(*args, seed=1234, subsequence=6, **kw)
        assert not same_bits(other, out)


# ----------------------------------------------------------------------------- dsx_loss
def _loss_sampler(loss_type, reduction):
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    s = GaussianSamplerDdpm(None, 32, loss_type=loss_type, lr_reduction=reduction)
    s.set_loss("cuda")
    return s


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 3, 64, 67)])   # 105 elements: one partial; 12864: several
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_loss_against_float64_numpy(shape, loss_type):
    """Relative error <= 2^-23: the terms are exact (L1) or correctly rounded (L2) in double, the summation order costs
    at most N 2^-53, and the result is rounded to fp32 once."""
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import lib
    a, b = nets.rand(shape, 13), nets.rand(shape, 14)
    d = a.numpy().astype(np.float64) - b.numpy().astype(np.float64)
    term = np.abs(d) if loss_type == "l1" else d * d
    want = term.reshape(shape[0], -1).sum(axis=1)
    blocks = lib.dsx_loss_blocks(*shape[1:])
    assert (blocks == 1) == (shape[1] * shape[2] * shape[3] <= 4096) and blocks >= 1
    ag, bg = a.cuda(), b.cuda()
    per = engine.loss_per_sample(ag, bg, squared=loss_type == "l2")
    assert per.dtype == torch.float64 and per.shape == (shape[0],)
    rel = np.abs(per.cpu().numpy() - want) / want
    print(f"\ndsx_loss {loss_type} {shape}: per-sample rel err {rel.max():.3e}")
    assert rel.max() <= 2.0 ** -23
    assert torch.equal(per, engine.loss_per_sample(ag, bg, squared=loss_type == "l2"))    # bitwise repeatable
    for reduction, ref in (("sum", want.sum()), ("mean", want.sum() / a.numel())):
        got = _loss_sampler(loss_type, reduction)._loss(ag, bg)
        assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda and not got.requires_grad
        assert abs(float(got) - ref) / ref <= 2.0 ** -23
        assert same_bits(got, _loss_sampler(loss_type, reduction)._loss(ag, bg))
    zero = engine.loss_per_sample(ag, ag.clone(), squared=loss_type == "l2")
    assert bool((zero == 0).all())                                                        # a == b: exactly 0


# ----------------------------------------------------------------------------- parity with the reference
def _hook(net):
    rec = {}
    net.register_forward_hook(lambda m, inp, out: rec.update(x_recon=out))
    return rec


def _loss64(a, b, loss_type, reduction):
    """(float64 loss of the fixture's own tensors, the deviation the per-pixel bound FP32_TOL on b allows)."""
    a, b = np.broadcast_arrays(a.astype(np.float64), b.astype(np.float64))
    d = a - b
    if loss_type == "l1":
        val, tol = np.abs(d).sum(), FP32_TOL * d.size
    else:
        val, tol = (d * d).sum(), (2 * np.abs(d) * FP32_TOL + FP32_TOL ** 2).sum()
    n = d.size if reduction == "mean" else 1
    return val / n, tol / n, d.size


def _check_loss(name, got, g_loss, a, x_recon_ref, loss_type, reduction):
    ref, tol, n = _loss64(a, x_recon_ref, loss_type, reduction)
    assert abs(float(g_loss) - ref) <= n * 2.0 ** -24 * abs(ref)          # the fixture: within fp32 summation error
    print(f"\n{name}: loss {float(got):.6f}, float64 of the fixture {ref:.6f}, |diff| {abs(float(got) - ref):.3e} "
          f"(allowed {tol:.3e}), reference fp32 {float(g_loss):.6f}")
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda and not got.requires_grad
    assert abs(float(got) - ref) <= tol


def _check_recon(name, x_recon, ref):
    err = float(np.abs(x_recon.cpu().numpy().astype(np.float64) - ref).max())
    print(f"\n{name}: max|x_recon - reference| = {err:.3e}")
    assert err <= FP32_TOL


def test_p_losses_sr3_matches_the_reference():
    from diffsplitting_amd.model.samplers import GaussianSampler
    sd, g = golden_state_dict("objective_sr3")
    net = nets.unet("sr3", cases.UNET_CASES["sr3_tiny"]["cfg"])
    smp = GaussianSampler(net, 32, channels=3, loss_type="l1", conditional=True).cuda()
    smp.set_new_noise_schedule(cases.SCHEDULES["lin_25"], "cuda")
    smp.set_loss("cuda")
    nets.load(smp, sd)
    c = torch.from_numpy(g["continuous_sqrt_alpha_cumprod"])
    target, noise = torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["noise"]).cuda()
    assert same_bits(smp.q_sample(target, c, noise=noise), torch.from_numpy(g["x_noisy"]))
    rec = _hook(net)
    x_in = {"target": target, "input": torch.from_numpy(g["input"]).cuda()}
    loss = smp(x_in, noise, continuous_sqrt_alpha_cumprod=c)
    _check_recon("sr3", rec["x_recon"], g["x_recon"])
    _check_loss("sr3", loss, g["loss"], g["noise"], g["x_recon"], "l1", "sum")
    # the seeded host draws reproduce the reference's run: same t, same noise levels, same loss
    np.random.seed(int(g["seed_numpy"]))
    assert same_bits(smp.p_losses(x_in, noise), loss)
    # device noise: repeatable under torch's seed, finite, and another seed gives another value
    vals = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        vals.append(float(smp.p_losses(x_in, continuous_sqrt_alpha_cumprod=c)))
    assert vals[0] == vals[1] != vals[2] and np.isfinite(vals).all()


def test_p_losses_ddpm_matches_the_reference():
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    sd, g = golden_state_dict("objective_ddpm")
    net = nets.unet("ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"])
    smp = GaussianSamplerDdpm(net, 32, channels=1, loss_type="l2", lr_reduction="mean", conditional=True).cuda()
    smp.set_new_noise_schedule(cases.SCHEDULES["lin_8"], "cuda")
    smp.set_loss("cuda")
    nets.load(smp, sd)
    t = torch.from_numpy(g["t"])
    target, noise = torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["noise"]).cuda()
    assert same_bits(smp.q_sample(target, t.cuda(), noise=noise), torch.from_numpy(g["x_noisy"]))
    rec = _hook(net)
    x_in = {"target": target, "input": torch.from_numpy(g["input"]).cuda()}
    loss = smp(x_in, noise, t=t)
    _check_recon("ddpm", rec["x_recon"], g["x_recon"])
    _check_loss("ddpm", loss, g["loss"], g["noise"], g["x_recon"], "l2", "mean")
    torch.manual_seed(int(g["seed_torch"]))                   # the reference's own draw of t
    assert same_bits(smp.p_losses(x_in, noise), loss)


def test_p_losses_indi_matches_the_reference():
    from diffsplitting_amd.model.samplers import InDISampler
    sd, g = golden_state_dict("objective_indi")
    net = nets.unet("ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"])
    smp = InDISampler(net, 32, channels=2, loss_type="l1", out_channel=2, conditional=False,
                      val_schedule_opt={"n_timestep": N_INDI}).cuda()
    smp.set_new_noise_schedule({"n_timestep": N_INDI}, "cuda")
    smp.set_loss("cuda")
    nets.load(smp, sd)
    t = torch.from_numpy(g["t"])
    target, noise, inp = (torch.from_numpy(g[k]).cuda() for k in ("target", "noise", "input"))
    assert same_bits(smp.q_sample(target, inp, t, noise=noise), torch.from_numpy(g["x_noisy"]))
    assert same_bits(smp.q_sample(target, torch.cat([inp] * 2, dim=1), t.cuda(), noise=noise), torch.from_numpy(g["x_noisy"]))
    x_in = {"target": target, "input": inp}
    x_recon = smp.get_prediction_during_training(x_in, noise, t=t)
    _check_recon("indi", x_recon, g["x_recon"])
    loss = smp(x_in, noise, t=t)
    _check_loss("indi", loss, g["loss"], g["target"], g["x_recon"], "l1", "sum")
    torch.manual_seed(int(g["seed_torch"]))                   # the reference's own draw of t
    assert same_bits(smp.p_losses(x_in, noise), loss)


@pytest.mark.parametrize("tag,full", [("custom", False), ("full", True)])
def test_p_losses_joint_matches_the_reference(tag, full):
    from diffsplitting_amd.model.samplers import JointIndiSampler
    sd, g = golden_state_dict("objective_joint")
    cfg = cases.UNET_CASES["joint_32"]["cfg"]
    n1, n2 = nets.unet("ddpm", cfg), nets.unet("ddpm", cfg)
    smp = JointIndiSampler(None, 32, channels=1, loss_type="l1", out_channel=1, denoise_fn_ch1=n1, denoise_fn_ch2=n2,
                           conditional=False, val_schedule_opt={"n_timestep": N_INDI}, allow_full_translation=full).cuda()
    smp.load_state_dict(sd, strict=True)
    smp.set_new_noise_schedule({"n_timestep": N_INDI}, "cuda")
    smp.set_loss("cuda")
    target = torch.from_numpy(g["target"]).cuda()
    t1, t2 = torch.from_numpy(g[f"{tag}_t1"]), torch.from_numpy(g[f"{tag}_t2"])
    ch = [target[:, 0:1].contiguous(), target[:, 1:2].contiguous()]
    for i, (indi, t) in enumerate(((smp.indi1, t1), (smp.indi2, t2)), start=1):
        noise = torch.from_numpy(g[f"{tag}_noise{i}"]).cuda()
        x_in = {"target": ch[i - 1], "input": ch[2 - i]}
        assert same_bits(indi.q_sample(x_in["target"], x_in["input"], t, noise=noise), torch.from_numpy(g[f"{tag}_x_noisy{i}"]))
        _check_recon(f"joint {tag} indi{i}", indi.get_prediction_during_training(x_in, noise, t=t), g[f"{tag}_x_recon{i}"])
    # the reference hands ONE `noise` to both samplers (None in the fixture's run, so each drew its own): with one
    # injected tensor, the float64 value is recomputed from the fixture's x_recon only where its noise was used
    rec1, rec2 = _hook(n1), _hook(n2)
    noise1 = torch.from_numpy(g[f"{tag}_noise1"]).cuda()
    loss = smp({"target": target}, noise1, t=(t1, t2))
    _check_recon(f"joint {tag} forward indi1", rec1["x_recon"], g[f"{tag}_x_recon1"])
    l1, tol1, _ = _loss64(g["target"][:, 0:1], g[f"{tag}_x_recon1"], "l1", "sum")
    got1 = smp.indi1._loss(ch[0], rec1["x_recon"])
    assert abs(float(got1) - l1) <= tol1
    got2 = smp.indi2._loss(ch[1], rec2["x_recon"])
    assert same_bits(loss, (got1 + got2) / 2)
    log = smp.get_current_log()
    assert set(log) == {"loss_splitting", "alpha", "offset", "scale"}
    assert log["loss_splitting"] == float(loss)
    assert log["alpha"] == float(torch.sigmoid(smp.alpha_param)) and log["scale"] == float(smp.scale_param)
    assert log["offset"] == float(smp.offset_param)
    # the whole objective against the reference's: each sampler with the noise the reference drew for it
    draws = [torch.from_numpy(g[f"{tag}_noise{i}"]) for i in (1, 2)]
    smp.noise_source = lambda shape: draws.pop(0)
    loss = smp({"target": target}, t=(t1, t2))
    smp.noise_source = None
    ref1, tola, n_a = _loss64(g["target"][:, 0:1], g[f"{tag}_x_recon1"], "l1", "sum")
    ref2, tolb, n_b = _loss64(g["target"][:, 1:2], g[f"{tag}_x_recon2"], "l1", "sum")
    ref, tol = (ref1 + ref2) / 2, (tola + tolb) / 2
    assert abs(float(g[f"{tag}_loss"]) - ref) <= (n_a + n_b) * 2.0 ** -24 * ref
    assert g[f"{tag}_log"][0] == float(g[f"{tag}_loss"])
    print(f"\njoint {tag}: loss {float(loss):.6f}, float64 of the fixture {ref:.6f}, |diff| {abs(float(loss) - ref):.3e} "
          f"(allowed {tol:.3e})")
    assert abs(float(loss) - ref) <= tol
    assert smp.get_current_log()["loss_splitting"] == float(loss)


# ----------------------------------------------------------------------------- boundary
def test_eval_loss_at_the_model_boundary():
    from diffsplitting_amd.model import create_model
    sd, g = golden_state_dict("objective_indi")
    model = create_model(nets.opt(nets.tiny_indi_section()))
    model.netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()}, strict=True)
    model.feed_data({"input": torch.from_numpy(g["input"]), "target": torch.from_numpy(g["target"])})
    torch.manual_seed(5)
    val = model.eval_loss()
    assert isinstance(val, float) and np.isfinite(val) and val > 0
    assert model.get_current_log()["l_pix"] == val
    torch.manual_seed(5)
    again = model.netG(model.data)
    assert not again.requires_grad and again.grad_fn is None and float(again) == val
    with pytest.raises(NotImplementedError):
        model.optimize_parameters()
