"""Few-step solvers on the device (`-m gpu`): dsx_solver_step against the fp32 numpy recurrence (tests/solver_ref.py),
DDIM rows through dsx_solver_loop against the ancestral kernel on the same rows, the DPM-Solver++(2M) loop against the
chain of single steps and against the recurrence, graph handling, snapshots, the 16-bit executor, per-sample noise
streams and the command line."""
import json

import numpy as np
import pytest
import torch

from oracle import cases
from tests import nets, solver_ref
from tests.gpu_util import psnr
from tests.steps_util import BIAS, Source, constant_unet, off
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SCHED = dict(schedule="linear", n_timestep=20, linear_start=1e-4, linear_end=1e-1)
HW = (16, 16)
K = 5


def _sr3(dtype="f32"):
    from diffsplitting_amd.model.samplers import GaussianSampler
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    net = nets.unet("sr3", cases.UNET_CASES["sr3_tiny"]["cfg"])
    net.compute_dtype = dtype
    smp = GaussianSampler(net, 32, channels=3, conditional=True).cuda()
    smp.set_new_noise_schedule(SCHED, "cuda")
    nets.load(smp, sd)
    return smp


def _ddpm():
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    sd, _ = golden_state_dict("interpolate_ddpm")
    net = nets.unet("ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"])
    smp = GaussianSamplerDdpm(net, 32, channels=2, conditional=False).cuda()
    smp.set_new_noise_schedule(SCHED, "cuda")
    nets.load(smp, sd)
    return smp


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- dsx_solver_step against the recurrence
# per-sample coefficients, all different; cp is 0 for samples 0 and 2, sigma is 0 for sample 1
COEF = dict(a=torch.tensor([1.0371, 2.2360679, 1.0000501]), b=torch.tensor([0.2748, 2.0, 0.0100123]),
            cx=torch.tensor([0.1, 0.654321, 0.0123]), c0=torch.tensor([0.75623951, 0.31, 0.9990234]),
            cp=torch.tensor([0.0, -0.2137, 0.0]), sigma=torch.tensor([0.37, 0.0, 0.81]))
SHAPES = [(2, 3, 8, 8),       # 16-byte path
          (3, 3, 5, 7),       # H*W = 35: scalar path, groups of four straddle rows and samples
          (3, 1, 64, 67)]     # scalar path, more than one workgroup


def _inputs(shape, seed):
    """x, net, the previous x0 -- NaN for every sample whose cp is 0 -- and z."""
    B = shape[0]
    co = {k: v[:B] for k, v in COEF.items()}
    x, net, prev, z = nets.rand(shape, seed), 0.7 * nets.rand(shape, seed + 1), nets.rand(shape, seed + 2), nets.rand(shape, seed + 3)
    prev[co["cp"] == 0] = float("nan")
    return co, x, net, prev, z


def _ref(co, x, net, prev, z, clip):
    row = {k: _np(v).reshape(-1, 1, 1, 1) for k, v in co.items()}
    x0, out = solver_ref.step(row, _np(x), _np(net), _np(prev), _np(z), clip=clip)
    assert np.isfinite(x0).all() and np.isfinite(out).all()
    return torch.from_numpy(x0), torch.from_numpy(out)


def _step(co, x, net, prev, put=lambda t: t.cuda(), **kw):
    from diffsplitting_amd import engine
    d = {k: v.cuda() for k, v in co.items()}
    return engine.solver_step(put(x) if not x.is_cuda else x, put(net), d["a"], d["b"], d["cx"], d["c0"], d["sigma"], cp=d["cp"],
                              x0_prev=None if prev is None else (put(prev) if not prev.is_cuda else prev), **kw)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_solver_step_is_the_recurrence(shape, clip):
    co, x, net, prev, z = _inputs(shape, 10)
    rx0, rout = _ref(co, x, net, prev, z, clip)
    if clip:
        assert bool((rx0.abs() == 1).any())                                  # the clamp is exercised
    x0, out = _step(co, x, net, prev, clip=clip, z=z.cuda())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x0).all())     # the poisoned x0_prev was not read
    assert torch.equal(x0.cpu(), rx0) and torch.equal(out.cpu(), rout)
    # in place: x_out is x, x_recon_out is x0_prev
    xg, pg = x.cuda(), prev.cuda()
    r = _step(co, xg, net, pg, clip=clip, z=z.cuda(), x_out=xg, x_recon_out=pg)
    assert r[1].data_ptr() == xg.data_ptr() and r[0].data_ptr() == pg.data_ptr()
    assert torch.equal(xg.cpu(), rout) and torch.equal(pg.cpu(), rx0)
    # base pointers one float past a 16-byte boundary: the scalar path whatever H*W is
    outs = [torch.full((x.numel() + 1,), -7.25, device="cuda")[1:].view(shape) for _ in range(2)]
    _step(co, x, net, prev, put=off, clip=clip, z=off(z), x_recon_out=outs[0], x_out=outs[1])
    assert torch.equal(outs[0].cpu(), rx0) and torch.equal(outs[1].cpu(), rout)
    # no history at all: every cp counts as 0
    co0 = dict(co, cp=torch.zeros_like(co["cp"]))
    r0 = _ref(co0, x, net, prev, z, clip)
    g0 = _step(co, x, net, None, clip=clip, z=z.cuda())
    assert torch.equal(g0[0].cpu(), r0[0]) and torch.equal(g0[1].cpu(), r0[1])


@pytest.mark.parametrize("shape", SHAPES)
def test_solver_step_draws_what_randn_writes(shape):
    from diffsplitting_amd import engine
    co, x, net, prev, _ = _inputs(shape, 20)
    z = engine.randn(shape, 1234, 77)
    want = _step(co, x, net, prev, clip=True, z=z)
    got = _step(co, x, net, prev, clip=True, seed=1234, subsequence=77)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(_step(co, x, net, prev, clip=True, seed=1234, subsequence=78)[1], want[1])
    ids = [5, 9, 2][:shape[0]]
    zs = engine.randn_samples(shape, 99, ids, draw=3)
    want = _step(co, x, net, prev, clip=True, z=zs)
    got = _step(co, x, net, prev, clip=True, seed=99, sample_ids=ids, draw=3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = _step(co, x, net, prev, put=off, clip=True, seed=99, sample_ids=ids, draw=3)            # scalar path
    assert torch.equal(got[1], want[1])


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_solver_columns_map_onto_the_posterior_step(shape, clip):
    """Without a history a solver step is the ancestral step with c1 = c0 (x0's coefficient) and c2 = cx (x's): the
    solver's argument order is cx, c0, and COEF's two columns differ, so a swap cannot pass."""
    from diffsplitting_amd import engine
    co, x, net, _, z = _inputs(shape, 25)
    d = {k: v.cuda() for k, v in co.items()}
    assert not torch.equal(co["cx"], co["c0"])
    ids = [5, 9, 2][:shape[0]]
    for kw in (dict(z=z.cuda()), dict(seed=1234, subsequence=77), dict(seed=99, sample_ids=ids, draw=3)):
        x0, out = engine.solver_step(x.cuda(), net.cuda(), d["a"], d["b"], d["cx"], d["c0"], d["sigma"], clip=clip, **kw)
        px0, _, pout = engine.posterior_step(x.cuda(), net.cuda(), c1=d["c0"], c2=d["cx"], sigma=d["sigma"], a=d["a"], b=d["b"],
                                             predict_eps=True, clip=clip, x_recon_out=torch.empty(shape, device="cuda"),
                                             x_out=torch.empty(shape, device="cuda"), **kw)
        assert bool(torch.isfinite(out).all()) and torch.equal(x0, px0) and torch.equal(out, pout), kw


# ----------------------------------------------------------------------------- ddim rows: the ancestral kernel's bits
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_ddim_rows_through_both_loops_give_the_same_bits(eta):
    from diffsplitting_amd import engine
    smp = _sr3()
    B = 2
    shape = (B, 3) + HW
    cond, start = nets.rand(shape, 30).cuda(), nets.rand(shape, 31).cuda()
    t = smp.solver_table(steps=K, solver="ddim", eta=eta, spacing="uniform")
    assert t.n_steps == K and t.timesteps == [19, 14, 10, 5, 0] and np.all(t.cp == 0)
    assert np.all(t.sigma[:-1] > 0) if eta else np.all(t.sigma == 0)
    eng = smp.denoise_fn.engine()
    noise = torch.stack([nets.rand(shape, 40 + k) for k in range(K)]).cuda()
    for kw in (dict(noise=noise), dict(seed=4321), dict(seed=4321, sample_ids=[7, 3])):
        a, _ = eng.sample_loop(t.step_table(), start.clone(), cond=cond, **kw)
        s, _ = eng.solver_loop(t, start.clone(), cond=cond, **kw)
        assert bool(torch.isfinite(s).all()) and torch.equal(a, s), kw
    if eta:
        assert not torch.equal(eng.solver_loop(t, start.clone(), cond=cond, seed=4322)[0], s)


# ----------------------------------------------------------------------------- 2M: the loop is the chain of single steps
def _chain(smp, t, start, cond, clip=True):
    """UNet forward through the sampler's denoise_fn with the row's tcond, then engine.solver_step; the x0 history is
    carried here.  Returns the state after every row."""
    from diffsplitting_amd import engine
    B = start.shape[0]
    x, prev, states = start.clone(), None, []
    for k in range(t.n_steps):
        col = lambda name: torch.full((B,), float(getattr(t, name)[k]), device="cuda")
        time = col("tcond").view(B, 1) if smp.kind == "sr3" else col("tcond")
        net = smp.denoise_fn(x if cond is None else torch.cat([cond, x], dim=1), time)
        prev, x = engine.solver_step(x, net, col("a"), col("b"), col("cx"), col("c0"), col("sigma"), cp=col("cp"),
                                     x0_prev=prev, clip=clip)
        states.append(x)
    return states


@pytest.mark.parametrize("kind", ["sr3", "ddpm"])
def test_2m_loop_equals_the_chain_of_single_steps(kind):
    smp = _sr3() if kind == "sr3" else _ddpm()
    B, C = 2, smp.channels
    shape = (B, C) + HW
    cond = nets.rand((B, 3) + HW, 50).cuda() if kind == "sr3" else None
    start = nets.rand(shape, 51)
    t = smp.solver_table(steps=K)
    assert t.n_steps == K and np.all(t.cp[1:-1] != 0) and t.cp[0] == 0
    states = _chain(smp, t, start.cuda(), cond)
    smp.noise_source = Source([start])
    ret = smp.solver_sample_loop(cond if kind == "sr3" else shape, steps=K, continous=True)
    assert not smp.noise_source.draws and torch.equal(smp.last_full_batch, states[-1])
    if kind == "sr3":                                          # the start (the conditioning image), then every row's state
        assert ret.shape == ((K + 1) * B, C) + HW and torch.equal(ret[:B], cond)
        for k in range(K):
            assert torch.equal(ret[(k + 1) * B:(k + 2) * B], states[k]), k
    # snapshots after rows 0 and K - 1
    x, sn = smp.denoise_fn.engine().solver_loop(t, start.cuda(), cond=cond, snapshot_steps=[0, K - 1])
    assert torch.equal(sn[0], states[0]) and torch.equal(sn[1], states[-1]) and torch.equal(x, states[-1])
    # the history matters: the same rows without it end elsewhere
    t0 = smp.solver_table(steps=K)
    t0.cp[:] = 0
    assert not torch.equal(smp.denoise_fn.engine().solver_loop(t0, start.cuda(), cond=cond)[0], states[-1])


@pytest.mark.parametrize("clip", [True, False])
def test_2m_loop_on_a_constant_unet_is_the_recurrence(clip):
    """With the final conv's weights zero the UNet returns its bias, so the update and the x0 history are checked
    apart from the UNet: x0 = a*x - b*bias still varies with x."""
    smp = _ddpm()
    B = 2
    shape = (B, 2) + HW
    constant_unet(smp.denoise_fn, B)
    start = nets.rand(shape, 60)
    t = smp.solver_table(steps=K, clip_denoised=clip)
    net = np.broadcast_to(np.asarray(BIAS, dtype=np.float32).reshape(1, 2, 1, 1), shape)
    states, x0s = solver_ref.run(t.columns(), _np(start), lambda k, x: net, clip=clip)
    assert any(not np.array_equal(x0s[k], x0s[k + 1]) for k in range(K - 1))
    if clip:
        assert any((np.abs(x0) == 1).any() for x0 in x0s)
    smp.noise_source = Source([start])
    ret = smp.solver_sample_loop(shape, steps=K, clip_denoised=clip)
    assert torch.equal(ret.cpu(), torch.from_numpy(states[-1]))
    _, sn = smp.denoise_fn.engine().solver_loop(t, start.cuda(), snapshot_steps=range(K))
    for k in range(K):
        assert torch.equal(sn[k].cpu(), torch.from_numpy(states[k])), k


# ----------------------------------------------------------------------------- graph handling
def _run(smp, shape, start, steps, **kw):
    smp.noise_source = Source([start])
    return smp.solver_sample_loop(shape, steps=steps, **kw).clone()


def _ancestral(smp, shape, draws):
    smp.noise_source = Source(draws)
    return smp.p_sample_loop(shape).clone()


def test_graphs_are_kept_apart_and_history_is_not_stale():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.model import solvers
    shape = (2, 2) + HW
    start, other = nets.rand(shape, 70), nets.rand(shape, 71)
    draws = [nets.rand(shape, 80 + i) for i in range(SCHED["n_timestep"] + 1)]      # the start, then one per step (ddpm)
    fresh5, fresh3, fresh_anc = _run(_ddpm(), shape, start, 5), _run(_ddpm(), shape, other, 3), _ancestral(_ddpm(), shape, draws)
    assert not torch.equal(fresh5, fresh3)
    eager = _ddpm()
    eager.use_graph = False
    assert torch.equal(_run(eager, shape, start, 5), fresh5)                   # use_graph = 0 equals use_graph = 1
    smp = _ddpm()
    eng = smp.denoise_fn.engine()
    ws = eng.workspace_bytes(2, *HW)
    assert torch.equal(_run(smp, shape, start, 5), fresh5)
    assert torch.equal(_run(smp, shape, other, 3), fresh3)                     # K = 5, then K = 3 on one executor
    assert eng.workspace_bytes(2, *HW) == ws                                   # the history lives outside the workspace
    # ancestral, solver, ancestral on one sampler: each replays its own step
    assert torch.equal(_ancestral(smp, shape, draws), fresh_anc)
    assert torch.equal(_run(smp, shape, start, 5), fresh5)
    assert torch.equal(_ancestral(smp, shape, draws), fresh_anc)
    # refusals that need an executor
    t = smp.solver_table(steps=K)
    bad = solvers.SolverTableHost(**dict(t.columns(), cp=np.full(K, 0.5, dtype=np.float32)))
    with pytest.raises(DsxError, match="no previous x0 at the first step"):
        eng.solver_loop(bad, start.cuda())
    with pytest.raises(DsxError, match="sample_ids must hold B = 2"):
        eng.solver_loop(t, start.cuda(), seed=1, sample_ids=[1, 2, 3])
    with pytest.raises(DsxError, match="sample_ids together with injected noise"):
        eng.solver_loop(t, start.cuda(), noise=torch.zeros((K,) + shape).cuda(), seed=1, sample_ids=[1, 2])
    with pytest.raises(DsxError, match="pass a CUDA tensor"):
        _sr3().solver_sample_loop(torch.zeros(2, 3, *HW), steps=K)


# ----------------------------------------------------------------------------- 16-bit executor
def test_2m_loop_on_the_bf16_executor_runs_and_repeats():
    B = 2
    cond, start = nets.rand((B, 3) + HW, 90), nets.rand((B, 3) + HW, 91)
    outs = {}
    for dtype in ("f32", "bf16"):
        smp = _sr3(dtype)
        smp.noise_source = Source([start, start])
        smp.solver_sample_loop(cond.cuda(), steps=K)
        outs[dtype] = smp.last_full_batch.clone()
        smp.solver_sample_loop(cond.cuda(), steps=K)
        assert torch.equal(smp.last_full_batch, outs[dtype]) and bool(torch.isfinite(outs[dtype]).all()), dtype
    # logged, not bounded: nobody has measured what the 16-bit operands cost the few-step result
    print(f"\n2M K = {K}, bf16 against fp32 from the same start: PSNR {psnr(_np(outs['f32']), _np(outs['bf16'])):.2f} dB")


# ----------------------------------------------------------------------------- per-sample noise streams
@pytest.mark.parametrize("solver, eta", [("ddim", 0.7), ("dpmpp2m", 0.0)])
def test_a_sample_does_not_depend_on_its_batch_position(solver, eta):
    smp = _ddpm()
    shape = (3, 2) + HW
    a = smp.solver_sample_loop(shape, steps=K, solver=solver, eta=eta, seed=17, sample_ids=[5, 9, 2]).clone()
    b = smp.solver_sample_loop(shape, steps=K, solver=solver, eta=eta, seed=17, sample_ids=[9, 5, 2]).clone()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a[1], b[0]) and torch.equal(a[0], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0], a[1])
    c = smp.solver_sample_loop(shape, steps=K, solver=solver, eta=eta, seed=18, sample_ids=[5, 9, 2])
    assert not torch.equal(a, c)


# ----------------------------------------------------------------------------- the command line
def test_infer_with_and_without_a_solver(tmp_path):
    from diffsplitting_amd import infer
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.model import create_model
    from PIL import Image
    rng = np.random.default_rng(12)
    src = tmp_path / "src"
    src.mkdir()
    for k in range(3):
        y, x = np.mgrid[0:64, 0:48]
        smooth = np.stack([127 + 100 * np.sin(x / (5.0 + k) + c) * np.cos(y / (7.0 + c)) for c in range(3)], -1)
        Image.fromarray(np.clip(smooth + rng.normal(0, 12, smooth.shape), 0, 255).astype(np.uint8)).save(src / f"{k}.png")
    section = {"which_model_G": "sr3", "finetune_norm": False,
               "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": 32, "norm_groups": 32,
                        "channel_multiplier": [1, 2, 4], "attn_res": [16], "res_blocks": 2, "dropout": 0.2},
               "beta_schedule": {"train": dict(SCHED), "val": dict(SCHED)},
               "diffusion": {"image_size": 32, "channels": 3, "conditional": True}}
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    model = create_model(dict_to_nonedict({"model": section, "phase": "val", "gpu_ids": [0], "distributed": False,
                                           "path": {"resume_state": None, "checkpoint": str(tmp_path)}}))
    model.netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()}, strict=False)
    model.save_network(epoch=1, iter_step=10)

    def run(name, *flags):
        cfg = {"name": name, "phase": "val", "gpu_ids": [0],
               "path": {"log": str(tmp_path / name / "logs"), "results": str(tmp_path / name / "results"),
                        "checkpoint": str(tmp_path), "resume_state": str(tmp_path / "I10_E1")},
               "datasets": {"val": {"name": "tiny", "mode": "LRHR", "dataroot": str(src), "datatype": "hr_only",
                                    "l_resolution": 8, "r_resolution": 32, "data_len": -1}},
               "model": section}
        p = tmp_path / f"{name}.json"
        p.write_text(json.dumps(cfg))
        return infer.main(["-c", str(p), "-p", "val", "-gpu", "0", "--batch", "3", *flags]), tmp_path / name / "results"

    res, out = run("few", "--solver", "dpmpp2m", "--solver-steps", "4", "--sample-seed", "11")
    for idx in range(1, 4):
        assert all((out / f"0_{idx}_{kind}.png").exists() for kind in ("hr", "sr", "inf"))
    print(f"\ninfer --solver dpmpp2m --solver-steps 4: PSNR {res['psnr']:.4f}, SSIM {res['ssim']:.6f}")
    assert np.isfinite(res["psnr"]) and -1.0 <= res["ssim"] <= 1.0 and len(res["files"]) == 3
    assert res["diffusion"].solver == dict(solver="dpmpp2m", steps=4, eta=0.0, spacing=None)
    netG = res["diffusion"].netG
    want = netG.solver_sample_loop(res["diffusion"].data["SR"], steps=4, seed=11, sample_ids=range(3))
    assert torch.equal(netG.last_full_batch[-1], want)
    infer._save(netG.last_full_batch[1], str(tmp_path / "few_1.png"))
    assert (tmp_path / "few_1.png").read_bytes() == (out / "0_2_sr.png").read_bytes()
    # without --solver: the ancestral loop, byte for byte
    res, out = run("full", "--sample-seed", "11")
    assert res["diffusion"].solver is None
    netG = res["diffusion"].netG
    netG.p_sample_loop(res["diffusion"].data["SR"], seed=11, sample_ids=range(3))
    for b in range(3):
        infer._save(netG.last_full_batch[b], str(tmp_path / f"full_{b}.png"))
        assert (tmp_path / f"full_{b}.png").read_bytes() == (out / f"0_{b + 1}_sr.png").read_bytes()
    with pytest.raises(SystemExit, match="--solver needs --solver-steps"):
        run("bad", "--solver", "ddim")
    with pytest.raises(SystemExit, match="belong to --solver"):
        run("bad", "--eta", "0.5")
