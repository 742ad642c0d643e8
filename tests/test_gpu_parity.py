"""Parity of the HIP path (through the C ABI) against the CPU oracle and the
committed golden vectors.  Runs on the MI355X box only (`-m gpu`).

Tolerances (north_star): fp32 path <= 1e-3 max-abs per pixel vs the reference
CPU loop on identical weights + identical injected noise; bf16 operands are
judged by PSNR against the fp32 oracle.
"""
import numpy as np
import pytest
import torch

from oracle import cases, samplers, tiling
from oracle.unet import time_predictor_forward, unet_forward
from tests.gpu_util import DrawRecorder, build_engine, maxabs, psnr
from tests.nets import dev  # noqa: F401  (the fixture)
from tests.util import golden_state_dict, load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3


# ----------------------------------------------------------------------------- UNet forward
@pytest.mark.parametrize("name", ["ddpm_tiny", "sr3_tiny", "joint_32", "hagen_64", "sr3_128"])
def test_unet_forward_fp32(name, dev):
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x, t = cases.make_unet_inputs(name)
    eng = build_engine(case["cfg"], case["flavour"], sd)
    y = eng.forward(x.to(dev), t.to(dev).float()).cpu().numpy()
    ref = unet_forward(sd, case["cfg"], case["flavour"], x, t).numpy()
    assert maxabs(y, ref) <= FP32_TOL, f"vs oracle: {maxabs(y, ref)}"
    assert maxabs(y, g["y"]) <= FP32_TOL, f"vs golden: {maxabs(y, g['y'])}"
    print(f"\n{name}: max|hip-oracle| = {maxabs(y, ref):.3e}  launches={eng.num_launches(*x.shape[:1], *x.shape[2:])}")


def test_unet_forward_cond_split(dev):
    """cond/x passed as two tensors (no torch.cat) gives the same result as the concatenated input."""
    name = "sr3_tiny"
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x, t = cases.make_unet_inputs(name)
    eng = build_engine(case["cfg"], case["flavour"], sd)
    y = eng.forward(x.to(dev), t.to(dev), cond_channels=3).cpu().numpy()
    assert maxabs(y, g["y"]) <= FP32_TOL


@pytest.mark.parametrize("name", ["sr3_tiny", "hagen_64", "sr3_128"])
def test_unet_forward_bf16_psnr(name, dev):
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x, t = cases.make_unet_inputs(name)
    eng = build_engine(case["cfg"], case["flavour"], sd, dtype="bf16")
    y = eng.forward(x.to(dev), t.to(dev).float()).cpu().numpy()
    p = psnr(g["y"], y)
    print(f"\n{name}: bf16 PSNR vs fp32 oracle = {p:.1f} dB, max-abs {maxabs(y, g['y']):.3e}")
    assert p > 35.0


# round 3: items of the persistent kernel carry several 64-byte chunks where a layer has enough of them; the second
# setting lowers the minimum chunk counts so that the small parity grids run the two- and four-chunk forms everywhere
_WS_FORCED = [{}, {"DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4", "DSX_WS_C4_MIN": "4"}]


@pytest.mark.parametrize("chunks", _WS_FORCED, ids=["default", "many-chunk items"])
@pytest.mark.parametrize("name", ["sr3_tiny", "ddpm_tiny", "hagen_64", "sr3_128"])
def test_unet_forward_persistent_kernel_forced(name, chunks, dev, monkeypatch):
    """The warp-specialised persistent conv kernel (the one the B = 16 benchmark runs on) forced onto the
    small test grids (DSX_WS_MIN_GRID=1): fp32 build within 1e-3 of the golden output, bf16 build by PSNR.
    (ddpm_tiny is 32 x 48: three tiles per row, i.e. the multiply-high divisions of the kernel's start-up with a
    divisor that is not a power of two.)"""
    monkeypatch.setenv("DSX_WS_MIN_GRID", "1")
    for k, v in chunks.items():
        monkeypatch.setenv(k, v)
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x, t = cases.make_unet_inputs(name)
    eng = build_engine(case["cfg"], case["flavour"], sd)
    descs = eng.op_descriptions(*x.shape[:1], *x.shape[2:])
    n_ws = sum("ws" in d.split() for d in descs)
    assert n_ws > 0, "no launch of this plan uses the persistent kernel"
    n_multi = sum(("c2" in d.split() or "c4" in d.split()) for d in descs)
    y = eng.forward(x.to(dev), t.to(dev).float() if case["flavour"] == "sr3" else t.to(dev)).cpu().numpy()
    assert maxabs(y, g["y"]) <= FP32_TOL, maxabs(y, g["y"])
    eng16 = build_engine(case["cfg"], case["flavour"], sd, dtype="bf16")
    y16 = eng16.forward(x.to(dev), t.to(dev).float() if case["flavour"] == "sr3" else t.to(dev)).cpu().numpy()
    p = psnr(g["y"], y16)
    print(f"\n{name}: persistent kernel forced: fp32 max-abs {maxabs(y, g['y']):.3e} ({n_ws} ws launches, {n_multi} with "
          f"several chunks per item in the fp32 plan), bf16 PSNR {p:.1f} dB")
    assert p > 35.0
    # the bounded LDS-counter spins of the loader -> compute hand-off must never have given up
    assert eng.handoff_timeouts() == 0 and eng16.handoff_timeouts() == 0


def test_benchmark_batch_matches_single_image_path(dev):
    """B = 16 of the headline config runs on the persistent kernels (128x128 / 64x128 / 128x64 tiles), B = 1 on
    k_conv_mfma: image 0 of the batch must agree with the single-image forward (same bf16 operands, other tiling)."""
    name = "sr3_128"
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x1, t1 = cases.make_unet_inputs(name)
    gen = torch.Generator().manual_seed(7)
    x = torch.cat([x1, torch.randn((15,) + tuple(x1.shape[1:]), generator=gen)])
    t = torch.cat([t1.float(), 0.05 + 0.95 * torch.rand((15, 1), generator=gen)])
    eng = build_engine(case["cfg"], case["flavour"], sd, dtype="bf16")
    n_ws = sum("ws" in d.split() for d in eng.op_descriptions(16, 128, 128))
    assert n_ws >= 60, n_ws
    y16 = eng.forward(x.to(dev), t.to(dev)).cpu().numpy()
    y1 = eng.forward(x1.to(dev), t1.to(dev).float()).cpu().numpy()
    p = psnr(y1[0], y16[0])
    print(f"\nB=16 (persistent kernels, {n_ws} ws launches) vs B=1 (k_conv_mfma): PSNR {p:.1f} dB; vs fp32 golden {psnr(g['y'][0], y16[0]):.1f} dB")
    assert p > 50.0
    assert psnr(g["y"][0], y16[0]) > 35.0
    assert eng.handoff_timeouts() == 0      # 256-pixel tiles hand over through LDS counters with bounded spins


def test_hosted_groupnorm_finalize_is_bitwise_neutral(dev, monkeypatch):
    """At the benchmark batch the residual 1 x 1 convs run the finalize of their block's second GroupNorm in their compute
    waves' start-up wait (one launch less per block).  It is the same per-(image, group) code on the same partial sums
    as the k_gn_finalize launch it replaces: with DSX_HOST_FIN=0 the forward must be bitwise identical."""
    name = "sr3_128"
    sd, _ = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((16, 6, 128, 128), generator=gen).to(dev)
    t = (0.05 + 0.95 * torch.rand((16, 1), generator=gen)).to(dev)
    for dtype in ("bf16", "f32"):
        eng = build_engine(case["cfg"], case["flavour"], sd, dtype=dtype)
        descs = eng.op_descriptions(16, 128, 128)
        n_host = sum("+gn" in d for d in descs)
        n_fin = sum(d.startswith("gn_finalize") for d in descs)
        assert n_host >= 10, (dtype, n_host)
        y_host = eng.forward(x, t).cpu()
        monkeypatch.setenv("DSX_HOST_FIN", "0")
        eng0 = build_engine(case["cfg"], case["flavour"], sd, dtype=dtype)
        descs0 = eng0.op_descriptions(16, 128, 128)
        assert sum("+gn" in d for d in descs0) == 0
        assert sum(d.startswith("gn_finalize") for d in descs0) == n_fin + n_host
        y_plain = eng0.forward(x, t).cpu()
        monkeypatch.delenv("DSX_HOST_FIN")
        assert torch.equal(y_host, y_plain), (dtype, float((y_host - y_plain).abs().max()))
        print(f"\n{dtype}: {n_host} finalizes hosted by residual convs, {n_fin} launches left; bitwise equal to the unhosted plan")


def test_unet_forward_naive_conv_crosscheck(dev, monkeypatch):
    """The plain direct-conv kernel (DSX_CONV_IMPL=naive) and the MFMA kernel agree."""
    monkeypatch.setenv("DSX_CONV_IMPL", "naive")
    name = "ddpm_tiny"
    sd, g = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    x, t = cases.make_unet_inputs(name)
    eng = build_engine(case["cfg"], case["flavour"], sd)
    y = eng.forward(x.to(dev), t.to(dev)).cpu().numpy()
    assert maxabs(y, g["y"]) <= FP32_TOL


def test_unet_batch_independence_and_determinism(dev):
    """Size-independent properties at the headline config: images of a batch do not
    interact (GroupNorm/attention are per-sample) and reruns are bitwise identical."""
    name = "sr3_128"
    sd, _ = golden_state_dict("unet_" + name)
    case = cases.UNET_CASES[name]
    g = torch.Generator().manual_seed(11)
    x = torch.randn((4, 6, 128, 128), generator=g).to(dev)
    t = (0.1 + 0.9 * torch.rand((4, 1), generator=g)).to(dev)
    eng = build_engine(case["cfg"], "sr3", sd)
    y4 = eng.forward(x, t)
    y4b = eng.forward(x, t)
    assert torch.equal(y4, y4b)
    y1 = eng.forward(x[2:3].contiguous(), t[2:3].contiguous())
    assert maxabs(y1.cpu(), y4[2:3].cpu()) <= 1e-5


# ----------------------------------------------------------------------------- sampling loops
def _sr3_engine_run(eng, sch, cond, draws, dev, use_graph, clip=True, kind="sr3"):
    from diffsplitting_amd import engine
    bufs, gam = engine.gaussian_buffers(sch)
    tab = engine.gaussian_step_table(bufs, gam, kind, clip)
    T = tab.n_steps
    x0 = draws[0].to(dev)
    per_step = draws[1:]
    noise = torch.zeros((T,) + tuple(x0.shape))
    for s, d in enumerate(per_step):
        noise[s] = d
    snaps = engine.gaussian_snapshot_steps(T)
    x, sn = eng.sample_loop(tab, x0.clone(), cond=cond.to(dev), noise=noise.to(dev),
                            snapshot_steps=snaps, use_graph=use_graph)
    torch.cuda.synchronize()
    return x.cpu(), sn.cpu()


@pytest.mark.parametrize("sched,use_graph", [("lin_8", False), ("lin_8", True), ("lin_25", True)])
def test_sr3_loop(sched, use_graph, dev):
    sd, g = golden_state_dict("loop_sr3_" + sched)
    case = cases.UNET_CASES["sr3_tiny"]
    sch = cases.SCHEDULES[sched]
    cond = cases.make_cond("sr3_loop")
    rec = DrawRecorder(cases.LOOP_SEED)
    osd = {"denoise_fn." + k: v for k, v in sd.items()}
    ret, full = samplers.sr3_p_sample_loop(osd, case["cfg"], samplers.gaussian_schedule(sch), cond, randn=rec,
                                           continous=True, return_full=True)
    eng = build_engine(case["cfg"], "sr3", sd)
    x, sn = _sr3_engine_run(eng, sch, cond, rec.draws, dev, use_graph)
    assert maxabs(x, full) <= FP32_TOL, maxabs(x, full)
    # continuous stack = [cond | snapshots...] (diffusion.py:195-199)
    stack = torch.cat([cond] + [s for s in sn], dim=0)
    assert stack.shape == ret.shape
    assert maxabs(stack, ret) <= FP32_TOL
    print(f"\nsr3 {sched} graph={use_graph}: max|hip-oracle| = {maxabs(x, full):.3e}")


def test_sr3_loop_seeded_matches_golden(dev):
    """Same torch seed as the golden run -> the injected draws equal the reference's own."""
    sd, g = golden_state_dict("loop_sr3_lin_8")
    case = cases.UNET_CASES["sr3_tiny"]
    sch = cases.SCHEDULES["lin_8"]
    cond = cases.make_cond("sr3_loop")
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(2, 3, 32, 32) for _ in range(8)]  # init + T-1 steps, reference draw order
    eng = build_engine(case["cfg"], "sr3", sd)
    x, sn = _sr3_engine_run(eng, sch, cond, draws, dev, True)
    stack = torch.cat([cond] + [s for s in sn], dim=0).numpy()
    assert maxabs(stack, g["ret"]) <= FP32_TOL
    assert maxabs(x[-1].numpy(), g["last"]) <= FP32_TOL  # non-continuous return = last batch element (Q1)


def test_ddpm_loop(dev):
    sd, g = golden_state_dict("loop_ddpm_lin_8")
    cfg = cases.DDPM_COND_CASE["cfg"]
    sch = cases.SCHEDULES["lin_8"]
    cond = cases.make_cond("ddpm_loop")
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(2, 1, 32, 32) for _ in range(9)]  # init + T draws (drawn even at t == 0)
    eng = build_engine(cfg, "ddpm", sd)
    x, sn = _sr3_engine_run(eng, sch, cond, draws, dev, True, kind="ddpm")
    stack = torch.cat([cond] + [s for s in sn], dim=0).numpy()
    assert maxabs(stack, g["ret"]) <= FP32_TOL, maxabs(stack, g["ret"])


def _indi_engine_run(eng, x_in, n, t0, out_channel, draws, dev, use_graph=True, e=0.01, stream=None):
    from diffsplitting_amd import engine
    tab = engine.indi_step_table(n, t0, e)
    xin = torch.cat([x_in] * out_channel, dim=1)
    x0 = xin + draws[0] * (e * torch.Tensor([t0]))  # indi.py:80-82
    noise = torch.stack(draws[1:1 + n])
    x, sn = eng.sample_loop(tab, x0.to(dev), noise=noise.to(dev), snapshot_steps=engine.indi_snapshot_steps(n),
                            use_graph=use_graph, stream=stream)
    return x0, x, sn


@pytest.mark.parametrize("n,t0", [(1, 1.0), (3, 1.0), (10, 1.0), (20, 1.0), (4, 0.6)])
def test_indi_loop(n, t0, dev):
    sd, g = golden_state_dict(f"loop_indi_n{n}_t{t0}")
    case = cases.UNET_CASES["ddpm_tiny"]
    x_in = cases.make_cond("indi_loop")
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(3, 2, 32, 48) for _ in range(n + 1)]
    eng = build_engine(case["cfg"], "ddpm", sd)
    x0, x, sn = _indi_engine_run(eng, x_in, n, t0, 2, draws, dev)
    torch.cuda.synchronize()
    stack = torch.cat([x0] + [s for s in sn.cpu()], dim=0).numpy()
    assert stack.shape == g["ret"].shape
    assert maxabs(stack, g["ret"]) <= FP32_TOL, maxabs(stack, g["ret"])
    assert maxabs(x.cpu()[-1:].numpy(), g["last"]) <= FP32_TOL


@pytest.mark.parametrize("n", cases.C1_STEPS)
def test_c1_cifar_indi_loop(n, dev):
    """BASELINE C1 (config/splitting_cifar10_indi.json:43-44,65,71; indi.py:71-95): UNet 6 -> 6, inner 16, mults
    [1,2,4,8], GN16, x_in (4, 1, 32, 32) replicated x6, n = 20 and n = 100 (no drift assert in the engine), against the
    reference-generated fixture and the oracle on the same draws."""
    sd, g = golden_state_dict(f"loop_c1_cifar_n{n}")
    cfg = cases.C1_CASE["cfg"]
    x_in = cases.make_cond("c1_cifar")
    torch.manual_seed(cases.LOOP_SEED)
    draws = [torch.randn(4, 6, 32, 32) for _ in range(n + 1)]
    eng = build_engine(cfg, "ddpm", sd)
    x0, x, sn = _indi_engine_run(eng, x_in, n, 1.0, 6, draws, dev)
    torch.cuda.synchronize()
    blocks = torch.stack([x0] + [s for s in sn.cpu()], dim=0).numpy()
    assert blocks.shape[0] == int(g["nblocks"])
    err = maxabs(blocks[cases.c1_keep(blocks.shape[0])], g["blocks"])
    print(f"C1 cifar InDI n={n}: max|hip - reference| = {err:.3e}")
    assert err <= FP32_TOL, err
    assert maxabs(x.cpu()[-1:].numpy(), g["last"]) <= FP32_TOL
    rec = iter(draws)
    osd = {"denoise_fn." + k: v for k, v in sd.items()}
    _, ref = samplers.indi_inference(osd, cfg, x_in, n, 6, randn=lambda shape: next(rec), return_full=True)
    assert maxabs(x.cpu(), ref) <= FP32_TOL


def test_joint_indi_two_streams(dev):
    """JointIndi (joint_indi.py:131-135): the two InDI loops run concurrently on two HIP streams."""
    sd, g = golden_state_dict("loop_joint_n3")
    case = cases.UNET_CASES["joint_32"]
    x_in = cases.make_cond("joint_loop")
    torch.manual_seed(cases.LOOP_SEED)
    d1 = [torch.randn(2, 1, 32, 32) for _ in range(4)]  # all of indi1's draws first (Q4)
    d2 = [torch.randn(2, 1, 32, 32) for _ in range(4)]
    e1 = build_engine(case["cfg"], "ddpm", sd, prefix="indi1.denoise_fn.")
    e2 = build_engine(case["cfg"], "ddpm", sd, prefix="indi2.denoise_fn.")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a0, a, asn = _indi_engine_run(e1, x_in, 3, 0.5, 1, d1, dev, stream=s1)
    b0, b, bsn = _indi_engine_run(e2, x_in, 3, 0.5, 1, d2, dev, stream=s2)
    torch.cuda.synchronize()
    ch1 = torch.cat([a0] + [s for s in asn.cpu()], dim=0)
    ch2 = torch.cat([b0] + [s for s in bsn.cpu()], dim=0)
    stack = torch.cat([ch1, ch2], dim=1).numpy()
    assert maxabs(stack, g["ret"]) <= FP32_TOL, maxabs(stack, g["ret"])


def test_sr3_2000_steps_tiny(dev):
    """The full 2000-step schedule of sr_sr3_16_128 on the tiny UNet: drift stays under
    1e-3 with injected noise (re-association noise ~2e-6 over 2000 steps)."""
    from tests.gpu_util import oracle_sr3_loop_tiny
    sd, case, sch, cond, draws, full = oracle_sr3_loop_tiny("sr3_2000", (1, 3, 16, 16))
    eng = build_engine(case["cfg"], "sr3", sd)
    x, _ = _sr3_engine_run(eng, sch, cond, draws, dev, True)
    print(f"\n2000 steps: max|hip-oracle| = {maxabs(x, full):.3e}")
    assert maxabs(x, full) <= FP32_TOL


def test_device_rng_statistics(dev):
    from diffsplitting_amd import engine
    z = engine.randn((1 << 20,), seed=5).cpu().numpy().astype(np.float64)
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1.0) < 5e-3
    assert abs(np.mean(z ** 3)) < 2e-2 and abs(np.mean(z ** 4) - 3.0) < 5e-2
    z2 = engine.randn((1 << 20,), seed=5).cpu().numpy()
    assert np.array_equal(z.astype(np.float32), z2)              # reproducible
    z3 = engine.randn((1 << 20,), seed=6).cpu().numpy()
    assert abs(np.corrcoef(z[:100000], z3[:100000])[0, 1]) < 2e-2  # seeds decorrelate


def test_perf_mode_loop_runs_and_is_seeded(dev):
    """Device-noise mode: same seed -> identical images, different seed -> different."""
    from diffsplitting_amd import engine
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    case = cases.UNET_CASES["sr3_tiny"]
    bufs, gam = engine.gaussian_buffers(cases.SCHEDULES["lin_25"])
    tab = engine.gaussian_step_table(bufs, gam, "sr3", True)
    cond = cases.make_cond("sr3_loop").to(dev)
    eng = build_engine(case["cfg"], "sr3", sd)
    outs = []
    for seed in (1, 1, 2):
        x0 = engine.randn((2, 3, 32, 32), seed=seed)
        x, _ = eng.sample_loop(tab, x0, cond=cond, seed=seed)
        torch.cuda.synchronize()
        outs.append(x.cpu())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert torch.isfinite(outs[0]).all()


# ----------------------------------------------------------------------------- time predictor
def test_time_predictor(dev):
    from diffsplitting_amd import engine, _lib
    import ctypes as C
    sd, g = golden_state_dict("time_predictor")
    cfg = cases.TIME_PRED_CFG
    x = cases.make_cond("time_pred")
    eng = build_engine(cfg, "ddpm", sd, prefix="unet.", with_time_emb=False)
    ex = eng.executor(3, 32, 32)
    w = sd["foreground_mask.layer.weight"].contiguous()
    b = sd["foreground_mask.layer.bias"].contiguous()
    _lib.check(_lib.lib.dsx_time_predictor_set_mask(ex, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr())))
    xd = x.to(dev).contiguous()
    out = torch.empty(3, device=dev)
    _lib.check(_lib.lib.dsx_time_predictor_forward(ex, C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    ref = time_predictor_forward(sd, cfg, x).numpy()
    assert maxabs(out.cpu().numpy(), g["t"]) <= FP32_TOL and maxabs(out.cpu().numpy(), ref) <= FP32_TOL


# ----------------------------------------------------------------------------- tiling
@pytest.mark.parametrize("name,data_shape,grid_shape,patch_shape", cases.TILE_CASES)
def test_gather_and_stitch(name, data_shape, grid_shape, patch_shape, dev):
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan(data_shape, grid_shape, patch_shape)
    oplan = tiling.TilePlan(data_shape, grid_shape, patch_shape)
    n = plan.total
    rng = np.random.default_rng(1)
    C = 2
    if name == "hagen_490":
        data_shape = (2, 2048, 2048)  # same plan geometry per frame; keep the CPU check quick
        plan = TilePlan(data_shape, grid_shape, patch_shape)
        oplan = tiling.TilePlan(data_shape, grid_shape, patch_shape)
        n = plan.total
        assert n == 98
    frames = rng.standard_normal(tuple(data_shape) + (C,)).astype(np.float32)
    # gather each channel's tiles on the device, compare with the oracle crop
    tiles = torch.stack([plan.gather(torch.from_numpy(np.ascontiguousarray(frames[..., c])).to(dev))
                         for c in range(C)], dim=1)          # (n, C, ph, pw)
    ref_tiles = np.stack([tiling.extract_patch(frames, oplan, i) for i in range(n)])
    assert np.array_equal(tiles.cpu().numpy(), ref_tiles)
    out = plan.stitch(tiles)
    assert np.array_equal(out.cpu().numpy(), tiling.stitch(ref_tiles, oplan))
    assert np.array_equal(out.cpu().numpy(), frames)          # encode -> decode round trip


def test_stitch_known_answer_on_device(dev):
    """tests/test_tiling_setup.py of the reference, through the HIP gather/stitch (exact)."""
    from diffsplitting_amd.data.tiling import TilePlan
    n, H, W, C = 5, 512, 512, 2
    data = np.arange(n * H * W * C).reshape(n, H, W, C).astype(np.float32)  # < 2^24: exact in fp32
    plan = TilePlan((n, H, W), (1, 128, 128), (1, 256, 256))
    assert plan.total == 45
    tiles = torch.stack([plan.gather(torch.from_numpy(np.ascontiguousarray(data[..., c])).to(dev))
                         for c in range(C)], dim=1)
    assert np.array_equal(plan.stitch(tiles).cpu().numpy(), data)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("name,data_shape,grid_shape,patch_shape", [c for c in cases.TILE_CASES if c[0] != "hagen_490"])
def test_cropped_exchange_kernels(name, data_shape, grid_shape, patch_shape, world, dev):
    """The multi-rank exchange of CROPPED tiles (tile_stitcher.py:38-56 before the collective), every rank's
    part played on the one GPU: pack each shard's valid regions batch by batch (device tables indexed by tile id), lay
    the runs side by side as the all-gather would, paste from the packed layout -> bit-exact equal to the one-rank
    stitch and to the oracle; the fused RangeInvariantPsnr sums equal the whole-tile path's."""
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan(data_shape, grid_shape, patch_shape)
    oplan = tiling.TilePlan(data_shape, grid_shape, patch_shape)
    C = 2
    rng = np.random.default_rng(7)
    pred = rng.standard_normal((plan.total, C, patch_shape[1], patch_shape[2])).astype(np.float32)
    gt = rng.standard_normal(tuple(data_shape) + (C,)).astype(np.float32)
    pred_d, gt_d = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    off, runs = plan.pack_layout(world)
    ooff, oruns = tiling.pack_layout(oplan, world)
    assert np.array_equal(off, ooff) and np.array_equal(runs, oruns)
    stride = plan.rank_stride(world, C)
    full = torch.zeros((world, max(stride, 1)), dtype=torch.float32, device=dev)
    for r in range(world):
        ids = list(range(r, plan.total, world))
        for i in range(0, len(ids), 3):                                # batches of 3 tiles into the same run
            chunk = ids[i:i + 3]
            plan.pack(pred_d[chunk], world, chunk[0], full[r])
        ref_run = tiling.pack_rank(pred[ids], ids, oplan, off, max(stride, 1))
        assert np.array_equal(full[r].cpu().numpy(), ref_run)
    canvas, ps = plan.paste_packed(full, C, world, gt=gt_d)
    whole, ps_whole = plan.stitch_with_psnr(pred_d, gt_d)
    assert torch.equal(canvas, whole) and torch.equal(ps, ps_whole)
    assert np.array_equal(canvas.cpu().numpy(), tiling.stitch(pred, oplan))
    assert torch.equal(plan.paste_packed(full, C, world), whole)


def test_tile_id_lists_that_are_not_sequences(dev):
    """Arbitrary id lists take the per-call upload forms (dsx_tiles_gather / dsx_stitch), sequences the plan's device
    tables: same bytes either way."""
    from diffsplitting_amd.data.tiling import TilePlan, as_sequence
    plan = TilePlan((2, 96, 128), (1, 32, 32), (1, 64, 64))
    frames = torch.randn(2, 96, 128, device=dev)
    every = plan.gather(frames)
    ids = [5, 0, 7, 3]
    assert as_sequence(ids) is None and as_sequence([1, 4, 7]) == (1, 3, 3) and as_sequence([]) == (0, 1, 0)
    assert torch.equal(plan.gather(frames, ids), every[ids])
    assert torch.equal(plan.gather(frames, [1, 4, 7]), every[[1, 4, 7]])
    tiles = every.unsqueeze(1).contiguous()
    a = plan.stitch(tiles[ids], ids)
    b = plan.stitch(tiles[[0, 3, 5, 7]], [0, 3, 5, 7])
    assert torch.equal(a, b)
    c = plan.stitch(tiles[[1, 4, 7]], [1, 4, 7], canvas=plan.stitch(tiles[[0, 3, 6]], [0, 3, 6]))
    d = plan.stitch(tiles[[0, 1, 3, 4, 6, 7]], [0, 1, 3, 4, 6, 7])
    assert torch.equal(c, d)


def test_single_step_entry_points_equal_the_loop(dev):
    """dsx_indi_step / dsx_sr3_step (one reverse step per call, indi.py:62-69, sr3 diffusion.py:141-175) step
    through the same schedule as dsx_sample_loop with the same injected draws: bitwise the same final state."""
    import ctypes as C
    from diffsplitting_amd import _lib, engine
    lib, check = _lib.lib, _lib.check
    # InDI
    sd, _ = golden_state_dict("loop_indi_n3_t1.0")
    case = cases.UNET_CASES["ddpm_tiny"]
    eng = build_engine(case["cfg"], "ddpm", sd)
    n = 3
    tab = engine.indi_step_table(n, 1.0)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(3, 2, 32, 48, generator=g).to(dev)
    noise = torch.randn(n, 3, 2, 32, 48, generator=g).to(dev)
    ref, _ = eng.sample_loop(tab, x0.clone(), noise=noise, use_graph=False)
    ex = eng.executor(3, 32, 48)
    x = x0.clone()
    for s in range(n):
        check(lib.dsx_indi_step(ex, float(tab.tcond[s]), float(tab.c1[s]), float(tab.c2[s]), float(tab.sigma[s]),
                                C.c_void_p(x.data_ptr()), C.c_void_p(noise[s:s + 1].contiguous().data_ptr()), 0, None))
    torch.cuda.synchronize()
    assert torch.equal(x, ref)
    # SR3
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    case = cases.UNET_CASES["sr3_tiny"]
    eng = build_engine(case["cfg"], "sr3", sd)
    bufs, gam = engine.gaussian_buffers(cases.SCHEDULES["lin_8"])
    tab = engine.gaussian_step_table(bufs, gam, "sr3", clip_denoised=True)
    T = tab.n_steps
    cond = torch.randn(2, 3, 32, 32, generator=g).to(dev)
    x0 = torch.randn(2, 3, 32, 32, generator=g).to(dev)
    noise = torch.randn(T, 2, 3, 32, 32, generator=g).to(dev)
    ref, _ = eng.sample_loop(tab, x0.clone(), cond=cond, noise=noise, use_graph=False)
    ex = eng.executor(2, 32, 32, 3)
    x = x0.clone()
    for s in range(T):
        check(lib.dsx_sr3_step(ex, float(tab.tcond[s]), float(tab.a[s]), float(tab.b[s]), float(tab.c1[s]), float(tab.c2[s]),
                               float(tab.sigma[s]), 1, C.c_void_p(cond.data_ptr()), C.c_void_p(x.data_ptr()),
                               C.c_void_p(noise[s:s + 1].contiguous().data_ptr()), 0, None))
    torch.cuda.synchronize()
    assert torch.equal(x, ref)
