"""Every capped launch once past its cap, on the MI355X (`-m gpu`): the second trip of the grid-stride loops, with a
sample boundary and a ragged tail inside it, against the references that the small-shape tests use.

The caps.  Per launcher: its cap, the size from which the loop repeats, and the test that crosses it.

grid_for (dsx_kernels.h): 4096 workgroups of 256 threads.
  * k_randn, k_randn_samples (four elements per thread): 2^22 elements, per row.  test_randn_* here.
  * launch_groups4 -- k_q_sample, k_step, k_step_streams, k_interp_start, k_update (four elements per thread): 2^22
    elements.  test_q_sample_*, test_step_*, test_interp_start_* and test_loop_update_* here.
  * k_tiles_randn (four pixels per thread): 2^22 pixels per tile.  Not crossed and left out: no plan has such tiles.
  * k_moments_update, k_moments_finish: 2^20 elements.  test_moments_* here; elsewhere the largest count is 4097
    (tests/test_gpu_input_stack.py).
  * k_msssim_pool: 2^20 pooled pixels, all planes together.  test_msssim_pool_* here, in the fp32 instantiation
    (scale 0 -> 1); elsewhere at most 539 700 (tests/test_gpu_msssim.py).  The double instantiation (scale s -> s + 1,
    the same loop) would need four times the planes and is not crossed.
  * k_nchw_to_nhwc, k_nhwc_to_nchw: 2^20 elements.  The UNet input of test_c4_unet_512 (6 x 512 x 512,
    tests/test_gpu_fullsize.py) crosses the first; test_loop_update_* here crosses both on a state of 2^22 elements.
tile_grid_x (dsx_tiles.hip): 64 workgroups of 256 threads, 16 384 elements per tile.
  * k_tiles_gather, k_stitch: crossed by the 256 x 256 patches of tests/test_gpu_parity.py.
  * k_tiles_gather_norm, _norm_planes, _mix, _mix_items, k_tiles_gather_canvas, k_tiles_pack: test_tiles_* here;
    elsewhere the patches hold at most 64 x 64 pixels (the whole-frame tiles of 128 x 128 in tests/test_gpu_boundary.py
    fill the first trip exactly).
  * k_stitch_psnr takes its grid from the caller, k_blend and k_tiles_gather_input are not capped: left out.
select_blocks (dsx_select.hip): 2048 workgroups, 2^21 elements in the 16-byte form and 2^19 in the scalar one.  Not
  crossed by any test: the largest count is 3 x 211 x 223 (tests/test_gpu_select.py).
lpips_minmax_blocks (dsx_lpips.hip): 1024 workgroups, 262 144 pixels.  Not crossed by any test: the largest stack has
  3 x 160 x 192 pixels (tests/test_gpu_lpips.py).
launch_splitk_reduce (dsx_ops.hip): 2048 workgroups, 524 288 outputs.  Crossed by test_c4_unet_512, against the oracle:
  its split-K layers reduce 1024 x 1024 and 4096 x 256 outputs (the launches without fused statistics take the capped
  kernel).

The normal stream beyond its first 2^22 elements is compared with tests/normal_ref.py (the bound: see
tests/test_gpu_normal_stream.py); Philox counter word 1 (block index >> 32) would need 2^34 elements and stays
untested on the device.  Every launch here is a valid one.

Wall times on the MI355X machine (pytest's call durations; every case prints its own): the loop with default noise and
its chain of single steps 0.50 s (the loop of two steps 0.27 s), with sample streams 0.04 s; MS-SSIM 0.35 s; randn
against the restatement 0.23 s; q_sample 0.13 s and 0.08 s; the steps 0.09 s and 0.02 s; moments 0.08 s; every other
case 0.02 s or less.  The module took 6.3 s in two runs, imports and the one engine build included.  No case was left
out for time.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import cases, tiling
from tests import blend_ref, cifar_files, mixed_ref, mixed_util, msssim_ref, nets
from tests import normal_ref as nr
from tests.bits import same_bits
from tests.gpu_util import build_engine
from tests.steps_util import ref_interp, ref_q, ref_step
from tests.tiled_util import numpy_item, welford
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CAP = 1 << 22                             # elements of the first trip of a four-per-thread grid_for launch
SEED, SUBSEQ = 7 | 5 << 40, (3 << 24) | 1 | 1 << 60


def _timed(name, t0):
    torch.cuda.synchronize()
    print(f"\n{name}: {time.perf_counter() - t0:.2f} s")


# ----------------------------------------------------------------------------- k_randn, k_randn_samples
def test_randn_past_the_grid_cap_is_the_restated_stream():
    """n = 2^22 + 4099: 1025 Philox blocks in the second trip, the last one cut after three elements."""
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    n = CAP + 4099
    got = engine.randn((n,), SEED, subsequence=SUBSEQ).cpu().numpy()
    z, radius = nr.stream(SEED, SUBSEQ, n)
    worst, i = nr.worst_ratio(got, z, radius)
    tail, j = nr.worst_ratio(got[CAP:], z[CAP:], radius[CAP:])
    print(f"\nrandn {n}: max |got - z| / (2^-24 radius) = {worst:.3f} at {i}; beyond 2^22: {tail:.3f} at {CAP + j} "
          f"(K = {nr.K_DEVICE})")
    assert tail <= nr.K_DEVICE, (tail, CAP + j)                      # the second trip on its own
    assert worst <= nr.K_DEVICE, (worst, i)
    _timed("randn past the cap", t0)


@pytest.mark.parametrize("chw", [CAP + 4099, CAP + 4096], ids=["scalar", "vec16"])
def test_randn_samples_rows_past_the_grid_cap(chw):
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    ids, draw = [5, 1 << 33], 7
    got = engine.randn_samples((2, chw), SEED, ids, draw)
    for b, sid in enumerate(ids):
        assert same_bits(got[b], engine.randn((chw,), SEED, subsequence=nr.sample_subseq(sid, draw))), sid
        # both sides are fresh allocations: were the second trip missing in both, equal leftovers would compare equal.
        # The 4096+ elements beyond 2^22 are normals: their spread is 1 +- 0.011 (one standard error), 9 of them allowed
        assert 0.9 < float(got[b, CAP:].std()) < 1.1, sid
    _timed(f"randn_samples 2 x {chw}", t0)


# ----------------------------------------------------------------------------- the pointwise kernels of launch_groups4
# (6, 3, 500, 560): H*W % 4 == 0, the 16-byte path; 5 * C*H*W = 4 200 000 > 2^22: the boundary between samples 4 and 5 lies in
# the second trip.  (6, 3, 499, 561): H*W odd, the scalar path; 5 * C*H*W = 4 199 085 and n % 4 == 2: a cut last group.
SHAPES = [(6, 3, 500, 560), (6, 3, 499, 561)]
# per-sample coefficients, all different; sample 4 has sigma = 0, sample 5 has not
COEF = dict(a=torch.tensor([1.0371, 2.2360679, 1.0000501, 1.5, 1.118034, 1.25]),
            b=torch.tensor([0.2748, 2.0, 0.0100123, 1.118034, 0.5, 0.75]),
            c1=torch.tensor([0.75623951, 0.31, 0.9990234, 0.5, 0.123456, 0.87]),
            c2=torch.tensor([0.1, 0.654321, 0.0123, 0.45, 0.8, 0.11]),
            sigma=torch.tensor([0.37, 0.0, 0.81, 0.25, 0.0, 0.6]))
_OPERANDS = {}


def _operands(shape):
    """(x, net, z, z') on the host and the same on the device, made once per shape and never written to"""
    if shape not in _OPERANDS:
        assert shape[0] == 6 and 5 * shape[1] * shape[2] * shape[3] > CAP
        host = [nets.rand(shape, 1), 0.7 * nets.rand(shape, 2), nets.rand(shape, 3), nets.rand(shape, 4)]
        _OPERANDS[shape] = (host, [t.cuda() for t in host])
    return _OPERANDS[shape]


def _dev(co):
    return {k: v.cuda() for k, v in co.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=["vec16", "scalar"])
def test_q_sample_past_the_grid_cap(shape):
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    (x0, _, z, _), (x0d, _, zd, _) = _operands(shape)
    c0, c1, c2 = COEF["c1"], COEF["b"], COEF["c2"]
    xe = x0[:, :1].contiguous() * 0.5 + 0.25                          # Ce = 1, read at channel c % 1
    out, z_used = engine.q_sample(x0d, c0.cuda(), c2.cuda(), z=zd)
    assert same_bits(out, ref_q(x0, c0, c2, z)) and same_bits(z_used, zd)
    out, _ = engine.q_sample(x0d, c0.cuda(), c2.cuda(), xe=xe.cuda(), c1=c1.cuda(), z=zd)
    assert same_bits(out, ref_q(x0, c0, c2, z, xe, c1))
    # drawn: the normals are dsx_randn's at the flat index, and the sum is the injected one
    out, drawn = engine.q_sample(x0d, c0.cuda(), c2.cuda(), seed=SEED, subsequence=SUBSEQ, want_z=True)
    assert same_bits(drawn, engine.randn(shape, SEED, SUBSEQ))
    assert same_bits(out, ref_q(x0, c0, c2, drawn.cpu()))
    _timed(f"q_sample {shape}", t0)


def _step(shape, co, **kw):
    from diffsplitting_amd import engine
    _, (xd, netd, _, _) = _operands(shape)
    d = _dev(co)
    outs = [torch.full(shape, float("nan"), device="cuda") for _ in range(3)]
    engine.posterior_step(xd, netd, d["c1"], d["c2"], d["sigma"], a=d["a"], b=d["b"], predict_eps=True, clip=True,
                          x_recon_out=outs[0], mean_out=outs[1], x_out=outs[2], **kw)
    return outs


def _same3(got, ref):
    return all(same_bits(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("shape", SHAPES, ids=["vec16", "scalar"])
def test_step_past_the_grid_cap(shape):
    """k_step: injected and drawn normals, one draw per sample and sample 0's for all (`repeat`)."""
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    (x, net, z, _), (_, _, zd, _) = _operands(shape)
    ref = ref_step(x, net, COEF, z, 1, 1)
    assert bool((ref[0][5].abs() == 1).any())                         # the clamp is exercised beyond the boundary
    assert same_bits(ref[2][4], ref[1][4]) and not same_bits(ref[2][5], ref[1][5])     # sigma 0: the mean; else not
    assert _same3(_step(shape, COEF, z=zd), ref)
    z1 = z[:1].contiguous()
    assert _same3(_step(shape, COEF, z=z1.cuda(), repeat_noise=True), ref_step(x, net, COEF, z1, 1, 1, repeat=True))
    drawn = engine.randn(shape, SEED, SUBSEQ)
    assert _same3(_step(shape, COEF, seed=SEED, subsequence=SUBSEQ), ref_step(x, net, COEF, drawn.cpu(), 1, 1))
    first = engine.randn((1,) + shape[1:], SEED, SUBSEQ)
    assert _same3(_step(shape, COEF, seed=SEED, subsequence=SUBSEQ, repeat_noise=True),
                  ref_step(x, net, COEF, first.cpu(), 1, 1, repeat=True))
    _timed(f"posterior_step {shape}", t0)


@pytest.mark.parametrize("shape", SHAPES, ids=["vec16", "scalar"])
def test_step_streams_past_the_grid_cap(shape):
    """k_step_streams: sample b draws its own stream from element 0; samples 4 and 5 begin beyond 2^22."""
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    (x, net, _, _), _ = _operands(shape)
    ids, draw = [3, 1 << 33, 2 ** 40 - 1, 0, 77, 1 << 20], 9
    co = dict(COEF, sigma=torch.tensor([0.37, 0.0, 0.81, 0.25, 0.6, 0.0]))     # this time sample 5 without noise
    z = engine.randn_samples(shape, SEED, ids, draw)
    assert _same3(_step(shape, co, seed=SEED, sample_ids=ids, draw=draw), ref_step(x, net, co, z.cpu(), 1, 1))
    _timed(f"posterior_step with sample streams {shape}", t0)


@pytest.mark.parametrize("shape", SHAPES, ids=["vec16", "scalar"])
def test_interp_start_past_the_grid_cap(shape):
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    (x1, x2, z1, z2), (x1d, x2d, z1d, z2d) = _operands(shape)
    a0, s0, lam = COEF["c1"], COEF["c2"], 0.3
    out = engine.interp_start(x1d, x2d, a0.cuda(), s0.cuda(), lam, z1=z1d, z2=z2d)
    assert same_bits(out, ref_interp(x1, x2, a0, s0, lam, z1, z2))
    out = engine.interp_start(x1d, x2d, a0.cuda(), s0.cuda(), lam, seed=SEED, subsequence=SUBSEQ)
    d1, d2 = engine.randn(shape, SEED, SUBSEQ), engine.randn(shape, SEED, SUBSEQ + 1)
    assert same_bits(out, ref_interp(x1, x2, a0, s0, lam, d1.cpu(), d2.cpu()))
    _timed(f"interp_start {shape}", t0)


# ----------------------------------------------------------------------------- k_update: the loop against single steps
# The golden UNet ddpm_tiny on its golden map, 32 x 48 (attention over 96 tokens, as in its own tests), 1368 samples of
# C*H*W = 3072: 4 202 496 state elements, samples 1366 and 1367 whole in the second trip.  One schedule per sample;
# sample 1366 has sigma = 0 at both steps, every other sample at the second.  The loop (k_update on the NHWC state, both
# layout conversions of the state) against T = 2 x (dsx_unet_forward, dsx_posterior_step on the NCHW tensor).
LOOP_B, LOOP_T = 1368, 2


_LOOP_ENGINE = []


def _loop_case():
    from diffsplitting_amd import engine
    if not _LOOP_ENGINE:                                               # one engine and one executor for both tests
        sd, _ = golden_state_dict("loop_indi_n3_t1.0")
        _LOOP_ENGINE.append(build_engine(cases.UNET_CASES["ddpm_tiny"]["cfg"], "ddpm", sd))
    eng = _LOOP_ENGINE[0]
    shape = (LOOP_B, 2, 32, 48)
    assert (LOOP_B - 2) * 3072 > CAP
    rng = np.random.default_rng(5)
    col = lambda lo, hi: rng.uniform(lo, hi, (LOOP_T, LOOP_B)).astype(np.float32)
    cols = dict(tcond=col(0.1, 1.0), a=col(1.0, 1.3), b=col(0.05, 0.6), c1=col(0.2, 0.9), c2=col(0.05, 0.6), sigma=col(0.1, 0.8))
    cols["sigma"][1, :] = 0
    cols["sigma"][:, LOOP_B - 2] = 0
    tab = engine.StepTableHost(cols["tcond"], cols["c1"], cols["c2"], cols["sigma"], a=cols["a"], b=cols["b"],
                               predict_eps=True, clip=True, per_sample=LOOP_B)
    return eng, tab, cols, shape, nets.rand(shape, 70).cuda()


def _chain(eng, cols, x, noise):
    """T single steps on the NCHW tensor; noise(s) -> the keywords that name step s's draws"""
    from diffsplitting_amd import engine
    dev = lambda k, s: torch.from_numpy(cols[k][s]).cuda()
    for s in range(LOOP_T):
        net = eng.forward(x, time=torch.from_numpy(cols["tcond"][s]))
        x = engine.posterior_step(x, net, dev("c1", s), dev("c2", s), dev("sigma", s), a=dev("a", s), b=dev("b", s),
                                  predict_eps=True, clip=True, x_out=torch.empty_like(x), **noise(s))[2]
    return x


def test_loop_update_past_the_grid_cap_default_noise():
    """Default noise: step s draws the stream (seed, s + 1) at the flat NHWC index.  torch.equal: the loop adds z * 0
    where the single step adds nothing, a difference in the sign of a zero at most."""
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    eng, tab, cols, shape, x0 = _loop_case()
    B, Cn, H, W = shape
    got, _ = eng.sample_loop(tab, x0.clone(), seed=SEED)
    _timed(f"loop of {LOOP_T} steps at {shape}", t0)
    nhwc = lambda s: engine.randn((B, H, W, Cn), SEED, s + 1).permute(0, 3, 1, 2).contiguous()
    ref = _chain(eng, cols, x0.clone(), lambda s: dict(z=nhwc(s)))
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, x0)
    assert torch.equal(got, ref)
    assert torch.equal(got[-2:], ref[-2:]) and not torch.equal(got[-1], got[-2])         # the second trip on its own
    _timed("loop and chain", t0)


def test_loop_update_past_the_grid_cap_sample_streams():
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    eng, tab, cols, shape, x0 = _loop_case()
    ids = [(b * 2654435761) % (1 << 40) for b in range(LOOP_B)]
    got, _ = eng.sample_loop(tab, x0.clone(), seed=SEED, sample_ids=ids)
    _timed(f"stream loop of {LOOP_T} steps at {shape}", t0)
    ref = _chain(eng, cols, x0.clone(), lambda s: dict(seed=SEED, sample_ids=ids, draw=s + 1))
    assert bool(torch.isfinite(got).all())
    assert same_bits(got, ref)
    _timed("stream loop and chain", t0)


# ----------------------------------------------------------------------------- k_moments_update / k_moments_finish
def test_moments_past_the_grid_cap():
    """count = 2^20 + 300 (the kernels take one element per thread): bitwise the float64 recurrence."""
    from diffsplitting_amd import engine
    t0 = time.perf_counter()
    count, n = (1 << 20) + 300, 3
    rng = np.random.default_rng(31)
    xs = [(1000 + 1e-2 * rng.standard_normal(count)).astype(np.float32) for _ in range(n)]
    mean = m2 = None
    for r, x in enumerate(xs):
        mean, m2 = engine.moments_update(torch.from_numpy(x).cuda(), mean, m2, r)
    got_mean, got_std = engine.moments_finish(mean, m2, n)
    want_mean, want_std = welford(xs)
    assert same_bits(got_mean.cpu(), torch.from_numpy(want_mean)) and same_bits(got_std.cpu(), torch.from_numpy(want_std))
    assert bool((got_std[1 << 20:] > 0).all())
    _timed("moments", t0)


# ----------------------------------------------------------------------------- k_msssim_pool
def test_msssim_pool_past_the_grid_cap():
    """69 planes of 250 x 250: 125 x 125 pooled pixels each, 1 078 125 in all; plane 67 straddles 2^20, plane 68 lies
    beyond it.  Two scales, so that the pooled planes are read; the workspace is poisoned, so that a pooled pixel that
    is not written shows.  Per-scale means within the tolerance of tests/test_gpu_msssim.py."""
    from diffsplitting_amd.core import metrics
    from diffsplitting_amd._lib import check, lib
    t0 = time.perf_counter()
    shape, L, w = (23, 3, 250, 250), 3.7, (0.5, 0.5)
    t, p = msssim_ref.structured_pair(shape, 11)
    assert 67 * 125 * 125 < (1 << 20) < 68 * 125 * 125
    need = check(lib.dsx_msssim_workspace(250, 250, 2)) * 69
    poisoned = torch.full((need // 8,), float("nan"), dtype=torch.float64, device="cuda")
    means = metrics._msssim_means(torch.tensor(p).cuda(), torch.tensor(t).cuda(), 2, False, L, workspace=poisoned)
    assert means.shape == (23, 3, 2, 2) and np.isfinite(means).all()
    for plane in (0, 33, 66, 67, 68):
        b, c = divmod(plane, 3)
        _, wm = msssim_ref.msssim(p[b, c], t[b, c], weights=w, data_range=L)
        err = np.abs(means[b, c] - wm).max()
        print(f"plane {plane}: max |mean - ref| = {err:.3e}")
        assert err <= 1e-9, (plane, means[b, c], wm)
    _timed("msssim", t0)


# ----------------------------------------------------------------------------- the tile kernels of tile_grid_x
# frames (2, 200, 200); patches of 132 x 128 = 16 896 and 130 x 130 = 16 900 pixels: the 64 workgroups take a second trip.
# 18 tiles each, the last row and column of tiles shifted back into the frame (starts 68 / 72 and 70 / 70) and clipped.
FRAMES = (2, 200, 200)
PLANS = [((1, 66, 64), (1, 132, 128)), ((1, 66, 66), (1, 130, 130))]
PLAN_IDS = ["pw128", "pw130"]
NORM6 = (1246.59, 1211.3, 759.685, 741.25, 486.905, 470.5)         # mean / std of the input, of target 0, of target 1
_ptr = lambda t: C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(grid, patch):
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan(FRAMES, grid, patch)
    ph, pw = patch[1:]
    assert plan.total == 18 and ph * pw > 64 * 256 and tuple(plan.patch_start[-1]) == (1, 200 - ph, 200 - pw)
    return plan, ph, pw


def _channels():
    ch0, ch1 = mixed_util.frames(FRAMES, 21)
    return ch0, ch1, torch.from_numpy(ch0.astype(np.float32)).cuda(), torch.from_numpy(ch1.astype(np.float32)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("grid,patch", PLANS, ids=PLAN_IDS)
def test_tiles_gather_norm_past_the_grid_cap(grid, patch):
    from diffsplitting_amd._lib import check, lib
    plan, ph, pw = _plan(grid, patch)
    ch0, ch1, f0, f1 = _channels()
    nd = dict(mean_input=np.float64(NORM6[0]), std_input=np.float64(NORM6[1]), mean_target=np.array([NORM6[2], NORM6[4]]),
              std_target=np.array([NORM6[3], NORM6[5]]))
    w = (1.0, 0.3)
    for from_norm in (0, 1):
        tin, ttar = _nan(plan.total, 1, ph, pw), _nan(plan.total, 2, ph, pw)
        check(lib.dsx_tileplan_gather_norm(plan.handle, _ptr(f0), _ptr(f1), 0, 1, plan.total, w[0], w[1],
                                           (C.c_double * 6)(*NORM6), from_norm, _ptr(tin), _ptr(ttar), _stream()))
        tin, ttar = tin.cpu().numpy(), ttar.cpu().numpy()
        for k in range(plan.total):
            ref = numpy_item(ch0, ch1, tuple(int(v) for v in plan.patch_start[k]), (ph, pw), nd, w, from_norm)
            assert same_bits(tin[k], ref["input"]) and same_bits(ttar[k], ref["target"]), (from_norm, k)


@pytest.mark.parametrize("grid,patch", PLANS, ids=PLAN_IDS)
def test_tiles_gather_norm_planes_past_the_grid_cap(grid, patch):
    from diffsplitting_amd._lib import check
    plan, ph, pw = _plan(grid, patch)
    rng = np.random.default_rng(11)
    N, Cc, H, W = 2, 2, 200, 200
    a = rng.integers(0, 256, size=(N, Cc, H, W), dtype=np.uint8)
    b = rng.integers(0, 256, size=(N, Cc, H, W), dtype=np.uint8)
    loc = [tuple(int(v) for v in s) for s in plan.patch_start[::4]]     # tiles 0, 4, 8, 12, 16: unshifted and shifted
    w, mean_inp, std_inp = (1, 0.3), 171.25, 93.5
    mt, st = np.array([101.0, 117.5, 130.25, 99.0]), np.array([61.0, 57.5, 70.25, 66.0])
    want_in, want_tar = cifar_files.numpy_items(a, b, loc, ph, pw, w, mean_inp, std_inp, mt, st)
    fa, fb = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (a, b))
    tin, ttar = _nan(len(loc), Cc, ph, pw), _nan(len(loc), 2 * Cc, ph, pw)
    check(cifar_files.gather_planes(fa, fb, (N, Cc, H, W), (ph, pw), loc, w, mean_inp, std_inp, mt, st, tin, ttar))
    assert same_bits(tin.cpu().numpy(), want_in) and same_bits(ttar.cpu().numpy(), want_tar)


def _ref_targets(plan, ch0, ch1, ids, ph, pw):
    t0, t1 = [], []
    for i in ids:
        n, y, x = (int(v) for v in plan.patch_start[i])
        t0.append(mixed_ref.normalize(ch0[n, y:y + ph, x:x + pw], NORM6[2], NORM6[3]))
        t1.append(mixed_ref.normalize(ch1[n, y:y + ph, x:x + pw], NORM6[4], NORM6[5]))
    return np.stack(t0), np.stack(t1)


@pytest.mark.parametrize("grid,patch", PLANS, ids=PLAN_IDS)
def test_tiles_gather_mix_past_the_grid_cap(grid, patch):
    """k_tiles_gather_mix through the plan's tables (one t and one table row for the launch) and
    k_tiles_gather_mix_items (one of each per item), bitwise the fp32 chain of tests/mixed_ref.py."""
    from diffsplitting_amd._lib import check, lib
    plan, ph, pw = _plan(grid, patch)
    ch0, ch1, f0, f1 = _channels()
    norm4 = (C.c_double * 4)(*NORM6[2:])
    lohi, t = (-2.0, 3.0, -1.5, 2.5), 0.29
    ids = list(range(1, plan.total, 2))                                 # tile 17 among them: shifted both ways
    t0, t1 = _ref_targets(plan, ch0, ch1, ids, ph, pw)
    tar, mix, cls = (_nan(len(ids), 2, ph, pw) for _ in range(3))
    check(lib.dsx_tileplan_gather_mix(plan.handle, _ptr(f0), _ptr(f1), 1, 2, len(ids), norm4, t, (C.c_double * 4)(*lohi),
                                      _ptr(tar), _ptr(mix), _ptr(cls), _stream()))
    want_mix, want_cls = mixed_ref.chain_f32(t0, t1, t, lohi)
    assert same_bits(tar.cpu().numpy(), np.stack([t0, t1], axis=1))
    assert same_bits(mix.cpu().numpy(), np.moveaxis(want_mix, 0, 1)) and same_bits(cls.cpu().numpy(), np.moveaxis(want_cls, 0, 1))
    # one record per item
    ts = np.array([0.0, 0.1, 0.29, 0.5, 1.0, 0.75, 0.33, 0.9, 0.02][:len(ids)], dtype=np.float64)
    rows = np.array([(-2.0 - 0.1 * k, 3.0 + 0.2 * k, -1.5 - 0.3 * k, 2.5 + 0.1 * k) for k in range(len(ids))], dtype=np.float64)
    loc = np.ascontiguousarray(plan.patch_start[ids], dtype=np.int64)
    pd = C.POINTER(C.c_double)
    tar, mix, cls = (_nan(len(ids), 2, ph, pw) for _ in range(3))
    check(lib.dsx_tiles_gather_mix_items(_ptr(f0), _ptr(f1), nets.i64(*FRAMES), nets.i64(1, ph, pw),
                                         loc.ctypes.data_as(C.POINTER(C.c_int64)), len(ids), norm4, ts.ctypes.data_as(pd),
                                         rows.ctypes.data_as(pd), _ptr(tar), _ptr(mix), _ptr(cls), _stream()))
    tar, mix, cls = tar.cpu().numpy(), mix.cpu().numpy(), cls.cpu().numpy()
    assert same_bits(tar, np.stack([t0, t1], axis=1))
    for k in range(len(ids)):
        want_mix, want_cls = mixed_ref.chain_f32(t0[k], t1[k], float(ts[k]), tuple(rows[k]))
        assert same_bits(mix[k], want_mix) and same_bits(cls[k], want_cls), k


@pytest.mark.parametrize("grid,patch", PLANS, ids=PLAN_IDS)
def test_tiles_gather_canvas_and_pack_past_the_grid_cap(grid, patch):
    """k_tiles_gather_canvas against numpy slicing; k_tiles_pack (valid regions of 2 x 99 x 96 and 2 x 98 x 98 elements
    and the clipped ones of the shifted tiles) against the oracle's packed runs."""
    plan, ph, pw = _plan(grid, patch)
    oplan = tiling.TilePlan(FRAMES, grid, patch)
    Cn, world = 2, 2
    rng = np.random.default_rng(7)
    canvas = rng.standard_normal(FRAMES + (Cn,)).astype(np.float32)
    cut = blend_ref.cut_tiles(plan, canvas)
    got = plan.gather_canvas(torch.from_numpy(canvas).cuda())
    assert same_bits(got.cpu().numpy(), cut)
    assert int(plan.regions[0][3]) * int(plan.regions[0][4]) * Cn > 64 * 256
    off, runs = plan.pack_layout(world)
    stride = plan.rank_stride(world, Cn)
    for r in range(world):
        ids = list(range(r, plan.total, world))
        flat = torch.zeros(stride, device="cuda")
        plan.pack(got[ids].contiguous(), world, r, flat)
        assert same_bits(flat.cpu().numpy(), tiling.pack_rank(cut[ids], ids, oplan, off, stride)), r
