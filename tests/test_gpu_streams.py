"""Per-sample noise streams on the MI355X (`-m gpu`): dsx_randn_samples against the existing generator, the stream form
of the loop against the same draws injected, invariance under a permutation of the batch, the caller-driven steps
against the loop, and the samplers' seed= / sample_ids= keywords.  Every comparison is bitwise."""
import functools

import numpy as np
import pytest
import torch

from oracle import cases
from tests import nets
from tests.bits import same_bits
from tests.gpu_util import build_engine
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOP = (1 << 40) - 1
SR3_T4 = dict(schedule="linear", n_timestep=4, linear_start=1e-4, linear_end=2e-1)


# ----------------------------------------------------------------------------- 1. randn_samples
@pytest.mark.parametrize("chw", [(3, 5, 7), (3, 8, 8)])           # 105: scalar stores and a cut last block; 192: 16-byte stores
@pytest.mark.parametrize("draw", [0, 1, (1 << 24) - 1])
def test_randn_samples_rows_are_the_existing_streams(chw, draw):
    from diffsplitting_amd import engine
    ids = [9, 0, TOP, 1 << 33, 4, (1 << 33) + (1 << 20)]         # unordered, sparse, the largest id
    n = int(np.prod(chw))
    out = engine.randn_samples((len(ids),) + chw, 2024, ids, draw=draw)
    assert out.shape == (len(ids),) + chw
    for b, i in enumerate(ids):
        assert same_bits(out[b].reshape(-1), engine.randn((n,), 2024, subsequence=(i << 24) | draw)), (b, i)
    # a row does not depend on the batch it is drawn in or on its position there
    alone = engine.randn_samples((1,) + chw, 2024, [ids[3]], draw=draw)
    assert same_bits(alone[0], out[3])


def test_randn_samples_more_rows_than_one_launch_carries():
    """The ids travel in the kernel arguments, 32 per launch: 70 rows take three launches (tail path, odd row length)."""
    from diffsplitting_amd import engine
    ids = [(k * 7919) % 1000 + (k << 30) for k in range(70)]
    out = engine.randn_samples((70, 1, 3, 7), 5, ids, draw=3)
    for b in (0, 31, 32, 63, 64, 69):
        assert same_bits(out[b].reshape(-1), engine.randn((21,), 5, subsequence=(ids[b] << 24) | 3)), b


def test_randn_samples_ids_differing_above_bit_32_differ():
    from diffsplitting_amd import engine
    out = engine.randn_samples((3, 3, 8, 8), 1, [5, 5 + (1 << 32), 5 + (1 << 39)])
    assert not same_bits(out[0], out[1]) and not same_bits(out[0], out[2]) and not same_bits(out[1], out[2])
    other_seed = engine.randn_samples((3, 3, 8, 8), 2, [5, 5 + (1 << 32), 5 + (1 << 39)])
    assert not same_bits(out, other_seed)


def test_randn_samples_moments():
    """Mean and variance of n = 2^20 values within 5 standard errors of 0 and 1: se(mean) = 1 / sqrt(n),
    se(variance) = sqrt(2 / n) for normal values."""
    from diffsplitting_amd import engine
    ids = [3, TOP, 1 << 35, 77]
    v = engine.randn_samples((4, 4, 256, 256), 7, ids, draw=1).double()
    n = v.numel()
    assert n >= 10 ** 6
    mean, var = float(v.mean()), float(v.var())
    print(f"randn_samples moments over {n}: mean {mean:.3e} (5 se = {5 / n ** 0.5:.3e}), var - 1 {var - 1:.3e} "
          f"(5 se = {5 * (2 / n) ** 0.5:.3e})")
    assert abs(mean) <= 5 / n ** 0.5
    assert abs(var - 1) <= 5 * (2 / n) ** 0.5


def test_bad_ids_are_refused_by_name():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    with pytest.raises(DsxError, match="sample id"):
        engine.randn_samples((2, 3, 8, 8), 1, [0, 1 << 40])
    with pytest.raises(DsxError, match="draw ordinal"):
        engine.randn_samples((2, 3, 8, 8), 1, [0, 1], draw=1 << 24)
    with pytest.raises(DsxError, match="B = 2"):
        engine.randn_samples((2, 3, 8, 8), 1, [0, 1, 2])


# ----------------------------------------------------------------------------- 2. loop: streams against injection
@functools.lru_cache(maxsize=None)
def _engine(name, dtype):
    fixture, case, flavour = {"sr3": ("loop_sr3_lin_8", "sr3_tiny", "sr3"), "indi2": ("loop_indi_n3_t1.0", "ddpm_tiny", "ddpm"),
                              "indi1": ("unet_joint_32", "joint_32", "ddpm")}[name]
    sd, _ = golden_state_dict(fixture)
    return build_engine(cases.UNET_CASES[case]["cfg"], flavour, sd, dtype=dtype)


def _case(name, B, per_sample=False):
    """(table, state shape, cond or None) of a loop case: an SR3-type table (T = 4, last sigma 0, clip on, C = 3), or an
    InDI-type table (n = 3) with C = 2 / C = 1, optionally one schedule per sample."""
    from diffsplitting_amd import engine
    if name == "sr3":
        bufs, gamma = engine.gaussian_buffers(SR3_T4)
        tab = engine.gaussian_step_table(bufs, gamma, "sr3", True)
        assert tab.n_steps == 4 and tab.sigma[-1] == 0 and tab.clip
        return tab, (B, 3, 32, 32), nets.rand((B, 3, 32, 32), 40).cuda()
    if per_sample:
        tab = engine.indi_step_table_per_sample(3, [1.0, 0.6, 0.8, 0.35][:B])
    else:
        tab = engine.indi_step_table(3, 1.0)
    return tab, ((B, 2, 32, 48) if name == "indi2" else (B, 1, 32, 32)), None


def _injection(shape, T, seed, ids):
    from diffsplitting_amd import engine
    return torch.stack([engine.randn_samples(shape, seed, ids, draw=d) for d in range(1, T + 1)])   # (T, B, C, H, W)


def _both(eng, tab, shape, cond, seed, ids, use_graph):
    """The final states of the loop with sample streams and of the loop fed the same draws, from the same start."""
    from diffsplitting_amd import engine
    x0 = engine.randn_samples(shape, seed, ids, draw=0)
    got, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=seed, sample_ids=ids, use_graph=use_graph)
    ref, _ = eng.sample_loop(tab, x0.clone(), cond=cond, noise=_injection(shape, tab.n_steps, seed, ids),
                             use_graph=use_graph)
    torch.cuda.synchronize()
    return got, ref, x0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name,per_sample", [("sr3", False), ("indi2", False), ("indi1", False), ("indi2", True)])
def test_loop_with_streams_equals_loop_with_the_same_draws_injected(name, per_sample, use_graph, dtype):
    B = 3
    tab, shape, cond = _case(name, B, per_sample)
    got, ref, x0 = _both(_engine(name, dtype), tab, shape, cond, 11, [6, TOP, 1 << 34], use_graph)
    assert bool(torch.isfinite(got).all()) and not same_bits(got, x0)
    assert same_bits(got, ref)


@pytest.mark.parametrize("name", ["sr3", "indi2"])
def test_kept_graph_serves_calls_with_other_ids(name):
    """Two consecutive stream calls on one executor: the second replays the graph the first captured (the ids live in
    executor-owned device memory, nothing of them in a kernel node) and still draws from ITS ids."""
    from diffsplitting_amd import engine
    eng = _engine(name, "f32")
    tab, shape, cond = _case(name, 3)
    ids_a, ids_b = [1, 2, 3], [3, 1 << 36, 1]
    x0 = nets.rand(shape, 41).cuda()
    got_a, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=5, sample_ids=ids_a, use_graph=True)
    got_b, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=5, sample_ids=ids_b, use_graph=True)
    for got, ids in ((got_a, ids_a), (got_b, ids_b)):            # eager references: the kept graph is not touched
        ref, _ = eng.sample_loop(tab, x0.clone(), cond=cond, noise=_injection(shape, tab.n_steps, 5, ids), use_graph=False)
        assert same_bits(got, ref)
    assert not same_bits(got_a, got_b)
    # the default noise still works on the same executor afterwards, and differs
    dflt, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=5, use_graph=True)
    assert bool(torch.isfinite(dflt).all()) and not same_bits(dflt, got_a)


def test_loop_refusals_on_the_device():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    eng = _engine("indi2", "f32")
    tab, shape, _ = _case("indi2", 3)
    x0 = nets.rand(shape, 42).cuda()
    with pytest.raises(DsxError, match="injected noise"):
        eng.sample_loop(tab, x0.clone(), noise=torch.zeros((3,) + shape, device="cuda"), sample_ids=[1, 2, 3])
    with pytest.raises(DsxError, match="B = 3"):
        eng.sample_loop(tab, x0.clone(), sample_ids=[1, 2])
    with pytest.raises(DsxError, match="sample id"):
        eng.sample_loop(tab, x0.clone(), sample_ids=[1, 2, 1 << 40])


# ----------------------------------------------------------------------------- 3. permutation
@pytest.mark.parametrize("name", ["sr3", "indi2"])
def test_permuting_inputs_and_ids_permutes_the_outputs(name):
    eng = _engine(name, "f32")
    B, perm = 4, [2, 0, 3, 1]
    tab, shape, cond = _case(name, B)
    ids = [10, 1 << 38, 7, 123456789]
    x0 = nets.rand(shape, 43).cuda()
    out, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=9, sample_ids=ids)
    out_p, _ = eng.sample_loop(tab, x0[perm].clone(), cond=None if cond is None else cond[perm].contiguous(), seed=9,
                               sample_ids=[ids[p] for p in perm])
    assert same_bits(out_p, out[perm])
    # the default noise is indexed by the position in the batch: the same permutation changes the result
    dflt, _ = eng.sample_loop(tab, x0.clone(), cond=cond, seed=9)
    dflt_p, _ = eng.sample_loop(tab, x0[perm].clone(), cond=None if cond is None else cond[perm].contiguous(), seed=9)
    assert not same_bits(dflt_p, dflt[perm])


# ----------------------------------------------------------------------------- 4. caller-driven against the loop
@functools.lru_cache(maxsize=None)
def _sr3_sampler():
    from diffsplitting_amd.model.samplers import GaussianSampler
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    smp = GaussianSampler(nets.unet("sr3", cases.UNET_CASES["sr3_tiny"]["cfg"]), 32, channels=3, conditional=True).cuda()
    smp.set_new_noise_schedule(SR3_T4, "cuda")
    nets.load(smp, sd)
    return smp


@functools.lru_cache(maxsize=None)
def _indi_sampler():
    from diffsplitting_amd.model.samplers import InDISampler
    sd, _ = golden_state_dict("loop_indi_n3_t1.0")
    smp = InDISampler(nets.unet("ddpm", cases.UNET_CASES["ddpm_tiny"]["cfg"]), 32, channels=2, out_channel=2,
                      conditional=False, val_schedule_opt={"n_timestep": 3}).cuda()
    smp.set_new_noise_schedule({"n_timestep": 3}, "cuda")
    nets.load(smp, sd)
    return smp


@functools.lru_cache(maxsize=None)
def _joint_sampler():
    from diffsplitting_amd.model import networks
    sd, _ = golden_state_dict("loop_joint_n3")
    netG = networks.define_G(nets.opt(nets.tiny_indi_section(1, 1, "joint_indi"))).cuda()
    netG.load_state_dict(sd, strict=True)
    netG.set_new_noise_schedule({"n_timestep": 3}, "cuda")
    return netG


def test_p_sample_calls_with_ids_reproduce_the_loop():
    from diffsplitting_amd import engine
    smp = _sr3_sampler()
    cond = nets.rand((2, 3, 32, 32), 44).cuda()
    ids, seed, T = [1 << 37, 12], 21, 4
    smp.p_sample_loop(cond, seed=seed, sample_ids=ids)
    loop = smp.last_full_batch.clone()
    img = engine.randn_samples((2, 3, 32, 32), seed, ids, draw=0)
    for t in reversed(range(T)):
        img = smp.p_sample_seeded(img, t, seed, ids, condition_x=cond)
    assert same_bits(loop, img)


def test_inference_one_step_calls_with_ids_reproduce_the_loop():
    from diffsplitting_amd import engine
    smp = _indi_sampler()
    n, ids, seed = 3, [8, TOP, 1 << 20], 22
    x_in = cases.make_cond("indi_loop").cuda()                                  # (3, 1, 32, 48)
    smp.inference(x_in, seed=seed, sample_ids=ids)
    loop = smp.last_full_batch.clone()
    x = torch.cat([x_in] * 2, dim=1) + engine.randn_samples((3, 2, 32, 48), seed, ids, draw=0) * \
        (smp.e * torch.Tensor([1.0])).cuda()                                    # indi.py:80-82
    delta, cur = 1.0 / n, 1.0
    for s in range(n):
        x = smp.inference_one_step_seeded(x, delta, cur, seed, ids, draw=s + 1)
        cur -= delta
    assert smp.e == 0.01 and same_bits(loop, x)


@pytest.mark.parametrize("shape", [(40, 3, 5, 7), (40, 2, 4, 8), (3, 1, 5, 5)])
def test_posterior_step_with_ids_draws_the_sample_streams(shape):
    """sigma = 1 and c1 = c2 = 0 make x_out the draw itself (0 + z * 1): compared with randn_samples directly, on the
    scalar path (H*W odd: groups straddle samples), the 16-byte path, and 40 samples (two launches of 32 ids at most);
    a sample with sigma == 0 keeps its mean."""
    from diffsplitting_amd import engine
    B = shape[0]
    ids = [(b * 104729) % 5000 + ((b % 3) << 35) for b in range(B)]
    x, net = nets.rand(shape, 46).cuda(), nets.rand(shape, 47).cuda()
    zero, sigma = torch.zeros(B, device="cuda"), torch.ones(B, device="cuda")
    sigma[1] = 0.0
    out = engine.posterior_step(x, net, zero, zero, sigma, seed=13, sample_ids=ids, draw=6, x_out=torch.empty_like(x))[2]
    z = engine.randn_samples(shape, 13, ids, draw=6)
    keep = [b for b in range(B) if b != 1]
    assert same_bits(out[keep], z[keep])
    assert bool((out[1] == 0).all())                                           # its mean, 0 * net + 0 * x: a zero of either sign


# ----------------------------------------------------------------------------- 5. samplers
def _sampler_runs(run):
    """run(seed, ids) -> the full batch; checks repeatability, seed and id sensitivity, and torch's generator."""
    state = torch.get_rng_state().clone()
    cuda_state = torch.cuda.get_rng_state().clone()
    a, b = run(3, [5, 6]), run(3, [5, 6])
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(), cuda_state)
    assert same_bits(a, b)
    assert not same_bits(a, run(4, [5, 6]))
    c = run(3, [5, 7])
    assert same_bits(a[0], c[0]) and not same_bits(a[1], c[1])                # sample 0 kept its id: it kept its bits
    return a


def test_gaussian_sampler_keywords():
    from diffsplitting_amd._lib import DsxError
    smp = _sr3_sampler()
    cond = nets.rand((2, 3, 32, 32), 45).cuda()

    def run(seed, ids):
        smp.super_resolution(cond, seed=seed, sample_ids=ids)
        return smp.last_full_batch.clone()
    a = _sampler_runs(run)
    smp.predict(cond, seed=3, sample_ids=[5, 6])
    assert same_bits(a, smp.last_full_batch)
    with pytest.raises(DsxError, match="noise_source together with sample_ids"):
        smp.noise_source = lambda shape: torch.zeros(shape)
        try:
            smp.super_resolution(cond, seed=3, sample_ids=[5, 6])
        finally:
            smp.noise_source = None
    with pytest.raises(DsxError, match="only together with sample_ids"):
        smp.super_resolution(cond, seed=3)


def test_indi_sampler_keywords():
    smp = _indi_sampler()
    x_in = cases.make_cond("indi_loop")[:2].cuda()

    def run(seed, ids):
        smp.inference(x_in, seed=seed, sample_ids=ids)
        return smp.last_full_batch.clone()
    _sampler_runs(run)
    # per-sample start times take the same streams
    smp.inference(x_in, t_float_start=torch.tensor([1.0, 1.0]), seed=3, sample_ids=[5, 6])
    assert same_bits(smp.last_full_batch, run(3, [5, 6]))


def test_joint_sampler_channels_do_not_share_draws():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    netG = _joint_sampler()
    x_in = cases.make_cond("joint_loop").cuda()                                  # (2, 1, 32, 32)

    def run(seed, ids):
        netG.inference(x_in, seed=seed, sample_ids=ids)
        torch.cuda.synchronize()
        return netG.last_full_batch.clone()
    _sampler_runs(run)
    # the initial perturbations of the two channels: draw 0 of the ids, and of the ids with bit 39 set
    ids = [5, 6]
    p1 = netG.indi1._start(x_in, 0.5, (3, ids)) - x_in
    p2 = netG.indi2._start(x_in, 0.5, (3, netG.second_ids(ids))) - x_in
    assert netG.second_ids(ids) == [5 + (1 << 39), 6 + (1 << 39)]
    assert not same_bits(p1, p2) and float((p1 - p2).abs().max()) > 0
    z2 = engine.randn_samples(x_in.shape, 3, [5 + (1 << 39), 6 + (1 << 39)])
    assert same_bits(netG.indi2._start(x_in, 0.5, (3, netG.second_ids(ids))), x_in + z2 * (netG.indi2.e * torch.Tensor([0.5])).cuda())
    with pytest.raises(DsxError, match=r"2\^39"):
        netG.inference(x_in, seed=3, sample_ids=[5, 1 << 39])
    # the concurrent and the back-to-back form draw the same
    a = run(3, ids)
    netG.concurrent = False
    try:
        assert same_bits(a, run(3, ids))
    finally:
        netG.concurrent = True


def test_predict_tiled_with_a_seed_does_not_depend_on_the_batch_order():
    """One rank: the batches of predict_tiled taken in reversed order give the same canvas with a seed (the sampler's
    own e = 0.01), and another without."""
    from diffsplitting_amd.data.tiled_predict import predict_tiled
    from diffsplitting_amd.model import networks
    sd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()})
    assert netG.e == 0.01
    frames = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 96, 160)).astype(np.float32)).cuda()
    pred, plan = predict_tiled(netG, frames, patch_size=64, grid_size=32, batch_tiles=4, sampler_kwargs=dict(num_timesteps=2),
                               seed=11)
    assert plan.total == 8

    def reversed_batches(**kw):
        out = {}
        for i in reversed(range(0, plan.total, 4)):
            chunk = list(range(i, i + 4))
            extra = dict(seed=kw["seed"], sample_ids=chunk) if "seed" in kw else {}
            netG.inference(plan.gather(frames, chunk).unsqueeze(1), continuous=False, num_timesteps=2, **extra)
            out[i] = netG.last_full_batch.clone()
        return plan.stitch(torch.cat([out[i] for i in sorted(out)]))
    assert same_bits(pred, reversed_batches(seed=11))
    torch.manual_seed(0)
    plain, _ = predict_tiled(netG, frames, patch_size=64, grid_size=32, batch_tiles=4, sampler_kwargs=dict(num_timesteps=2))
    torch.manual_seed(0)
    assert not torch.equal(plain, reversed_batches())


# ----------------------------------------------------------------------------- the command lines
def test_split_sample_seed(tmp_path):
    """`split --sample-seed S`: the same seed twice gives the same canvas, another seed or no seed another one."""
    import json
    from diffsplitting_amd import split
    cfg = {"name": "tiny_hagen_indi", "phase": "train", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"val": {"name": "Hagen", "patch_size": 64, "datatype": "img"}}, "model": nets.tiny_indi_section()}
    p = tmp_path / "tiny.json"
    p.write_text(json.dumps(cfg, indent=2))

    def run(*extra):
        torch.manual_seed(0)                                                    # the random initial weights
        return split.main(["-c", str(p), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--synthetic", "1,128,128",
                           "--steps", "2", "--batch-tiles", "3", *extra]).clone()
    a, b = run("--sample-seed", "7"), run("--sample-seed", "7")
    assert a.shape == (1, 128, 128, 2) and bool(torch.isfinite(a).all())
    assert same_bits(a, b)
    assert not same_bits(a, run("--sample-seed", "8")) and not same_bits(a, run())
    with pytest.raises(SystemExit, match="--sample-seed"):
        run("--sample-seed", "7", "--validate")


def test_infer_sample_seed_regenerates_one_image(tmp_path):
    """`infer --sample-seed S`: image 3 of the folder (ordinal 2) is a batch of its own under --batch 2 and under
    --batch 1; its sample is the same in both runs although other images ran before it in other batches -- and is not
    without the flag."""
    import json
    from diffsplitting_amd import infer
    from PIL import Image
    rng = np.random.default_rng(12)
    src = tmp_path / "src"
    src.mkdir()
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)).save(src / f"{k}.png")
    sec = {"which_model_G": "sr3", "finetune_norm": False,
           "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": 32, "norm_groups": 32,
                    "channel_multiplier": [1, 2, 4], "attn_res": [16], "res_blocks": 2, "dropout": 0.2},
           "beta_schedule": {"train": dict(SR3_T4), "val": dict(SR3_T4)},
           "diffusion": {"image_size": 32, "channels": 3, "conditional": True}}

    def run(tag, *extra):
        cfg = {"name": "tiny_sr3", "phase": "val", "gpu_ids": [0],
               "path": {"log": str(tmp_path / "logs"), "results": str(tmp_path / tag), "checkpoint": str(tmp_path),
                        "resume_state": None},
               "datasets": {"val": {"name": "tiny", "mode": "LRHR", "dataroot": "unused", "datatype": "hr_only",
                                    "l_resolution": 8, "r_resolution": 32, "data_len": -1}}, "model": sec}
        p = tmp_path / f"{tag}.json"
        p.write_text(json.dumps(cfg, indent=2))
        infer.main(["-c", str(p), "-p", "val", "-gpu", "0", "--dataroot", str(src), "--seed", "5", *extra])
        return np.asarray(Image.open(tmp_path / tag / "0_3_sr.png")).copy()
    by2, by1 = run("s2", "--batch", "2", "--sample-seed", "9"), run("s1", "--batch", "1", "--sample-seed", "9")
    assert by2.shape == (32, 32, 3) and np.array_equal(by2, by1)
    assert not np.array_equal(run("p2", "--batch", "2"), run("p1", "--batch", "1"))
