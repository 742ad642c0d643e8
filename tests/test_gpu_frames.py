"""Frame diffusion for the InDI family on the MI355X (`-m gpu`): dsx_tileplan_blend_step bit for bit against the numpy
restatement of its contract (tests/blend_step_ref.py) with the noise taken from the sample streams; ``predict_stack_frames``
with one tile per frame against the unfused field chain, in general against the test's own restatement (numpy cuts,
``denoise_fn`` on the device, the step on the host), under two posterior samples and over ranks; what it is for, measured
against the float64 oracle; and ``split --frame-steps`` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import blend_ref, nets
from tests import tiled_util as T
from tests.bits import same_bits
from tests.blend_step_ref import blend_step_ref
from tests.rank_worker import run_ranks
from tests.tiled_util import BLEND_PLANS, SEED

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ((1 / 3, 2 / 3, 0.00666), (0.5, 0.5, 0.0), (1.0, 0.0, 0.25))      # (c_x0, c_xt, sigma): a row, no noise, no state


def _state(plan, Cn, seed=21):
    return np.random.default_rng(seed).standard_normal(plan.data_shape + (Cn,)).astype(np.float32)


def _same(state, want):
    return same_bits(state.cpu(), torch.from_numpy(want))


# ----------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("name", ["triangle", "hann"])
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_blend_step_is_its_restatement(shape, patch, grid, name):
    """odd W = 57 and C > 1: the stream index (c*H + y)*W + x of a pixel takes every residue mod 4 along a row and from
    row to row, so every component of a Philox block is picked at every lane position"""
    plan = T.plan_of(shape, patch, grid)
    plan.set_window(name)
    win = blend_ref.window_pair(plan, name)
    for Cn in (1, 2, 3):
        tiles, X = T.random_tiles(plan, Cn), _state(plan, Cn)
        dev = torch.from_numpy(tiles).cuda()
        for (c0, cx, sg), draw, id_base in zip(ROWS, (1, 4, 2), (0, 0, 7)):
            state = torch.from_numpy(X).cuda()
            got = plan.blend_step(dev, state, c0, cx, sg, SEED, draw, id_base=id_base)
            assert got.data_ptr() == state.data_ptr()                  # in place
            Z = T.frame_field(plan, Cn, SEED, draw, id_base) if sg != 0 else None
            assert _same(state, blend_step_ref(plan, tiles, *win, X, c0, cx, sg, Z)), (Cn, c0, cx, sg)
        # sigma == 0: c_x0 * blend + c_xt * X, whatever the draw
        blend = plan.blend(dev).cpu().numpy()
        f = np.float32
        want = ((f(0.5) * blend).astype(f) + (f(0.5) * X).astype(f)).astype(f)
        for draw in (0, 9):
            assert _same(plan.blend_step(dev, torch.from_numpy(X).cuda(), 0.5, 0.5, 0.0, SEED, draw), want), (Cn, draw)
        # a second call with the next draw: other noise
        c0, cx, sg = ROWS[0]
        one = plan.blend_step(dev, torch.from_numpy(X).cuda(), c0, cx, sg, SEED, 1)
        two = plan.blend_step(dev, torch.from_numpy(X).cuda(), c0, cx, sg, SEED, 2)
        assert not torch.equal(one, two)
        assert _same(two, blend_step_ref(plan, tiles, *win, X, c0, cx, sg, T.frame_field(plan, Cn, SEED, 2)))


@pytest.mark.parametrize("Cn", [4, 5])
def test_blend_step_wide_and_any_channel_count(Cn):
    """C = 4 (one 16-byte access per pixel) and C = 5 (the kernel's any-C form)"""
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("triangle")
    tiles, X = T.random_tiles(plan, Cn), _state(plan, Cn)
    c0, cx, sg = ROWS[0]
    got = plan.blend_step(torch.from_numpy(tiles).cuda(), torch.from_numpy(X).cuda(), c0, cx, sg, SEED, 3, id_base=5)
    want = blend_step_ref(plan, tiles, *blend_ref.window_pair(plan, "triangle"), X, c0, cx, sg, T.frame_field(plan, Cn, SEED, 3, 5))
    assert _same(got, want)


@pytest.mark.parametrize("Cn", [2, 4])
def test_blend_step_on_an_unaligned_view(Cn):
    """the state one float past a 16-byte boundary: one dword per channel; its NaN neighbours stay NaN"""
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("hann")
    tiles, X = T.random_tiles(plan, Cn), _state(plan, Cn)
    n = X.size
    buf = torch.full((n + 9,), float("nan"), device="cuda")
    view = buf[5:5 + n].view(X.shape)
    view.copy_(torch.from_numpy(X))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    c0, cx, sg = ROWS[0]
    plan.blend_step(torch.from_numpy(tiles).cuda(), view, c0, cx, sg, SEED, 1)
    want = blend_step_ref(plan, tiles, *blend_ref.window_pair(plan, "hann"), X, c0, cx, sg, T.frame_field(plan, Cn, SEED, 1))
    assert _same(view, want)
    assert bool(torch.isnan(buf[:5]).all()) and bool(torch.isnan(buf[5 + n:]).all())


@pytest.mark.parametrize("world", [2, 3])
def test_the_rank_slot_layouts_give_the_one_rank_bits(world):
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("hann")
    c0, cx, sg = ROWS[0]
    for Cn in (1, 2, 3):
        tiles, X = T.random_tiles(plan, Cn), _state(plan, Cn)
        one = plan.blend_step(torch.from_numpy(tiles).cuda(), torch.from_numpy(X).cuda(), c0, cx, sg, SEED, 1)
        buf = torch.from_numpy(blend_ref.slots(plan, tiles, world)).cuda()
        got = plan.blend_step(buf, torch.from_numpy(X).cuda(), c0, cx, sg, SEED, 1, world=world, Cn=Cn)
        assert same_bits(got, one), Cn


# ----------------------------------------------------------------------------- 2. one tile per frame: the unfused chain
@pytest.mark.parametrize("make", [T.indi, T.joint], ids=["indi", "joint_indi"])
def test_one_tile_per_frame_is_the_unfused_chain(make):
    """frames (2, 32, 32), patch 32: gather and blend are copies, so frame diffusion is ``inference`` row by row"""
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames
    netG, stack = make(), T.stack((2, 32, 32), 32, 16)
    assert stack.plan.total == 2
    want, _ = predict_stack(netG, stack, batch_tiles=2, num_timesteps=3, seed=SEED, noise="field")
    got, plan = predict_stack_frames(netG, stack, batch_tiles=2, num_timesteps=3, seed=SEED)
    assert plan is stack.plan and set(got) == {"mean"} and bool(torch.isfinite(got["mean"]).all())
    assert got["mean"].shape == (2, 32, 32, 2) and same_bits(got["mean"], want["mean"])
    other, _ = predict_stack_frames(netG, stack, batch_tiles=2, num_timesteps=3, seed=SEED + 1)
    assert not torch.equal(other["mean"], got["mean"])
    assert netG.noise_field is None and netG.noise_source is None


# ----------------------------------------------------------------------------- 3. in general: the restatement
FOURS = [(list(range(i, i + 4)), 4) for i in (0, 4, 8)]
FIVES = [([0, 1, 2, 3, 4], 5), ([5, 6, 7, 8, 9], 5), ([7, 8, 9, 10, 11], 2)]     # the short last batch moved back


@pytest.mark.parametrize("window", ["triangle", "hann"])
@pytest.mark.parametrize("make", [T.indi, T.joint], ids=["indi", "joint_indi"])
def test_frame_diffusion_is_its_restatement(make, window):
    """frames (2, 40, 57), patch 32, grid 16: 12 tiles in batches of 4, then of 5 with the last moved back"""
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames
    netG, stack = make(), T.stack32()
    got, _ = predict_stack_frames(netG, stack, batch_tiles=4, num_timesteps=3, seed=SEED, window=window)
    assert got["mean"].shape == (2, 40, 57, 2)
    assert _same(got["mean"], T.restated_frames(netG, stack, 3, FOURS, window=window))
    five, _ = predict_stack_frames(netG, stack, batch_tiles=5, num_timesteps=3, seed=SEED, window=window)
    assert _same(five["mean"], T.restated_frames(netG, stack, 3, FIVES, window=window))
    unfused, _ = predict_stack(netG, stack, batch_tiles=4, num_timesteps=3, seed=SEED, noise="field", stitch="blend",
                               window=window)
    assert not torch.equal(unfused["mean"], got["mean"])


# ----------------------------------------------------------------------------- 4. two samples
def test_two_samples():
    """sample r takes id_base = r * frames; mean and spread are the float64 Welford of the two restated frame states"""
    from diffsplitting_amd.data.tiled_predict import predict_stack_frames
    netG, stack = T.indi(), T.stack32()
    got, _ = predict_stack_frames(netG, stack, batch_tiles=4, num_timesteps=3, seed=SEED, samples=2, return_std=True)
    xs = [T.restated_frames(netG, stack, 3, FOURS, r=r) for r in range(2)]
    assert not np.array_equal(xs[0], xs[1])
    mean, std = T.welford(xs)
    assert _same(got["mean"], mean)
    assert _same(got["std"], std) and bool((got["std"] > 0).any())


# ----------------------------------------------------------------------------- 5. sharding
@pytest.mark.parametrize("world", [2, 3])
def test_frame_diffusion_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout), gloo transport: on every rank the frames equal
    the one-rank restatement, bitwise (tests/multi_rank_predict_frames.py)"""
    r = run_ranks("multi_rank_predict_frames.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_FRAMES_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ----------------------------------------------------------------------------- 6. what it is for
INDI_CFG = dict(in_channel=2, out_channel=2, inner_channel=16, norm_groups=16, channel_mults=(1, 2, 4), attn_res=(),
                res_blocks=1, image_size=32)


def oracle_seams(plan, table, sd64, x_in, scale, fields):
    """The float64 oracle (oracle/unet.py; blend and update in float64) on the input frame ``x_in`` (N, H, W, C) and the
    frame noise ``fields[d]`` (N, H, W, C) of every draw: the final tiles without frame diffusion (every tile runs the
    InDI rows on its own, with its crops of the fields) and the x0 tiles of the last row with it -> (field, frames)."""
    from oracle import unet as oracle_unet
    n = table.n_steps
    c1, c2, sg, tc = (np.asarray(getattr(table, k), dtype=np.float64) for k in ("c1", "c2", "sigma", "tcond"))
    net = lambda x, s: oracle_unet.unet_forward(sd64, INDI_CFG, "ddpm", torch.from_numpy(x),
                                                torch.tensor([tc[s]], dtype=torch.float64)).numpy()
    start = x_in + fields[0] * scale
    x = blend_ref.cut_tiles(plan, start)
    for s in range(n):
        x = c1[s] * net(x, s) + c2[s] * x + blend_ref.cut_tiles(plan, fields[s + 1]) * sg[s]
    wy, wx = blend_ref.window_pair(plan, "triangle")
    X, x0 = start, None
    for s in range(n):
        x0 = net(blend_ref.cut_tiles(plan, X), s)
        X = c1[s] * blend_ref.blend_ref(plan, x0, wy, wx, dtype=np.float64) + c2[s] * X + fields[s + 1] * sg[s]
    return x, x0


def test_frame_diffusion_narrows_what_the_field_leaves():
    """The setting of test_fusion_narrows_what_the_field_leaves: one (1, 64, 96) frame of smooth input, all 15 tiles in
    one batch, the seam RMS over the 12 crop lines, InDI with n = 4.  With frame diffusion: of the x0 tiles of the LAST
    row, before the last ``blend_step`` -- there c_x0 = delta / t is 1 up to rounding, so these are what every tile
    would become.  Without: of the final tiles of the unfused field run, where every tile ran all rows on its own.

    The bound on rms_frames / rms_field is twice the ratio of the float64 oracle on the same weights, input and noise,
    and never above 1; the factor 2 is for fp32 and the planner's choice of kernels.  Measured on one MI355X:
    frames 0.506617, field 0.835374, ratio 0.606455; the oracle gives the same six digits (largest |device - oracle|
    over the tiles 1.7e-5 frames, 2.3e-5 field), so the bound is 1.  Random weights only: no trained checkpoint is at hand, so this says nothing about image quality."""
    from diffsplitting_amd import engine
    from diffsplitting_amd.data.tiled_predict import frame_sample, input_frames
    netG = T.indi()
    stack = T.stack((1, 64, 96), 32, 16, seed=2)
    plan = stack.plan
    ids = list(range(plan.total))
    assert plan.total == 15 and all(int(v) % 8 == 0 for v in plan.patch_start[:, 1:].reshape(-1))   # no shifted tile
    n = 4
    try:
        netG.noise_field = lambda shape, draw: plan.randn_field(ids, shape[1], SEED, draw)
        netG.inference(stack.tiles(ids)["input"], continuous=False, num_timesteps=n)
        got = {"field": netG.last_full_batch.cpu().numpy()}
    finally:
        netG.noise_field = None
    plan.set_window("triangle")
    x_in = input_frames(stack, 15)
    rows = []
    frame_sample(netG, stack, x_in, n, 1.0, 15, SEED, 0, keep_tiles=rows)
    assert len(rows) == n
    got["frames"] = rows[-1].cpu().numpy()
    table = engine.indi_step_table(n, 1.0, netG.e)
    assert abs(float(table.c1[-1]) - 1) < 1e-6
    sd64 = {k: v.detach().double().cpu() for k, v in netG.denoise_fn.state_dict().items()}
    fields = [T.frame_field(plan, 2, SEED, d).astype(np.float64) for d in range(n + 1)]
    x64 = np.concatenate([x_in.cpu().numpy().astype(np.float64)] * 2, axis=-1)
    scale = float((netG.e * torch.Tensor([1.0])).item())
    want = dict(zip(("field", "frames"), oracle_seams(plan, table, sd64, x64, scale, fields)))
    rms = {k: T.seam_rms(plan, got[k])[0] for k in got}
    rms64 = {k: T.seam_rms(plan, want[k])[0] for k in want}
    assert T.seam_rms(plan, got["frames"])[1] == 12
    ratio, ratio64 = rms["frames"] / rms["field"], rms64["frames"] / rms64["field"]
    print(f"\nseam rms over 12 seams: frames {rms['frames']:.6f}, field {rms['field']:.6f}, ratio {ratio:.6f}; float64 "
          f"oracle: frames {rms64['frames']:.6f}, field {rms64['field']:.6f}, ratio {ratio64:.6f}")
    print("largest |device - oracle| over the tiles:", {k: float(np.abs(got[k] - want[k]).max()) for k in got})
    assert ratio64 < 1.0
    assert ratio <= min(1.0, 2.0 * ratio64)


# ----------------------------------------------------------------------------- 7. split, end to end
def split_frame_runs(tmp_path, runs):
    """fresh `split` processes at once on a tiny indi config -> the bytes of every --out"""
    cfg = {"name": "tiny_indi", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 32, "max_qval": 0.98, "upper_clip": False, "train": {"name": "Hagen"},
                        "val": {"name": "Hagen"}},
           "model": nets.tiny_indi_section()}
    cfg_path = str(tmp_path / "tiny_indi.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "diffsplitting_amd.split", "-c", cfg_path, "-p", "val", "-gpu", "0", "--synthetic", "1,64,64",
            "--sample-seed", "3", "--batch-tiles", "3"]
    procs = {}
    for name, flags in runs.items():
        root = tmp_path / name
        root.mkdir()
        procs[name] = subprocess.Popen(base + flags + ["-rootdir", str(root), "--out", str(root / "pred.npy")], env=env,
                                       cwd=str(root), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for name, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-3000:])
    pred = np.load(tmp_path / next(iter(runs)) / "pred.npy")
    assert pred.shape == (1, 64, 64, 2) and pred.dtype == np.float32 and np.isfinite(pred).all()
    return {name: open(tmp_path / name / "pred.npy", "rb").read() for name in runs}


def test_split_frame_steps_end_to_end(tmp_path):
    """fresh processes at once: --frame-steps twice (byte for byte the same file), the unfused field run blended and cropped"""
    data = split_frame_runs(tmp_path, {"a": ["--frame-steps"], "b": ["--frame-steps"],
                                       "blend": ["--noise-field", "--stitch", "blend"], "crop": ["--noise-field"]})
    assert data["a"] == data["b"] and data["a"] != data["blend"] and data["a"] != data["crop"]
