"""Frame-keyed noise and the Gaussian tiled path on the MI355X (`-m gpu`): dsx_tileplan_randn against the crops of the
existing sample streams (every row residue mod 4, the 16-byte and the scalar stores, an unaligned output), what the
field is for (tiles of one frame share the bits of their overlap), ``predict_stack`` with a Gaussian sampler (solvers
and the ancestral loop) and with ``noise="field"`` against the test's own restatement through ``noise_source``, InDI and
JointIndi, ``split`` end to end, and the seam property measured against the float64 oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tiled_util as T
from tests.bits import same_bits
from tests.tiled_util import BATCH, SCHED, SEED, SOLVERS, TINY, Source

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(patch, grid, shape=(2, 40, 57)):
    from diffsplitting_amd.data.tiling import TilePlan
    return TilePlan(shape, (1, grid, grid), (1, patch, patch))


ID_LISTS = {"all": lambda total: list(range(total)), "strided": lambda total: list(range(3, total, 4)),
            "list": lambda total: [17, 2, total - 1, 2, 30, 0]}


# ----------------------------------------------------------------------------- 1. crops
@pytest.mark.parametrize("draw,id_base", [(0, 0), (5, 7), (0, 7), (5, 0)])
@pytest.mark.parametrize("Cn", [1, 2, 3])
def test_randn_field_is_the_crop_of_the_sample_stream(Cn, draw, id_base):
    """W = 57 is odd: the stream index of a tile row's first element takes every residue mod 4, so a group is one
    Philox block or straddles two at every offset; patch 16: one 16-byte store per group"""
    plan = _plan(16, 8)
    assert plan.total == 56 and {int(x) % 4 for x in plan.patch_start[:, 2]} == {0, 1}     # (the shifted last column: 41)
    for name, make in ID_LISTS.items():
        ids = make(plan.total)
        got = plan.randn_field(ids, Cn, SEED, draw, id_base)
        assert got.shape == (len(ids), Cn, 16, 16) and got.data_ptr() % 16 == 0
        assert same_bits(got, T.crops(plan, ids, Cn, SEED, draw, id_base)), name
    assert plan.randn_field([], Cn, SEED, draw, id_base).shape == (0, Cn, 16, 16)


# ----------------------------------------------------------------------------- 2. the scalar path
@pytest.mark.parametrize("patch,grid", [(6, 4), (10, 6)])
@pytest.mark.parametrize("Cn", [1, 3])
def test_randn_field_scalar_stores(patch, grid, Cn):
    """pw % 4 = 2: the last group of every tile row is ragged, and ends inside its first Philox block or in the second"""
    plan = _plan(patch, grid)
    for draw, id_base in ((0, 0), (5, 7)):
        for name, make in ID_LISTS.items():
            ids = make(plan.total)
            assert same_bits(plan.randn_field(ids, Cn, SEED, draw, id_base), T.crops(plan, ids, Cn, SEED, draw, id_base)), name


@pytest.mark.parametrize("patch,grid", [(16, 8), (6, 4)])
def test_randn_field_into_an_unaligned_view(patch, grid):
    """`out` one float past a 16-byte boundary: scalar stores whatever pw is; the floats around the view stay NaN"""
    import ctypes as C
    from diffsplitting_amd._lib import check, lib
    plan = _plan(patch, grid)
    Cn, first, stride, count = 2, 1, 3, (plan.total - 1 + 2) // 3
    n = count * Cn * patch * patch
    buf = torch.full((n + 9,), float("nan"), device="cuda")
    view = buf[5:5 + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    check(lib.dsx_tileplan_randn(plan.handle, Cn, first, stride, count, C.c_uint64(SEED), C.c_uint64(7), C.c_uint32(5), view,
                                 None))
    ids = list(range(first, plan.total, stride))
    assert len(ids) == count
    assert same_bits(view.view(count, Cn, patch, patch), T.crops(plan, ids, Cn, SEED, 5, 7))
    assert bool(torch.isnan(buf[:5]).all()) and bool(torch.isnan(buf[5 + n:]).all())


# ----------------------------------------------------------------------------- 3. what it is for
def test_tiles_of_a_frame_share_the_bits_of_their_overlap():
    plan = _plan(16, 8)
    Cn = 2
    N, H, W = plan.data_shape
    tiles = plan.randn_field(range(plan.total), Cn, SEED, 3, 0).cpu().numpy().view(np.int32)
    canvas = np.zeros((N, Cn, H, W), np.int32)
    seen = np.zeros((N, Cn, H, W), bool)
    compared = 0
    for i in range(plan.total):
        n, y, x = (int(v) for v in plan.patch_start[i])
        have, bits = seen[n, :, y:y + 16, x:x + 16], canvas[n, :, y:y + 16, x:x + 16]
        assert np.array_equal(bits[have], tiles[i][have]), i          # every pixel an earlier tile drew: the same bits
        compared += int(have.sum())
        bits[...] = tiles[i]
        have[...] = True
    assert compared > plan.total * Cn * 16 * 16 // 2 and seen.all()   # half a patch of overlap in both directions
    # another frame, draw or id_base: other noise at the same place
    per = plan.total // N
    assert tuple(plan.patch_start[0][1:]) == tuple(plan.patch_start[per][1:])
    assert not np.array_equal(tiles[0], tiles[per])
    one = plan.randn_field([0], Cn, SEED, 3, 0)
    for kw in (dict(draw=4), dict(draw=3, id_base=1), dict(draw=3, seed=SEED + 1)):
        other = plan.randn_field([0], Cn, kw.pop("seed", SEED), **kw)
        assert not torch.equal(one, other)
    assert same_bits(plan.randn_field([per], Cn, SEED, 3, 0), plan.randn_field([0], Cn, SEED, 3, 1))   # frame 1 = id 1


# ----------------------------------------------------------------------------- 4. the Gaussian tiled path
@pytest.mark.parametrize("name", list(SOLVERS))
def test_predict_stack_with_a_gaussian_sampler(name):
    """per-tile streams, as for InDI: the driver equals the test's own loop over the batches plus plan.stitch"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS[name]
    plan = stack.plan
    out, plan2 = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED)
    assert plan2 is plan and set(out) == {"mean"} and out["mean"].shape == plan.data_shape + (2,)
    assert bool(torch.isfinite(out["mean"]).all())
    tiles = []
    for i in range(0, plan.total, BATCH):
        chunk = list(range(i, i + BATCH))
        tiles.append(T.run(smp, stack.tiles(chunk)["input"], solver, seed=SEED, sample_ids=chunk))
    assert same_bits(out["mean"], plan.stitch(torch.cat(tiles)))
    again, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED + 1)
    assert not torch.equal(again["mean"], out["mean"])


def test_predict_stack_refusals():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack = T.sr3(), T.stack32()
    with pytest.raises(DsxError, match="noise='field' needs seed"):
        predict_stack(smp, stack, noise="field")
    with pytest.raises(DsxError, match="noise = 'frames'"):
        predict_stack(smp, stack, noise="frames", seed=1)
    with pytest.raises(DsxError, match="field_noise_bytes = 100000.*solver.*fewer rows.*smaller batch"):
        predict_stack(smp, stack, noise="field", seed=1, batch_tiles=BATCH, field_noise_bytes=100000)   # 11 rows x 32 KiB
    with pytest.raises(DsxError, match="solver: InDISampler is not a Gaussian sampler"):
        predict_stack(T.indi(), stack, solver=SOLVERS["ddim"])
    assert smp.noise_field is None and smp.noise_source is None


# ----------------------------------------------------------------------------- 5. the field through the driver
@pytest.mark.parametrize("name", list(SOLVERS))
def test_field_noise_through_the_driver(name):
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS[name]
    plan = stack.plan
    assert len(T.stochastic_steps(smp, solver)) == {"dpmpp2m": 0, "ddim": 3, "ancestral": 11}[name]
    state = torch.get_rng_state()
    out, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field")
    assert torch.equal(torch.get_rng_state(), state) and smp.noise_field is None
    want = T.restated_field(smp, stack, solver, BATCH)
    assert same_bits(out["mean"], plan.stitch(want))
    streams, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED)
    assert not torch.equal(streams["mean"], out["mean"])


def test_field_noise_two_samples():
    """sample r takes id_base = r * frames; mean and spread are the float64 Welford of the two restated samples"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["ddim"]
    plan = stack.plan
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", samples=2, return_std=True)
    xs = [T.restated_field(smp, stack, solver, BATCH, id_base=r * plan.data_shape[0]).cpu().numpy() for r in range(2)]
    assert not np.array_equal(xs[0], xs[1])
    mean, std = T.welford(xs)
    assert same_bits(got["mean"], plan.stitch(torch.from_numpy(mean).cuda()))
    assert same_bits(got["std"], plan.stitch(torch.from_numpy(std).cuda())) and bool((got["std"] > 0).any())


# ----------------------------------------------------------------------------- 6. InDI and JointIndi
def test_field_noise_indi():
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG, stack, n = T.indi(), T.stack32(), 3
    plan = stack.plan
    got, _ = predict_stack(netG, stack, batch_tiles=BATCH, num_timesteps=n, seed=SEED, noise="field")
    assert netG.noise_field is None
    tiles = []
    try:
        for i in range(0, plan.total, BATCH):
            chunk = list(range(i, i + BATCH))
            netG.noise_source = Source([T.crops(plan, chunk, 2, SEED, d) for d in range(n + 1)])
            netG.inference(stack.tiles(chunk)["input"], continuous=False, num_timesteps=n)
            assert not netG.noise_source.draws
            tiles.append(netG.last_full_batch.clone())
    finally:
        netG.noise_source = None
    assert same_bits(got["mean"], plan.stitch(torch.cat(tiles)))
    other, _ = predict_stack(netG, stack, batch_tiles=BATCH, num_timesteps=n, seed=SEED + 1, noise="field")
    assert not torch.equal(other["mean"], got["mean"])                # e = 0.01: the draws matter


def test_field_noise_joint_indi():
    """indi1 draws from the field ids of the frames, indi2 from the same ids with bit 39 set"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG, stack, n = T.joint(), T.stack32(), 3
    plan = stack.plan
    got, _ = predict_stack(netG, stack, batch_tiles=BATCH, num_timesteps=n, seed=SEED, noise="field")
    assert netG.noise_field is None and netG.indi1.noise_field is None and netG.indi2.noise_field is None
    tiles = []
    try:
        for i in range(0, plan.total, BATCH):
            chunk = list(range(i, i + BATCH))
            netG.noise_source = Source([T.crops(plan, chunk, 1, SEED, d, id_base=bit)
                                        for bit in (0, netG.STREAM2_BIT) for d in range(n + 1)])
            netG.inference(stack.tiles(chunk)["input"], continuous=False, num_timesteps=n)
            assert not netG.noise_source.draws
            tiles.append(netG.last_full_batch.clone())
    finally:
        netG.noise_source = netG.indi1.noise_source = netG.indi2.noise_source = None
    assert same_bits(got["mean"], plan.stitch(torch.cat(tiles)))


# ----------------------------------------------------------------------------- 7. split, end to end
def test_split_end_to_end(tmp_path):
    """three fresh processes at once: the flagged run twice (byte for byte the same file) and once without --noise-field"""
    cfg = {"name": "tiny_sr3", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 32, "max_qval": 0.98, "upper_clip": False, "train": {"name": "Hagen"},
                        "val": {"name": "Hagen"}},
           "model": {"which_model_G": "sr3", "loss_type": "l1", "finetune_norm": False,
                     "unet": {"in_channel": 3, "out_channel": 2, "inner_channel": 16, "norm_groups": 16,
                              "channel_multiplier": [1, 2], "attn_res": [], "res_blocks": 1, "dropout": 0},
                     "beta_schedule": {"train": SCHED, "val": SCHED},
                     "diffusion": {"image_size": 32, "channels": 2, "conditional": True}}}
    cfg_path = str(tmp_path / "tiny_sr3.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "diffsplitting_amd.split", "-c", cfg_path, "-p", "val", "-gpu", "0", "--synthetic", "1,64,64",
            "--solver", "dpmpp2m", "--solver-steps", "4", "--sample-seed", "3", "--batch-tiles", "3"]
    runs = {"a": ["--noise-field"], "b": ["--noise-field"], "streams": []}
    procs = {}
    for name, extra in runs.items():
        root = tmp_path / name
        root.mkdir()
        procs[name] = subprocess.Popen(base + extra + ["-rootdir", str(root), "--out", str(root / "pred.npy")], env=env,
                                       cwd=str(root), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for name, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-3000:])
        if name == "a":
            assert "dpmpp2m over 4 of the 12 trained timesteps" in log, log[-3000:]
    data = {name: open(tmp_path / name / "pred.npy", "rb").read() for name in runs}
    pred = np.load(tmp_path / "a" / "pred.npy")
    assert pred.shape == (1, 64, 64, 2) and pred.dtype == np.float32 and np.isfinite(pred).all()
    assert data["a"] == data["b"] and data["a"] != data["streams"]


# ----------------------------------------------------------------------------- 8. the seam property
def test_field_noise_narrows_the_seams():
    """ddim, eta = 0, 4 rows, one (1, 64, 96) frame of smooth input, all 15 tiles in one batch: a tile's result then is a
    function of its input tile and its initial noise.  With the field two neighbours start from the same noise on
    their overlap and differ only through GroupNorm statistics and the zero padding at the tile border.

    The bound on rms_field / rms_streams is twice the ratio of the float64 oracle (oracle/unet.py under the recurrence
    of tests/solver_ref.py) on the same weights, input and noise, and never above 1; the factor 2 is for fp32 and the
    planner's choice of kernels.  Measured on one MI355X: field 0.320729, streams 1.288142, ratio 0.248986; the oracle
    gives the same six digits (largest |device - oracle| over the tiles 4.3e-6), so the bound is 0.498."""
    from diffsplitting_amd import engine
    from oracle import unet as oracle_unet
    from tests import solver_ref
    smp = T.sr3()
    stack = T.stack((1, 64, 96), 32, 16, seed=2)
    plan = stack.plan
    ids = list(range(plan.total))
    assert plan.total == 15 and all(int(v) % 8 == 0 for v in plan.patch_start[:, 1:].reshape(-1))   # no shifted tile
    solver = dict(solver="ddim", steps=4, eta=0.0, spacing=None)
    x = stack.tiles(ids)["input"]
    start = {"field": plan.randn_field(ids, 2, SEED, 0), "streams": engine.randn_samples((15, 2, 32, 32), SEED, ids, 0)}
    assert same_bits(start["field"], T.crops(plan, ids, 2, SEED, 0))
    try:
        smp.noise_field = lambda shape, draw: plan.randn_field(ids, shape[1], SEED, draw)
        got = {"field": T.run(smp, x, solver).cpu().numpy()}
    finally:
        smp.noise_field = None
    got["streams"] = T.run(smp, x, solver, seed=SEED, sample_ids=ids).cpu().numpy()
    # the float64 oracle on the same weights, input tiles and initial noise
    table = smp.solver_table(**solver)
    sd64 = {k: v.double() for k, v in smp.weights.items()}
    cond = x.cpu().numpy().astype(np.float64)

    def net(k, state):
        time = torch.full((state.shape[0], 1), float(table.tcond[k]), dtype=torch.float64)
        inp = torch.from_numpy(np.concatenate([cond, state], axis=1))
        return oracle_unet.unet_forward(sd64, TINY, "sr3", inp, time).numpy()
    want = {k: solver_ref.run(table.columns(), v.cpu().numpy().astype(np.float64), net, clip=True, dtype=np.float64)[0][-1]
            for k, v in start.items()}
    rms = {k: T.seam_rms(plan, got[k])[0] for k in got}
    rms64 = {k: T.seam_rms(plan, want[k])[0] for k in want}
    assert T.seam_rms(plan, got["field"])[1] == 12                     # 3 rows of tiles, 4 seams each
    ratio, ratio64 = rms["field"] / rms["streams"], rms64["field"] / rms64["streams"]
    print(f"\nseam rms over 12 seams: field {rms['field']:.6f}, streams {rms['streams']:.6f}, ratio {ratio:.6f}; "
          f"float64 oracle: field {rms64['field']:.6f}, streams {rms64['streams']:.6f}, ratio {ratio64:.6f}")
    print("largest |device - oracle| over the tiles:", {k: float(np.abs(got[k] - want[k]).max()) for k in got})
    assert ratio64 < 1.0
    assert rms["field"] < rms["streams"]
    assert ratio <= min(1.0, 2.0 * ratio64)
