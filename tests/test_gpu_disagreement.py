"""Tile disagreement on the MI355X (`-m gpu`): dsx_tileplan_disagreement against the numpy restatement of its contract
(tests/disagreement_ref.py) -- map bits, counts and min / max equal, sums within the derived bound -- on ragged plans with
pw % 4 = 2, up to 12 contributors and a single tile, C = 1..4, band 1 and 8; tiles that agree; the rank-slot layouts
against the one-rank bits; an unaligned map; no map; past each grid cap; and the drivers: ``predict_stack`` under crop and
blend, the frame-state paths against their last ``keep_tiles`` entry, ``split --seam-report`` end to end, 1..3 ranks."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import blend_ref
from tests import disagreement_ref as ref
from tests import tiled_util as T
from tests.bits import same_bits
from tests.rank_worker import run_ranks
from tests.tiled_util import BATCH, BLEND_PLANS, SEED, SOLVERS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SINGLE = ((1, 32, 32), 32, 32)
KEYS = ("count", "sum_var", "min_var", "max_var", "rms_pair")


def _np(d):
    return {k: d[k].cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _variance(shape, patch, grid, Cn):
    """the restatement's per-pixel variance, computed once per (plan, C) and shared: read only"""
    plan = T.plan_of(shape, patch, grid)
    tiles = T.random_tiles(plan, Cn)
    var, k = ref.variance(plan, tiles)
    var.setflags(write=False)
    return tiles, var, k


def _check(plan, got, var, k, band):
    """the contract, figure by figure"""
    want_map = np.sqrt(var).astype(np.float32)
    want = ref.scores(var, k, *ref.near_masks(plan, band))
    g = _np(got)
    assert got["map"].shape == var.shape and got["map"].dtype == torch.float32
    assert same_bits(got["map"].cpu(), torch.from_numpy(want_map))
    assert g["count"].dtype == np.int64 and np.array_equal(g["count"], want["count"])
    assert same_bits(torch.from_numpy(g["min_var"]), torch.from_numpy(want["min_var"]))
    assert same_bits(torch.from_numpy(g["max_var"]), torch.from_numpy(want["max_var"]))
    err = np.abs(g["sum_var"] - want["sum_var"])
    print(f"\nsum var: largest |device - fsum| / bound = {np.max(err / np.maximum(want['bound'], 1e-300)):.3f}")
    assert (err <= want["bound"]).all()
    assert np.array_equal(np.isnan(g["rms_pair"]), want["count"] == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        own = np.sqrt(2.0 * g["sum_var"] / g["count"])
    assert np.array_equal(g["rms_pair"][g["count"] > 0], own[g["count"] > 0])
    assert ref.within_contract(got["map"].cpu().numpy(), g, want_map, want)


# ----------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("Cn", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_disagreement_is_its_restatement(shape, patch, grid, Cn):
    plan = T.plan_of(shape, patch, grid)
    tiles, var, k = _variance(shape, patch, grid, Cn)
    dev = torch.from_numpy(tiles).cuda()
    for band in (1, 8):
        got = plan.disagreement(dev, band=band)
        _check(plan, got, var, k, band)
        if (shape, patch, grid) == SINGLE:
            assert not got["count"].any() and torch.isnan(got["rms_pair"]).all() and not got["map"].any()
            assert torch.isposinf(got["min_var"]).all() and torch.isneginf(got["max_var"]).all()
        else:
            assert (got["count"] > 0).all() and (got["map"] > 0).any()
        again = plan.disagreement(dev, band=band)                     # a second call: the same bits
        assert same_bits(again["map"], got["map"]) and same_bits(again["partials"], got["partials"])
        sums = plan.disagreement(dev, band=band, want_map=False)      # no map: the same rows
        assert sums["map"] is None and same_bits(sums["partials"], got["partials"])
        assert tuple(got["partials"].shape) == (shape[0], plan.blend_blocks(), Cn, 8)
        assert not got["partials"][..., 6:].any()


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_tiles_cut_from_one_frame_do_not_disagree(shape, patch, grid):
    plan = T.plan_of(shape, patch, grid)
    for Cn in (1, 2, 3, 4):
        frame = np.random.default_rng(Cn).standard_normal(plan.data_shape + (Cn,)).astype(np.float32)
        got = plan.disagreement(torch.from_numpy(blend_ref.cut_tiles(plan, frame)).cuda())
        assert not got["map"].any() and not got["sum_var"].any()
        if plan.total > 1:
            assert (got["count"] > 0).all() and not got["rms_pair"].any() and not got["max_var"].any()
        else:
            assert not got["count"].any() and torch.isnan(got["rms_pair"]).all()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS[:4], ids=str)
def test_the_rank_slot_layouts_give_the_one_rank_bits(shape, patch, grid, world):
    plan = T.plan_of(shape, patch, grid)
    for Cn in (1, 2, 3, 4):
        tiles = _variance(shape, patch, grid, Cn)[0]
        one = plan.disagreement(torch.from_numpy(tiles).cuda())
        buf = blend_ref.slots(plan, tiles, world)
        assert np.isnan(buf).any() or plan.total % world == 0
        got = plan.disagreement(torch.from_numpy(buf).cuda(), world=world, Cn=Cn)
        assert same_bits(got["map"], one["map"]) and same_bits(got["partials"], one["partials"]), Cn


@pytest.mark.parametrize("Cn", [1, 2, 4])
def test_a_map_in_an_unaligned_view(Cn):
    """the map one float past a 16-byte boundary: one dword per channel whatever C is; its NaN neighbours stay NaN"""
    shape, patch, grid = BLEND_PLANS[0]
    plan = T.plan_of(shape, patch, grid)
    tiles = torch.from_numpy(_variance(shape, patch, grid, Cn)[0]).cuda()
    want = plan.disagreement(tiles)
    n = want["map"].numel()
    buf = torch.full((n + 8,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + n].view(want["map"].shape)
    got = plan.disagreement(tiles, out=view)
    assert got["map"].data_ptr() == view.data_ptr() and same_bits(view, want["map"])
    assert same_bits(got["partials"], want["partials"])
    assert torch.isnan(buf[0]) and torch.isnan(buf[1 + n:]).all() and not torch.isnan(buf[1:1 + n]).any()


@pytest.mark.parametrize("shape", [(1, 150, 40), (1, 24, 300)], ids=str)
def test_once_past_each_grid_cap(shape):
    """150 rows: more than the 128 row slots, a workgroup strides over two rows; 300 columns: two 256-column segments"""
    plan = T.plan_of(shape, 16, 8)
    assert plan.blend_blocks() == (128 if shape[1] > 128 else shape[1]) * (2 if shape[2] > 256 else 1)
    tiles, var, k = _variance(shape, 16, 8, 2)
    for band in (1, 8):
        _check(plan, plan.disagreement(torch.from_numpy(tiles).cuda(), band=band), var, k, band)


def test_python_refusals():
    from diffsplitting_amd._lib import DsxError
    plan = T.plan_of(*BLEND_PLANS[0])
    tiles = torch.zeros((plan.total, 5) + plan.patch_shape[1:], device="cuda")
    with pytest.raises(DsxError, match="disagreement: C = 5, must be in 1..4"):
        plan.disagreement(tiles)
    with pytest.raises(DsxError, match="disagreement needs every tile of the plan"):
        plan.disagreement(tiles[:3, :2])
    with pytest.raises(DsxError, match="tileplan_disagreement: band = 0"):
        plan.disagreement(tiles[:, :2].contiguous(), band=0)
    with pytest.raises(DsxError, match="disagreement: out must be a contiguous float32 CUDA tensor of shape"):
        plan.disagreement(tiles[:, :2].contiguous(), out=torch.zeros(3, device="cuda"))


# ----------------------------------------------------------------------------- 2. the drivers
def _same_scores(got, want, maps=True):
    for key in KEYS + (("map",) if maps else ()):
        assert same_bits(got[key], want[key]), key


@pytest.mark.parametrize("stitch", ["crop", "blend"])
def test_predict_stack_measures_the_tiles_of_its_own_loop(stitch):
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["dpmpp2m"]
    plan = stack.plan
    kw = dict(batch_tiles=BATCH, solver=solver, seed=SEED, stitch=stitch, window="hann")
    plain, _ = predict_stack(smp, stack, **kw)
    assert "disagreement" not in plain
    got, _ = predict_stack(smp, stack, disagreement=True, seam_band=3, **kw)
    assert same_bits(got["mean"], plain["mean"])
    tiles = torch.cat([T.run(smp, stack.tiles(list(range(i, i + BATCH)))["input"], solver, seed=SEED,
                             sample_ids=list(range(i, i + BATCH))) for i in range(0, plan.total, BATCH)])
    want = plan.disagreement(tiles, band=3)
    _same_scores(got["disagreement"], want)
    assert (want["count"] > 0).all() and (want["sum_var"] > 0).all()
    sums, _ = predict_stack(smp, stack, disagreement="sums", seam_band=3, **kw)
    assert sums["disagreement"]["map"] is None and same_bits(sums["mean"], plain["mean"])
    _same_scores(sums["disagreement"], want, maps=False)


def test_predict_stack_keeps_mean_and_std_and_measures_the_sample_means():
    """three samples per tile of the InDI sampler: 'mean' and 'std' keep their bits, the measured tiles are the per-tile
    sample means"""
    from diffsplitting_amd import engine
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG, stack = T.indi(), T.stack32()
    plan = stack.plan
    kw = dict(batch_tiles=BATCH, seed=SEED, samples=3, return_std=True)
    plain, _ = predict_stack(netG, stack, **kw)
    got, _ = predict_stack(netG, stack, disagreement=True, **kw)
    for key in plain:
        assert same_bits(got[key], plain[key]), key
    means = []
    for i in range(0, plan.total, BATCH):
        chunk = list(range(i, i + BATCH))
        mean = m2 = None
        for r in range(3):
            netG.inference(stack.tiles(chunk)["input"], continuous=False, seed=SEED,
                           sample_ids=[k + r * plan.total for k in chunk])
            mean, m2 = engine.moments_update(netG.last_full_batch.contiguous(), mean, m2, r)
        means.append(engine.moments_finish(mean, m2, 3, want_std=False)[0])
    _same_scores(got["disagreement"], plan.disagreement(torch.cat(means)))


def test_fused_steps_measure_the_tiles_before_the_last_blend():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiled_predict import fused_sample, predict_stack
    from diffsplitting_amd.data.tiling import fold_disagreement
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["dpmpp2m"]
    plan = stack.plan
    kw = dict(batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", fuse=True)
    plain, _ = predict_stack(smp, stack, **kw)
    got, _ = predict_stack(smp, stack, disagreement=True, **kw)
    assert same_bits(got["mean"], plain["mean"])
    table = smp.solver_table(**solver)
    want = []
    for r in range(2):
        rows = []
        fused_sample(smp, stack, table, BATCH, SEED, r * plan.data_shape[0], keep_tiles=rows)
        want.append(plan.disagreement(rows[-1]))
    _same_scores(got["disagreement"], want[0])
    two, _ = predict_stack(smp, stack, disagreement="sums", samples=2, **kw)
    _same_scores(two["disagreement"], fold_disagreement(fold_disagreement(None, want[0]), want[1]), maps=False)
    assert two["disagreement"].get("map") is None
    assert torch.equal(two["disagreement"]["count"], 2 * want[0]["count"])
    with pytest.raises(DsxError, match="disagreement=True on fuse=True with samples = 2"):
        predict_stack(smp, stack, disagreement=True, samples=2, **kw)


def test_frame_diffusion_measures_the_x0_tiles_of_the_last_row():
    from diffsplitting_amd.data.tiled_predict import frame_sample, input_frames, predict_stack_frames
    netG, stack = T.indi(), T.stack32()
    plan = stack.plan
    kw = dict(batch_tiles=BATCH, seed=SEED)
    plain, _ = predict_stack_frames(netG, stack, **kw)
    got, _ = predict_stack_frames(netG, stack, disagreement=True, seam_band=4, **kw)
    assert same_bits(got["mean"], plain["mean"])
    plan.set_window("triangle")
    rows = []
    frame_sample(netG, stack, input_frames(stack, BATCH), int(netG.num_timesteps), 1.0, BATCH, SEED, 0, keep_tiles=rows)
    assert len(rows) == int(netG.num_timesteps)
    _same_scores(got["disagreement"], plan.disagreement(rows[-1], band=4))


def test_split_seam_report_end_to_end(tmp_path, monkeypatch):
    """`split --seam-report --seam-map` in this process, with the driver's own return value recorded on the way"""
    from diffsplitting_amd import split
    from diffsplitting_amd.data import tiled_predict
    seen = {}
    real = tiled_predict.predict_stack

    def recording(netG, val_set, **kw):
        out, plan = real(netG, val_set, **kw)
        seen.update(netG=netG, val_set=val_set, kw=kw, out=out, plan=plan)
        return out, plan
    monkeypatch.setattr(tiled_predict, "predict_stack", recording)
    cfg = {"name": "tiny_sr3", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 32, "max_qval": 0.98, "upper_clip": False, "train": {"name": "Hagen"},
                        "val": {"name": "Hagen"}},
           "model": {"which_model_G": "sr3", "loss_type": "l1", "finetune_norm": False,
                     "unet": {"in_channel": 3, "out_channel": 2, "inner_channel": 16, "norm_groups": 16,
                              "channel_multiplier": [1, 2], "attn_res": [], "res_blocks": 1, "dropout": 0},
                     "beta_schedule": {"train": T.SCHED, "val": T.SCHED},
                     "diffusion": {"image_size": 32, "channels": 2, "conditional": True}}}
    p = lambda name: str(tmp_path / name)
    with open(p("tiny.json"), "w") as f:
        json.dump(cfg, f)
    argv = ["-c", p("tiny.json"), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--synthetic", "1,64,64", "--solver",
            "dpmpp2m", "--solver-steps", "4", "--sample-seed", "3", "--batch-tiles", "3", "--samples", "2"]
    torch.manual_seed(1234)                                          # the model's random initial weights
    pred = split.main(argv + ["--seam-report", p("seam.json"), "--seam-map", p("seam.npy"), "--seam-band", "4"])
    assert seen["kw"]["disagreement"] is True and seen["kw"]["seam_band"] == 4
    dis, plan, val_set = seen["out"]["disagreement"], seen["plan"], seen["val_set"]
    assert same_bits(pred, seen["out"]["mean"])
    want, _ = real(seen["netG"], val_set, **seen["kw"])               # the driver again: the same figures
    _same_scores(want["disagreement"], dis)
    std = np.asarray(val_set.get_normalization_dict()["std_target"], dtype=np.float64).reshape(-1)
    smap = np.load(p("seam.npy"))
    raw = (dis["map"] * torch.as_tensor(std, dtype=torch.float32, device="cuda")).cpu().numpy()
    assert smap.dtype == np.float32 and smap.shape == (1, 64, 64, 2) and np.array_equal(smap, raw) and (smap > 0).any()
    doc = json.load(open(p("seam.json")))
    assert (doc["band"], doc["stitch"], doc["tiles"], doc["patch"], doc["grid"], doc["samples"]) == (4, "crop", plan.total, 32, 16, 2)
    assert doc["measured"] == "per-tile mean of 2 samples" and len(doc["channels"]) == 2
    count, sums = dis["count"].sum(dim=0).cpu().numpy(), dis["sum_var"].sum(dim=0).cpu().numpy()
    for c, ch in enumerate(doc["channels"]):
        assert (ch["overlap_pixels"], ch["band_pixels"]) == (int(count[c, 0]), int(count[c, 1]))
        assert 0 < ch["band_pixels"] < ch["overlap_pixels"]
        for j, key in enumerate(("rms_pair_overlap", "rms_pair_band")):
            rms = float(np.sqrt(2.0 * sums[c, j] / count[c, j]))
            assert ch[key] == {"normalised": rms, "raw": float(rms * std[c])}
        largest = float(dis["map"][..., c].max().item())
        assert ch["largest_s"] == {"normalised": largest, "raw": float(largest * std[c])}
    torch.manual_seed(1234)
    again = split.main(argv)                                           # without the flags: as before
    assert same_bits(again, pred) and "disagreement" not in seen["out"]


@pytest.mark.parametrize("world", [2, 3])
def test_the_measure_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks, gloo transport: under crop and under blend every rank's figures equal, bitwise, those of the
    one-rank tiles restated in its own process, and 'mean' keeps the bits of the call without the option
    (tests/multi_rank_predict_disagreement.py).  One rank is test_predict_stack_measures_the_tiles_of_its_own_loop: the
    same comparison, in this process."""
    r = run_ranks("multi_rank_predict_disagreement.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_DISAGREEMENT_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
