"""dsx_consistency on the device (`-m gpu`): map, conditioned mean and spread against the float64 restatement
(tests/consistency_ref.py) bit for bit, counts, min and max exact, sums within the derived bound; the same bits run to
run, on either load path, for a frame alone and inside a call of three, in place and out of place; the drivers
(predict_stack, predict_stack_frames, two ranks) and the `split --input` command line end to end.

Grid cap: a frame is cut into at most 1024 workgroups of 256 threads (kConMaxBlocks, csrc/dsx_consistency.hip; 4096
pixels per workgroup below the cap), frames are the grid's second dimension (at most 65535, the entry point's limit).
`test_one_launch_past_the_workgroup_cap` runs a frame of 2049 x 2049 = 4 198 401 pixels > 1024 * 4096, where every
workgroup walks more than its four groups per thread."""
import json

import numpy as np
import pytest
import torch

from tests import consistency_ref as ref
from tests import nets
from tests.bits import same_bits
from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu
SLOTS = 10
# (pix, C, clip, std): every value of each appears, with neighbours that differ
COMBOS = [("u16", 2, "off", "given"), ("u8", 1, "on", "none"), ("f32", 3, "all", "zero"), ("u16", 4, "on", "huge"),
          ("u8", 3, "off", "given"), ("f32", 2, "on", "given"), ("u16", 1, "all", "given"), ("f32", 4, "off", "none"),
          ("u8", 2, "all", "huge"), ("u16", 3, "on", "zero"), ("u8", 4, "on", "given"), ("f32", 1, "off", "huge")]
PIX_CODE = {"u8": 0, "u16": 1, "f32": 3}


def _shifted(host, shift):
    """the array on the device, its base moved by `shift` elements (a contiguous view into a larger buffer)"""
    flat = np.ascontiguousarray(host).reshape(-1)
    if flat.dtype == np.uint16:
        flat = flat.view(np.int16)                                      # torch's portable 16-bit storage
    buf = torch.empty(flat.size + shift, dtype=torch.from_numpy(flat[:1]).dtype, device="cuda")
    buf[shift:] = torch.from_numpy(flat).cuda()
    return buf[shift:]


def _run(k, pix, shift=0, in_place=False, frames=None, report=True, want=("map", "mean", "std")):
    """one call of the entry point on the case `k` (frames = slice of its frames) -> dict of numpy outputs"""
    from diffsplitting_amd import _lib
    sl = slice(None) if frames is None else frames
    x, mean, std = k["x"][sl], k["mean"][sl], None if k["std"] is None else k["std"][sl]
    n, plane, C = x.shape[0], x.shape[1], mean.shape[-1]
    dx, dm = _shifted(x, shift), _shifted(mean, shift)
    ds = None if std is None else _shifted(std, shift)
    f32 = lambda count: torch.full((count + shift,), np.nan, dtype=torch.float32, device="cuda")[shift:]
    fmap = f32(n * plane) if "map" in want else None
    om = (dm if in_place else f32(n * plane * C)) if "mean" in want else None
    os_ = (ds if in_place else f32(n * plane * C)) if ("std" in want and std is not None) else None
    rows = part = None
    if report:
        blocks = _lib.check(_lib.lib.dsx_consistency_blocks(plane))
        rows = torch.full((n, SLOTS), np.nan, dtype=torch.float64, device="cuda")
        part = torch.empty((n, blocks, SLOTS), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.dsx_consistency(dx, PIX_CODE[pix], dm, ds, n, plane, C, k["a"], k["b"], k["w"], float(k["clip"]),
                                        float(k["noise_var"]), fmap, om, os_, rows, part, None))
    torch.cuda.synchronize()
    host = lambda t, shape: None if t is None else t.cpu().numpy().reshape(shape)
    return {"map": host(fmap, (n, plane)), "out_mean": host(om, (n, plane, C)), "out_std": host(os_, (n, plane, C)),
            "rows": host(rows, (n, SLOTS))}


def _equal(a, b):
    return all((a[n] is None and b[n] is None) or ref.same_bits(a[n], b[n]) for n in ("map", "out_mean", "out_std", "rows"))


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("plane", [37 * 41, 8 * 12, 130 * 129, 64 * 96])
def test_kernel_equals_the_restatement_and_repeats_its_bits(plane, frames):
    """37 x 41: odd, the scalar path; 8 x 12 and 64 x 96: the vector path (one and two workgroups) against the scalar path
    of the shifted bases; 130 x 129: five workgroups, plane % 4 == 2.  Every combo of COMBOS on each."""
    for pix, C, clip, std in COMBOS:
        k = ref.case(pix, frames, plane, C, seed=7, clip=clip, std=std)
        want = ref.restate(**k)
        got = _run(k, pix)
        where = (pix, C, clip, std)
        for name in ("map", "out_mean", "out_std"):
            assert (got[name] is None) == (want[name] is None), where
            assert got[name] is None or ref.same_bits(got[name], want[name]), (where, name)
        exact = [0, 1, 6, 8, 9]
        assert np.array_equal(got["rows"][:, exact], want["rows"][:, exact]), (where, got["rows"], want["rows"])
        sums = [2, 3, 4, 5, 7]
        print(where, "max |sum - ref| / bound:",
              np.max(np.abs(got["rows"][:, sums] - want["rows"][:, sums]) / np.maximum(want["bounds"][:, sums], 1e-300)))
        assert ref.rows_agree(got["rows"], want["rows"], want["bounds"]), (where, got["rows"], want["rows"])
        if clip == "all":
            assert got["rows"][-1, 0] == 0 and got["rows"][-1, 8] == np.inf and got["rows"][-1, 9] == -np.inf
        if std == "zero":
            assert ref.same_bits(got["out_mean"], k["mean"]) and ref.same_bits(got["out_std"], k["std"])
            assert not got["rows"][:, 6].any()
        # the same bits: run to run, on the other load path, in place
        assert _equal(_run(k, pix), got), where
        assert _equal(_run(k, pix, shift=1), got), where
        assert _equal(_run(k, pix, in_place=True), got), where
        assert _equal(_run(k, pix, shift=1, in_place=True), got), where
        # a frame alone against the same frame inside the call
        if frames == 3:
            alone = _run(k, pix, frames=slice(1, 2))
            assert all(alone[n] is None or ref.same_bits(alone[n][0], got[n][1]) for n in alone), where
        # fewer outputs change none of the others
        only = _run(k, pix, want=())
        assert only["map"] is None and ref.same_bits(only["rows"], got["rows"]), where
        quiet = _run(k, pix, report=False, want=("map",))
        assert quiet["rows"] is None and ref.same_bits(quiet["map"], got["map"]), where


def test_one_launch_past_the_workgroup_cap():
    from diffsplitting_amd import _lib
    plane = 2049 * 2049
    assert _lib.lib.dsx_consistency_blocks(plane) == 1024 and plane > 1024 * 4096
    k = ref.case("u8", 1, plane, 1, seed=3, clip="on", std="none")
    want = ref.restate(**k)
    got = _run(k, "u8", want=("map",))
    assert ref.same_bits(got["map"], want["map"])
    assert np.array_equal(got["rows"][:, [0, 1, 6, 8, 9]], want["rows"][:, [0, 1, 6, 8, 9]])
    assert got["rows"][0, 0] + got["rows"][0, 1] == plane
    assert ref.rows_agree(got["rows"], want["rows"], want["bounds"]), (got["rows"], want["rows"], want["bounds"])


def test_python_face_reports_in_raw_counts():
    from diffsplitting_amd.core.consistency import consistency
    k = ref.case("u16", 3, 37 * 41, 2, seed=5, clip="all", std="given")
    want = ref.restate(**k)
    nd = {"mean_target": k["b"], "std_target": k["a"]}
    x = torch.from_numpy(k["x"].view(np.int16).reshape(3, 37, 41)).cuda()
    mean, std = (torch.from_numpy(k[n].reshape(3, 37, 41, 2)).cuda() for n in ("mean", "std"))
    rep = consistency(mean, x, nd, weights=k["w"], std=std, clip=k["clip"], noise=1.5, project=True, want_map=True,
                      pix=1)
    assert ref.same_bits(rep["map"].cpu().numpy().reshape(3, -1), want["map"])
    assert ref.same_bits(rep["mean"].cpu().numpy().reshape(3, -1, 2), want["out_mean"])
    assert ref.same_bits(rep["std"].cpu().numpy().reshape(3, -1, 2), want["out_std"])
    assert ref.same_bits(mean.cpu().numpy().reshape(3, -1, 2), k["mean"])                      # the inputs are left alone
    rows = rep["rows"]
    assert ref.rows_agree(rows, want["rows"], want["bounds"])
    f0, tot = rep["frames"][0], rep["total"]
    assert f0["pixels"] == rows[0, 0] and f0["rms"] == np.sqrt(rows[0, 3] / rows[0, 0]) and f0["bias"] == rows[0, 2] / rows[0, 0]
    assert f0["chi2"] == rows[0, 7] / rows[0, 6] and f0["min"] == rows[0, 8] and f0["max"] == rows[0, 9]
    assert rep["frames"][2]["pixels"] == 0 and rep["frames"][2]["rms"] is None and rep["frames"][2]["saturated"] == 37 * 41
    k_tot = rows[0, 0] + rows[1, 0] + rows[2, 0]
    assert tot["pixels"] == k_tot and tot["rms"] == np.sqrt(((rows[0, 3] + rows[1, 3]) + rows[2, 3]) / k_tot)
    # no spread, no noise: the orthogonal projection; the recomputed residual vanishes to fp32 rounding of the outputs
    flat = consistency(mean, x, nd, weights=k["w"], clip=None, project=True, pix=1)
    assert "std" not in flat and "chi2" not in flat["total"]
    again = consistency(flat["mean"], x, nd, weights=k["w"], clip=None, pix=1)
    assert again["total"]["rms"] < 1e-3 * flat["total"]["rms"]


# ----------------------------------------------------------------------------- drivers
SHAPE, PATCH, GRID, BATCH, STEPS, SEED, CLIP = (2, 64, 96), 64, 32, 4, 2, 11, 5000.0


@pytest.fixture(scope="module")
def world():
    """The tiny InDI network with the golden weights, a synthetic uint16 acquisition of two frames with some counts
    above the input clip, and the three-sample prediction every driver test compares with (computed once)."""
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames
    from diffsplitting_amd.model import networks
    from tests.util import golden_state_dict
    torch.set_grad_enabled(False)
    sd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()})
    s = np.random.default_rng(5).integers(0, 6000, SHAPE).astype(np.uint16)
    s[0, 0, 0], s[1, -1, -1] = 0, 65535
    nd = dict(mean_input=np.float64(3000.0), std_input=np.float64(1700.0), mean_target=np.array([1500.0, 1400.0]),
              std_target=np.array([850.0, 800.0]), target0_max=None, target1_max=None, input_max=None)
    stack = InputStackTiledPred(s, PATCH, nd, grid_size=GRID, input_clip=CLIP)
    kw = dict(batch_tiles=BATCH, num_timesteps=STEPS, seed=SEED, samples=3, return_std=True)
    plain, _ = predict_stack(netG, stack, **kw)
    frames, _ = predict_stack_frames(netG, stack, **kw)
    return dict(netG=netG, s=s, nd=nd, stack=stack, kw=kw, plain=plain, frames=frames)


def _check_driver(world, run, plain):
    from diffsplitting_amd.core.consistency import consistency
    stack, w = world["stack"], (1.0, 0.5)
    dev, pix, _, clip = stack.acquisition()
    assert clip == CLIP
    rep, _ = run(consistency=True, consistency_noise=2.0, consistency_weights=w)
    assert set(rep) == {"mean", "std", "consistency"}
    assert same_bits(rep["mean"], plain["mean"]) and same_bits(rep["std"], plain["std"])
    want = consistency(plain["mean"], dev, world["nd"], weights=w, std=plain["std"], clip=clip, noise=2.0, project=True, pix=pix)
    assert np.array_equal(rep["consistency"]["rows"], want["rows"]) and rep["consistency"]["total"] == want["total"]
    assert want["total"]["saturated"] == int((world["s"] >= CLIP).sum()) > 0 and want["total"]["chi2"] > 0
    pro, _ = run(consistency="project", consistency_noise=2.0, consistency_weights=w)
    assert set(pro) == {"mean", "std", "mean_raw", "consistency"}
    assert same_bits(pro["mean_raw"], plain["mean"]) and same_bits(pro["mean"], want["mean"]) and same_bits(pro["std"], want["std"])
    assert not same_bits(pro["mean"], plain["mean"]) and bool((pro["std"] <= plain["std"]).all())
    assert np.array_equal(pro["consistency"]["rows"], want["rows"])                           # the residual BEFORE the projection
    assert "mean" not in pro["consistency"] and "std" not in pro["consistency"]


def test_predict_stack_reports_and_projects(world):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiled_predict import predict_stack
    _check_driver(world, lambda **kw: predict_stack(world["netG"], world["stack"], **world["kw"], **kw), world["plain"])
    with pytest.raises(DsxError, match="consistency='project' with quantiles= / ranks="):
        predict_stack(world["netG"], world["stack"], **world["kw"], consistency="project", quantiles=(0.5,))


def test_predict_stack_frames_reports_and_projects(world):
    from diffsplitting_amd.data.tiled_predict import predict_stack_frames
    _check_driver(world, lambda **kw: predict_stack_frames(world["netG"], world["stack"], **world["kw"], **kw),
                  world["frames"])


def test_two_ranks_report_the_bits_of_one():
    """Two fresh ranks on the one GPU, gloo transport: on every rank the projected canvases and the report rows equal
    core.consistency.consistency applied to the one-rank canvases (the worker checks: tests/multi_rank_consistency.py)."""
    r = run_ranks("multi_rank_consistency.py", 2, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "CONSISTENCY_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_command_line_round_trip(world, tmp_path, monkeypatch):
    from diffsplitting_amd import split
    from diffsplitting_amd.core.consistency import consistency, json_report
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.normalization import save_normalization
    from diffsplitting_amd.data.tiff import imread, imwrite
    from diffsplitting_amd.data.tiled_predict import predict_stack
    cfg = {"name": "tiny_input", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": PATCH, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 0.5],
                        "train": {"name": "Hagen"}, "val": {"name": "Hagen"}},
           "model": nets.hagen64_section()}
    p = lambda name: str(tmp_path / name)
    with open(p("tiny.json"), "w") as f:
        json.dump(cfg, f)
    nd = dict(world["nd"], target0_max=3000.0, target1_max=2800.0, input_max=5800.0)
    save_normalization(p("norm.json"), nd, data_type="Hagen", channel_weights=[1, 0.5], max_qval=0.98, upper_clip=False,
                       target_channel_idx=None)
    imwrite(p("s.tif"), world["s"])
    models = []
    create = split.create_model
    monkeypatch.setattr(split, "create_model", lambda opt: models.append(create(opt)) or models[-1])

    def main(*argv):
        torch.manual_seed(1234)                                       # the model's random initial weights
        return split.main(["-c", p("tiny.json"), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--steps", str(STEPS),
                           "--batch-tiles", str(BATCH), "--sample-seed", str(SEED), "--input", p("s.tif"), "--norm",
                           p("norm.json"), "--input-clip", str(CLIP)] + list(argv))

    main("--samples", "3", "--out", p("a.npy"), "--std-out", p("sd.npy"), "--project", "--consistency-noise", "2",
         "--consistency-report", p("c.json"), "--consistency-map", p("m.tif"))
    stack = InputStackTiledPred(p("s.tif"), PATCH, world["nd"], grid_size=GRID, input_clip=CLIP)
    plain, _ = predict_stack(models[-1].netG, stack, **world["kw"])
    dev, pix, _, clip = stack.acquisition()
    want = consistency(plain["mean"], dev, world["nd"], weights=(1.0, 0.5), std=plain["std"], clip=clip, noise=2.0,
                       project=True, want_map=True, pix=pix)
    doc = json.load(open(p("c.json")))
    assert doc["total"] == json.loads(json.dumps(json_report(want)["total"])) and doc["weights"] == [1.0, 0.5]
    assert doc["frames"] == json.loads(json.dumps(json_report(want)["frames"])) and doc["projected"] is True
    assert doc["noise"] == 2.0 and doc["clip"] == CLIP and doc["total"]["saturated"] > 0
    assert ref.same_bits(imread(p("m.tif")), want["map"].cpu().numpy())
    mean_t = torch.as_tensor(world["nd"]["mean_target"], dtype=torch.float32, device="cuda")
    std_t = torch.as_tensor(world["nd"]["std_target"], dtype=torch.float32, device="cuda")
    assert ref.same_bits(np.load(p("a.npy")), (want["mean"] * std_t + mean_t).cpu().numpy())
    assert ref.same_bits(np.load(p("sd.npy")), (want["std"] * std_t).cpu().numpy())
    # without --project the outputs are the plain ones, the report the same; weights from the command line
    main("--samples", "3", "--out", p("b.npy"), "--consistency-report", p("d.json"), "--consistency-noise", "2",
         "--channel-weights", "1,0.5")
    assert ref.same_bits(np.load(p("b.npy")), (plain["mean"] * std_t + mean_t).cpu().numpy())
    assert json.load(open(p("d.json")))["total"] == doc["total"]
    # one sample: the orthogonal projection, no spread anywhere
    main("--out", p("o.npy"), "--project", "--consistency-report", p("e.json"))
    one, _ = predict_stack(models[-1].netG, stack, batch_tiles=BATCH, num_timesteps=STEPS, seed=SEED)
    flat = consistency(one["mean"], dev, world["nd"], weights=(1.0, 0.5), clip=clip, project=True, pix=pix)
    assert ref.same_bits(np.load(p("o.npy")), (flat["mean"] * std_t + mean_t).cpu().numpy())
    assert "chi2" not in json.load(open(p("e.json")))["total"]
