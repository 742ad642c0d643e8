"""dsx_calibration on the MI355X (`-m gpu`): counts and coverage equal to tests/calibration_ref.py, the sums within its
derived bound, read in place from NaN-poisoned buffers; the bits of a call on either load path, against a contiguous
call and run to run; bin_edges against np.quantile; and the calibration of a tiny InDI network's posterior spread end
to end, through ``split --calibration`` / ``--apply-calibration``."""
import json

import numpy as np
import pytest
import torch

from tests import nets
from tests import calibration_ref as REF
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _span():
    """pixels up to which the canvases are one workgroup, read from dsx_calibration_blocks"""
    from diffsplitting_amd._lib import lib
    lo, hi = 1, 1 << 24
    assert lib.dsx_calibration_blocks(lo) == 1 and lib.dsx_calibration_blocks(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.dsx_calibration_blocks(mid) == 1 else (lo, mid)
    assert lib.dsx_calibration_blocks(2 * lo) == 2 and lib.dsx_calibration_blocks(2 * lo + 1) == 3
    return lo


def _poisoned(x, offset):
    """``x`` (n, C) fp32 on the device as a contiguous view ``offset`` elements into a (256-byte aligned) buffer that is
    NaN wherever the view does not point: offset 0 allows 16-byte loads (when n C % 4 == 0), offset 1 does not."""
    n, C = x.shape
    buf = torch.full((offset + n * C + 8,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[offset:offset + n * C].view(n, C)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    assert int(torch.isnan(buf).sum()) == buf.numel() - n * C
    return view


def _check(n, C, nbins, nz):
    from diffsplitting_amd.core.calibration import calibration_sums
    z = REF.Z_OF[nz]
    for name, (m, s, t) in REF.cases(n, C, seed=nbins + nz).items():
        what = (name, n, C, nbins, nz)
        edges = REF.edges_of(s, nbins)
        ref, bnd = REF.stats(m, s, t, edges, z, with_bounds=True)
        got = []
        for offset in (0, 1):
            dev = calibration_sums(*[_poisoned(x, offset) for x in (m, s, t)], edges, z)
            assert dev.dtype == torch.float64 and dev.is_cuda and dev.shape == ref.shape
            got.append(dev.cpu().numpy())
        plain = [torch.from_numpy(x).cuda() for x in (m, s, t)]
        got.append(calibration_sums(*plain, edges, z).cpu().numpy())
        got.append(calibration_sums(*plain, edges, z).cpu().numpy())
        ints = REF.is_integer_slot(nbins, nz)
        err = np.abs(got[0] - ref)
        worst = np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0))
        print(f"{what}: max err / bound {worst:.3f}")
        assert np.array_equal(got[0][:, ints], ref[:, ints]), what               # counts, coverage: exact
        assert (err <= bnd)[:, ~ints].all(), (what, worst)
        assert got[0][:, 0:3 * nbins:3].sum(axis=1).tolist() == [n] * C
        for other, how in zip(got[1:], ("offset by one element", "contiguous", "second run")):
            assert same_bits(other, got[0]), (what, how)
        if name == "equal" and nbins > 1:
            assert (got[0][:, 0:3 * (nbins - 1):3] == 0).all()                     # every pixel in the last bin


# every n of the partition (one thread, one wave, one workgroup and its neighbours, three workgroups) with C, nbins and
# nz rotating through their values, then every (C, nbins) pair at one ragged size
SMALL = [(1, 1, 1, 0), (2, 2, 2, 3), (63, 3, 7, 8), (64, 4, 64, 3), (65, 3, 64, 8), (257, 2, 7, 3)]


@pytest.mark.parametrize("n,C,nbins,nz", SMALL)
def test_small_canvases_against_the_restatement(n, C, nbins, nz):
    _check(n, C, nbins, nz)


@pytest.mark.parametrize("which,C,nbins,nz", [("span - 1", 4, 7, 8), ("span", 1, 64, 3), ("span + 1", 2, 2, 0),
                                             ("2 span + 1", 3, 7, 3), ("2 span + 1", 2, 64, 8)])
def test_one_to_three_workgroups(which, C, nbins, nz):
    s = _span()
    _check({"span - 1": s - 1, "span": s, "span + 1": s + 1, "2 span + 1": 2 * s + 1}[which], C, nbins, nz)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_every_channel_count_with_every_bin_count(C):
    for nbins in (1, 2, 7, 64):
        _check(257, C, nbins, 3)


def test_empty_bins_are_nan_in_python_and_shapes_are_checked():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core.calibration import bin_edges, calibration_stats, fit
    m, s, t = (torch.from_numpy(x).cuda().view(3, 5, 7, 2) for x in REF.cases(105, 2, seed=1)["equal"])
    st = calibration_stats(m, s, t, bins=6, z=(1, 2))
    assert st.count.shape == (2, 6) and (st.count[:, :5] == 0).all() and (st.count[:, 5] == 105).all() and st.n == 105
    assert np.isnan(st.rmv[:, :5]).all() and np.isnan(st.rmse[:, :5]).all() and (st.rmv[:, 5] == 0.75).all()
    assert st.coverage.shape == (2, 2) and ((0 < st.coverage) & (st.coverage <= 1)).all()
    line = fit(st)
    assert np.array_equal(line["a"], line["scale"]) and (line["c"] == 0).all()
    with pytest.raises(DsxError, match="of one shape"):
        calibration_stats(m[:2], s, t)
    with pytest.raises(DsxError, match="float32"):
        calibration_stats(m, s.double(), t)
    with pytest.raises(DsxError, match=r"edges of shape \(3, 2\)"):
        calibration_stats(m, s, t, edges=np.zeros((3, 2)))
    with pytest.raises(DsxError, match="bins = 65"):
        bin_edges(s, 65)


@pytest.mark.parametrize("n,C,bins", [(1, 1, 4), (2, 2, 3), (4099, 2, 32), (1000, 3, 64), (257, 4, 30), (64, 1, 1)])
def test_bin_edges_are_np_quantile(n, C, bins):
    from diffsplitting_amd.core.calibration import bin_edges
    for name in ("random", "ties", "wide"):
        s = REF.cases(n, C, seed=3)[name][1]
        got = bin_edges(torch.from_numpy(s).cuda(), bins)
        ref = REF.edges_of(s, bins)
        assert got.dtype == np.float64 and got.shape == (C, bins - 1)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (name, n, C, bins)


# ----------------------------------------------------------------------------- end to end
SHAPE, PATCH, GRID, BATCH, STEPS, SEED = (2, 64, 96), 64, 32, 4, 2, 11


def test_the_posterior_spread_of_a_tiny_network_end_to_end(tmp_path, monkeypatch):
    from diffsplitting_amd import split
    from diffsplitting_amd.core.calibration import Calibration
    from diffsplitting_amd.core.metrics import calculate_calibration
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    rng = np.random.default_rng(21)
    c0, c1 = (rng.integers(0, 3000, SHAPE).astype(np.float32) for _ in range(2))
    cfg = {"name": "tiny_cal", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": PATCH, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 1],
                        "train": {"name": "Hagen"}, "val": {"name": "Hagen"}},
           "model": nets.hagen64_section()}
    p = lambda name: str(tmp_path / name)
    with open(p("tiny.json"), "w") as f:
        json.dump(cfg, f)
    np.save(p("both.npy"), np.stack([c0, c1], axis=-1))
    models = []
    create = split.create_model
    monkeypatch.setattr(split, "create_model", lambda opt: models.append(create(opt)) or models[-1])

    def main(*argv):
        torch.manual_seed(1234)                                       # the model's random initial weights
        return split.main(["-c", p("tiny.json"), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--steps", str(STEPS),
                           "--batch-tiles", str(BATCH), "--sample-seed", str(SEED), "--frames", p("both.npy"),
                           "--samples", "3"] + list(argv))

    main("--out", p("mean.npy"), "--std-out", p("std.npy"), "--calibration", p("cal.json"), "--calibration-bins", "8")
    two = SplitDatasetTiledPred("Hagen", DataLocation(arrays=(c0, c1)), PATCH, grid_size=GRID, max_qval=0.98,
                                channel_weights=[1, 1])
    want, _ = predict_stack(models[-1].netG, two, samples=3, return_std=True, batch_tiles=BATCH, num_timesteps=STEPS, seed=SEED)
    assert want["std"].shape == SHAPE + (2,) and (want["std"] > 0).any()
    # the Python face on the very tensors against the restatement
    gt = two.normalized_target_frames()
    st = calculate_calibration(gt, want["mean"], want["std"], bins=8)
    host = [x.cpu().numpy().reshape(-1, 2) for x in (want["mean"], want["std"], gt)]
    edges = REF.edges_of(host[1], 8)
    assert np.array_equal(st.edges.view(np.uint64), edges.view(np.uint64))
    ref, bnd = REF.stats(*host, edges, (1.0, 2.0, 3.0), with_bounds=True)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    assert st.n == n and np.array_equal(st.count, ref[:, 0:24:3]) and np.array_equal(st.covered, ref[:, 24:])
    assert (np.abs(st.sv - ref[:, 1:24:3]) <= bnd[:, 1:24:3]).all() and (np.abs(st.se - ref[:, 2:24:3]) <= bnd[:, 2:24:3]).all()
    assert np.array_equal(st.coverage, ref[:, 24:] / n)
    assert (st.count > 0).all()
    assert np.array_equal(st.rmv, np.sqrt(st.sv / st.count)) and np.array_equal(st.rmse, np.sqrt(st.se / st.count))
    # what split wrote: the same curve, bit for bit, with its fit, the sample count and std_target
    cal = Calibration.load(p("cal.json"))
    mine = Calibration.from_stats(st, 3)
    for k in ("edges", "sv", "se", "rmv", "rmse", "coverage", "count", "covered"):
        assert np.array_equal(getattr(cal.stats, k), getattr(st, k)), k
    assert np.array_equal(cal.a, mine.a) and np.array_equal(cal.c, mine.c) and np.array_equal(cal.scale, mine.scale)
    nd = two.get_normalization_dict()
    assert (cal.samples, cal.channels) == (3, 2) and np.array_equal(cal.std_target, np.asarray(nd["std_target"]).reshape(-1))
    std_t = torch.as_tensor(np.asarray(nd["std_target"]).reshape(-1), dtype=torch.float32, device="cuda")
    same = lambda path, t: np.array_equal(np.load(path).view(np.int32), t.cpu().numpy().view(np.int32))
    assert same(p("std.npy"), want["std"] * std_t)
    # --apply-calibration changes the spread file to apply(std) * std_target and nothing else
    main("--out", p("mean2.npy"), "--std-out", p("std2.npy"), "--apply-calibration", p("cal.json"))
    assert np.array_equal(np.load(p("mean2.npy")).view(np.int32), np.load(p("mean.npy")).view(np.int32))
    assert same(p("std2.npy"), cal.apply(want["std"]) * std_t)
    assert not same(p("std2.npy"), want["std"] * std_t)
    with pytest.raises(SystemExit, match="--apply-calibration .*--std-out"):
        main("--apply-calibration", p("cal.json"))
