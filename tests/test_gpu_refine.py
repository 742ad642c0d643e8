"""Refining the mixing time from the split itself on the MI355X (`-m gpu`): estimate_time_from_estimates against the
restatement of tests/comoments_ref.py and against the torch loop it replaces, and predict_tiled_refined -- with oracle
samplers (the true channels as estimates: the planted mixing time must come back), with the tiny random-weight networks
of tests/test_gpu_mixed.py (rounds = 0 is predict_tiled_mixed bit for bit; every later round's start times are the
argmax rule applied to the reported moments; an all-NaN unit keeps its time), and over 1, 2 and 3 ranks."""
import types

import numpy as np
import pytest
import torch

from tests import comoments_ref as CR
from tests import mixed_util as MU
from tests.bits import same_bits
from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T_LIST = np.arange(0, 1.0, 0.05)


def test_estimate_time_from_estimates_matches_the_restatement():
    from diffsplitting_amd.core.psnr_based_t_refinement import estimate_time_from_estimates
    g, p1, p2 = CR.planted((4, 33, 130), seed=0)
    g[3] = 1.25                                                        # a constant input: its curve is NaN
    dev = lambda x: torch.from_numpy(x[:, None]).cuda()
    per_t, cons, curves, t_star = estimate_time_from_estimates(dev(g), dev(p1), dev(p2))
    m, mb = CR.moments(g, p1, p2, with_bounds=True)
    c, t = CR.curve(m, T_LIST, 1 - T_LIST)
    bound = CR.curve_bound(m, mb, T_LIST, 1 - T_LIST)
    assert curves.shape == (4, 20) and curves.dtype == torch.float64 and curves.is_cuda
    got = curves.cpu().numpy()
    assert np.isnan(got[3]).all() and np.isnan(c[3]).all() and (np.abs(got[:3] - c[:3]) <= bound[:3]).all()
    assert np.array_equal(per_t[:3], T_LIST[c[:3].argmax(axis=1)]) and np.isnan(per_t[3])
    assert (per_t[:3] == T_LIST[6]).all() and cons == T_LIST[6]
    ts = t_star.cpu().numpy()
    assert (np.abs(ts[:3] - t[:3]) <= CR.t_star_bound(m, mb)[:3]).all() and np.abs(ts[:3] - 0.3).max() < 0.02
    # other grids, (B, H, W) inputs; nothing but NaN curves: no consensus
    fine = np.arange(0.2, 0.4, 0.01)
    per_f, cons_f, curves_f, _ = estimate_time_from_estimates(dev(g)[:, 0], dev(p1)[:, 0], dev(p2)[:, 0], t_list=fine)
    assert curves_f.shape == (4, 20) and abs(cons_f - 0.3) < 0.011
    per_n, cons_n, _, _ = estimate_time_from_estimates(dev(g)[3:], dev(p1)[3:], dev(p2)[3:])
    assert np.isnan(per_n).all() and np.isnan(cons_n)


def test_fused_scan_equals_the_torch_loop_on_the_fixture_networks():
    """estimate_time_using_PSNR(fused=True) on the refine_n1 fixture's networks and inputs equals
    estimate_time_from_estimates on the same channel estimates, whose curves lie within the derived bound of the
    restatement; its argmax is the restatement's wherever the float64 top-two gap is at least twice that bound (the
    number of samples left out is printed).  fused=False still reproduces the fixture."""
    from oracle import cases
    from diffsplitting_amd.core import psnr_based_t_refinement as R
    from tests.util import load_golden
    i1, i2, tp, _, _ = MU.networks(1)
    g = load_golden("refine_n1")
    inp = cases.make_cond("time_pred")
    B = inp.shape[0]
    torch.manual_seed(cases.LOOP_SEED)
    seq = {(name, b): [torch.randn(1, 1, 32, 32) for _ in range(2)] for b in range(B) for name in ("i1", "i2")}

    def source_for(name):
        it = iter([seq[(name, b)][k] for b in range(B) for k in range(2)])
        return lambda shape: next(it)

    def run(**kw):
        i1.noise_source, i2.noise_source = source_for("i1"), source_for("i2")
        return R.estimate_time_using_PSNR(inp, i1, i2, tp, num_timesteps=1, **kw)

    per_loop, cons_loop = run()
    assert np.allclose(per_loop, g["per_sample_t"]) and abs(cons_loop - float(g["concensus_t"])) < 1e-9   # untouched
    per_fused, cons_fused = run(fused=True)
    i1.noise_source, i2.noise_source = source_for("i1"), source_for("i2")
    pred1, pred2 = R.get_channel_estimates(inp, i1, i2, tp, num_timesteps=1, as_numpy=False)
    per_direct, cons_direct, curves, _ = R.estimate_time_from_estimates(inp.cuda().float(), pred1, pred2)
    assert np.array_equal(per_fused, per_direct) and cons_fused == cons_direct
    m, mb = CR.moments(inp[:, 0].numpy(), pred1[:, 0].cpu().numpy(), pred2[:, 0].cpu().numpy(), with_bounds=True)
    c, _ = CR.curve(m, T_LIST, 1 - T_LIST)
    bound = CR.curve_bound(m, mb, T_LIST, 1 - T_LIST)
    assert (np.abs(curves.cpu().numpy() - c) <= bound).all()
    top = np.sort(c, axis=1)
    clear = (top[:, -1] - top[:, -2]) >= 2 * bound.max(axis=1)
    print(f"fused scan: {int((~clear).sum())} of {B} samples left out (float64 top-two gap under twice the bound)")
    assert np.array_equal(per_fused[clear], T_LIST[c.argmax(axis=1)][clear])
    agree = int((np.asarray(per_loop) == per_fused).sum())
    print(f"fused scan against the fp32 loop: {agree} of {B} per-sample times equal, consensus {cons_fused} / {cons_loop}")


# ---- the driver -----------------------------------------------------------------------------------------------------
class OracleSampler:
    """Stands in for indi1 / indi2: `inference` answers with the true normalised channel of the tiles last cut."""

    def __init__(self, ds, channel):
        self.ds, self.channel, self.noise_source, self.starts = ds, channel, None, []

    def inference(self, x, continuous=False, num_timesteps=None, t_float_start=0.5, **kw):
        self.starts.append(t_float_start)
        self.last_full_batch = self.ds.tiles(self.ds.last_ids)["target"][:, self.channel:self.channel + 1].contiguous()
        assert self.last_full_batch.shape == x.shape


def _remember_ids(ds):
    cut = ds.mixed_tiles

    def mixed_tiles(ids, *a, **k):
        ds.last_ids = list(ids)
        return cut(ids, *a, **k)
    ds.mixed_tiles = mixed_tiles
    return ds


def _tile_curves(moments):
    """(tiles, 2, 12) -> curve_k (tiles, G) of the driver's definition, in float64 numpy, and its own rounding bound"""
    c0, _ = CR.curve(moments[:, 0], 1 - T_LIST, T_LIST)
    c1, _ = CR.curve(moments[:, 1], 1 - T_LIST, T_LIST)
    zero = np.zeros_like(moments[:, 0])
    own = 0.5 * (CR.curve_bound(moments[:, 0], zero, 1 - T_LIST, T_LIST) + CR.curve_bound(moments[:, 1], zero, 1 - T_LIST, T_LIST))
    return 0.5 * (c0 + c1), own


@pytest.mark.parametrize("scope", ["tile", "frame", "set"])
def test_oracle_samplers_recover_the_planted_time(scope):
    """2 x 96 x 96 frames, patch 32, grid 16 (50 tiles), mixing_t = 0.3, no TimePredictor: round 0 starts at 0.5 and one
    round later every unit has chosen t_list[6]."""
    from diffsplitting_amd.data.tiled_predict import predict_tiled_refined
    ds, _, _ = MU.dataset((2, 96, 96), 9)
    _remember_ids(ds)
    netG = types.SimpleNamespace(indi1=OracleSampler(ds, 0), indi2=OracleSampler(ds, 1), noise_source=None)
    (canvas, psnr), pred_t, rep = predict_tiled_refined(netG, None, ds, 0.3, rounds=1, scope=scope, batch_tiles=8,
                                                        keep_tiles=True)
    T = len(ds)
    assert T == 50 and canvas.shape == (2, 96, 96, 2) and psnr.shape == (2, 2) and len(rep["rounds"]) == 2
    r0, r1 = rep["rounds"]
    assert (r0["start"] == 0.5).all() and all(s == 0.5 for s in netG.indi1.starts[:7] + netG.indi2.starts[:7])
    units = {"tile": 50, "frame": 2, "set": 1}[scope]
    assert r0["chosen"].shape == (units,) and (r0["chosen"] == T_LIST[6]).all()
    assert (r1["start"] == np.float32(T_LIST[6])).all() and torch.equal(pred_t.cpu(), torch.from_numpy(r1["start"]))
    assert r0["curves"].shape == (T, 20) and (np.nanargmax(r0["curves"], axis=1) == 6).all()
    assert np.abs(r0["t_star"] - 0.3).max() < 1e-4 and np.abs(r1["t_star"] - 0.3).max() < 1e-4
    # the estimates ARE the target: the stitched canvas is the normalised ground truth
    assert torch.equal(canvas, ds.normalized_target_frames())
    # the reported moments of the last round against the restatement on the kept tensors
    tiles, mix = rep["tiles"].cpu().numpy(), rep["mix"].cpu().numpy()
    assert tiles.shape == (T, 2, 32, 32)
    for ch in (0, 1):
        ref, bnd = CR.moments(mix[:, ch], tiles[:, ch], tiles[:, 1 - ch], with_bounds=True)
        assert (np.abs(r1["moments"][:, ch] - ref) <= bnd).all(), ch
    curves, own = _tile_curves(r1["moments"])                           # the device's float64 ops against numpy's
    fin = np.isfinite(curves) & np.isfinite(r1["curves"]) & np.isfinite(own)
    assert fin.sum() >= 18 * T and (np.abs(curves - r1["curves"])[fin] <= own[fin]).all()


def _second_ids(ids):
    return [int(v) | (1 << 39) for v in ids]


def test_tiny_networks_rounds_and_the_argmax_rule():
    """rounds = 0: predict_tiled_mixed(t_from="classifier") bit for bit on the same draws.  rounds = 2 on frames whose
    second frame is constant (its tiles' curves are all NaN): every round's start times are the argmax rule applied to
    the previous round's reported moments, and the constant frame's tiles keep the classifier's times."""
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_tiled_mixed, predict_tiled_refined
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    i1, i2, tp, _, _ = MU.networks(1)
    netG = types.SimpleNamespace(indi1=i1, indi2=i2, noise_source=None, second_ids=_second_ids)
    ch0, ch1 = MU.frames((2, 64, 64), 5)
    ch0[1], ch1[1] = 300, 120                                          # a constant frame: 9 tiles without a curve
    ds = SplitDatasetTiledPred("Hagen", DataLocation(arrays=(ch0, ch1)), 32, grid_size=16, max_qval=0.98)
    T = len(ds)
    assert T == 18
    table = compute_input_normalization_dict(ds._data_dict, 100, ds._mean_target, ds._std_target)
    kw = dict(num_timesteps=1, mmse_count=2, batch_tiles=6, table=table, seed=5)
    (c_m, p_m), t_m = predict_tiled_mixed(netG, tp, ds, 0.29, **kw)
    (c_0, p_0), t_0, rep0 = predict_tiled_refined(netG, tp, ds, 0.29, rounds=0, **kw)
    assert same_bits(c_0, c_m) and same_bits(t_0, t_m)
    assert torch.equal(torch.isnan(p_0), torch.isnan(p_m)) and same_bits(torch.nan_to_num(p_0), torch.nan_to_num(p_m))
    assert len(rep0["rounds"]) == 1 and rep0["rounds"][0]["curves"].shape == (T, 20)
    frame = ds.plan.patch_start[:, 0]
    assert np.isnan(rep0["rounds"][0]["curves"][frame == 1]).all() and np.isfinite(rep0["rounds"][0]["curves"][frame == 0]).all()
    skipped = total = 0
    for scope in ("tile", "frame", "set"):
        (_, _), pred_t, rep = predict_tiled_refined(netG, tp, ds, 0.29, rounds=2, scope=scope, **kw)
        assert len(rep["rounds"]) == 3 and np.array_equal(rep["rounds"][0]["start"], t_m.cpu().numpy())
        assert np.array_equal(rep["rounds"][0]["moments"], rep0["rounds"][0]["moments"])      # round 0 does not depend on the scope
        for q in range(2):
            prev, nxt = rep["rounds"][q], rep["rounds"][q + 1]
            curves, own = _tile_curves(prev["moments"])
            for u in range(int(rep["units"].max()) + 1):
                rows = rep["units"] == u
                total += 1
                finite = ~np.isnan(curves[rows])
                with np.errstate(invalid="ignore"):                      # nanmean, by hand: 0 / 0 where no tile has a value
                    mean = np.where(finite, curves[rows], 0).sum(axis=0) / finite.sum(axis=0)
                mean[T_LIST <= 0] = np.nan                               # no sampler starts at 0
                if np.isnan(mean).all():                                 # no curve: the unit keeps its times
                    assert np.array_equal(nxt["start"][rows], prev["start"][rows]) and np.isnan(prev["chosen"][u])
                    continue
                top = np.sort(mean[~np.isnan(mean)])
                if top[-1] - top[-2] < 2 * np.nanmax(own[rows]):
                    skipped += 1
                    continue
                want = np.float32(T_LIST[int(np.nanargmax(mean))])
                assert (nxt["start"][rows] == want).all() and np.float32(prev["chosen"][u]) == want, (scope, q, u)
        # the constant frame kept the classifier's times through both rounds, whatever the scope does elsewhere
        if scope != "set":
            assert np.array_equal(rep["rounds"][2]["start"][frame == 1], t_m.cpu().numpy()[frame == 1])
        else:                                                          # one unit: the finite curves decide for every tile
            assert len(np.unique(rep["rounds"][2]["start"])) == 1
        assert torch.equal(pred_t.cpu(), torch.from_numpy(rep["rounds"][2]["start"]))
    print(f"argmax rule: {skipped} of {total} units left out (float64 top-two gap under twice the curve's own bound)")
    assert skipped < total


def test_driver_refusals():
    from diffsplitting_amd.data.tiled_predict import predict_tiled_refined
    for kw, word in ((dict(rounds=-1), "rounds"), (dict(scope="batch"), "scope"), (dict(t_list=[]), "t_list")):
        with pytest.raises(ValueError, match=word):
            predict_tiled_refined(None, None, None, 0.3, **kw)


def test_split_command_line_refined(tmp_path, caplog):
    """`split --mix-t 0.29 --t-from refined` on one frame of 64 x 64 (9 tiles), without a TimePredictor: what it returns
    is predict_tiled_refined's canvas on the same seeds, and rank 0 logs every round."""
    import logging
    from diffsplitting_amd import split
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.tiled_predict import predict_tiled_refined
    from diffsplitting_amd.model import create_model
    cfgs, _ = MU.write_configs(tmp_path)
    cfg, cfg_path = cfgs["joint"]
    caplog.set_level(logging.INFO, logger="base")
    args = ["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--datapath", "--norm-from", "val",
            "--steps", "1", "--batch-tiles", "3", "--mix-t", "0.29", "--t-from", "refined", "--refine-rounds", "2",
            "--refine-scope", "tile", "--refine-step", "0.1", "--sample-seed", "4"]
    torch.manual_seed(1234)
    pred = split.main(args)
    assert pred.shape == (1, 64, 64, 2) and torch.isfinite(pred).all()
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("refinement round")]
    assert len(lines) == 3 and all("scope tile, 9 of 9 units" in ln and "|chosen - mix_t|" in ln for ln in lines), lines
    assert sum("refined start times" in r.getMessage() for r in caplog.records) == 1
    torch.manual_seed(1234)
    opt = dict_to_nonedict(dict(cfg, phase="val"))
    diffusion = create_model(opt)
    diffusion.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    _, val_set = split.get_datasets(opt, tiled_pred=True, norm_from="val")
    (canvas, _), pred_t, rep = predict_tiled_refined(diffusion.netG, None, val_set, 0.29, num_timesteps=1, batch_tiles=3,
                                                     rounds=2, scope="tile", t_list=np.arange(0, 1.0, 0.1), seed=4)
    assert torch.equal(pred, canvas) and len(rep["rounds"]) == 3 and rep["rounds"][0]["curves"].shape == (9, 10)
    assert (rep["rounds"][0]["start"] == 0.5).all() and set(np.unique(pred_t.cpu().numpy())) <= set(np.float32(rep["t_list"]))


@pytest.mark.parametrize("world", [2, 3])
def test_refined_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks sharing the GPU (gloo transport): on every rank canvas, PSNR, pred_t and the whole report of
    predict_tiled_refined(seed=) equal the one-rank run done in the same process, bitwise
    (tests/multi_rank_predict_refined.py)."""
    r = run_ranks("multi_rank_predict_refined.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_REFINED_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
