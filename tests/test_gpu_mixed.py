"""Mixed-input evaluation on the MI355X (`-m gpu`): the range table (dsx_mix_range) bitwise against the fixture the
reference's own code produced, the fused mixed tiles (dsx_tiles_gather_mix / dsx_tileplan_gather_mix) bitwise against
the fp32 restatement of tests/mixed_ref.py and within its derived bound of the float64 evaluation, TimePredictorDataset
items against the reference's, and the two drivers against the same pipelines built from the oracle.

Measured on the MI355X (figures printed by the tests, `-s`): see the docstrings below."""
import types

import numpy as np
import pytest
import torch

from oracle import cases, samplers, tiling
from oracle.unet import time_predictor_forward
from tests import mixed_ref as MR
from tests import mixed_util as MU
from tests.bits import same_bits
from tests.gpu_util import maxabs
from tests.util import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FP32_TOL = 1e-3
T_VALUES = [0.0, 0.1, 0.29, 0.5, 1.0]


def _table_array(tab):
    n = len(tab) - 1
    assert sorted(tab) == list(range(n + 1))
    for v in tab.values():
        assert isinstance(v, list) and len(v) == 2 and isinstance(v[0], np.float64) and isinstance(v[1], np.float64)
    return np.array([tab[t] for t in range(n + 1)], dtype=np.float64)


def _norm_dict(mean, std):
    return {"mean_input": np.float64(mean.sum()), "std_input": np.float64(std.sum()), "mean_target": np.asarray(mean),
            "std_target": np.asarray(std)}


def _tiled(g, name, patch=32, grid=16):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    ch0, ch1 = g[f"{name}_ch0"], g[f"{name}_ch1"]
    return SplitDatasetTiledPred("Hagen", DataLocation(arrays=(ch0, ch1)), patch, grid_size=grid,
                                 normalization_dict=_norm_dict(g[f"{name}_mean_target"], g[f"{name}_std_target"])), ch0, ch1


def _ref_tiles(ds, ch0, ch1, ids):
    """normalised float32 target channels of the tiles `ids`, (b, p, p) each, restated"""
    p = ds._patch_size
    mean, std = ds._mean_target.reshape(-1), ds._std_target.reshape(-1)
    t0, t1 = [], []
    for i in ids:
        n, y, x = ds.patch_location(int(i))
        t0.append(MR.normalize(ch0[n, y:y + p, x:x + p], mean[0], std[0]))
        t1.append(MR.normalize(ch1[n, y:y + p, x:x + p], mean[1], std[1]))
    return np.stack(t0), np.stack(t1)


def test_range_table_bitwise_equal_to_the_reference_and_repeatable():
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    g = load_golden("mix_range")
    for name in [str(c) for c in g["cases"]]:
        ch0, ch1 = g[f"{name}_ch0"], g[f"{name}_ch1"]
        mean, std = g[f"{name}_mean_target"], g[f"{name}_std_target"]
        dev = {0: torch.from_numpy(ch0.astype(np.float32)).cuda(), 1: torch.from_numpy(ch1.astype(np.float32)).cuda()}
        for n in [int(v) for v in g["timesteps"]]:
            a = _table_array(compute_input_normalization_dict(dev, n, mean, std))
            b = _table_array(compute_input_normalization_dict(dev, n, mean.reshape(-1, 1, 1), std.reshape(-1, 1, 1)))
            ref = g[f"{name}_table_{n}"]
            assert same_bits(a, ref), (name, n, np.abs(a - ref).max())
            assert same_bits(a, b), (name, n)
        # host frames (a list of uint16 arrays, as the reference holds them) are uploaded
        c = _table_array(compute_input_normalization_dict({0: [x for x in ch0], 1: [x for x in ch1]}, 20, mean, std))
        assert same_bits(c, g[f"{name}_table_20"])


@pytest.mark.parametrize("name", ["c", "a"])
def test_mixed_tiles_bitwise_equal_to_the_fp32_restatement(name):
    """Observed on the MI355X: mix and cls bitwise equal for every t and both forms; against float64 the largest
    error / bound ratio was 0.785 (case a, t = 0.29; 0.738 for case c): the derived bound holds and is not slack."""
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    g = load_golden("mix_range")
    ds, ch0, ch1 = _tiled(g, name)
    table = compute_input_normalization_dict(ds._data_dict, 100, ds._mean_target, ds._std_target)
    assert same_bits(_table_array(table), g[f"{name}_table_100"])
    seq = list(range(1, len(ds), 3))                                    # a shard: through the plan's device tables
    irregular = [len(ds) - 1, 0, 7, 7, 3]                               # through the per-call host table
    worst = 0.0
    for ids in (seq, irregular):
        t0, t1 = _ref_tiles(ds, ch0, ch1, ids)
        plain = ds.tiles(ids)["target"]
        for t in T_VALUES:
            out = ds.mixed_tiles(ids, t, table)
            assert sorted(out) == ["cls", "mix", "target"] and out["mix"].shape == (len(ids), 2, 32, 32)
            assert torch.equal(out["target"], plain)
            lohi = MR.rows(g[f"{name}_table_100"], t)
            mix, cls = MR.chain_f32(t0, t1, t, lohi)
            got_mix, got_cls = out["mix"].cpu().numpy(), out["cls"].cpu().numpy()
            assert same_bits(got_mix, np.moveaxis(mix, 0, 1)), (name, t)
            assert same_bits(got_cls, np.moveaxis(cls, 0, 1)), (name, t)
            m64, c64 = MR.chain_f64(t0, t1, t, lohi)
            bm, bc = MR.chain_bound(t0, t1, t, lohi)
            em = np.abs(np.moveaxis(got_mix, 1, 0) - m64)
            ec = np.abs(np.moveaxis(got_cls, 1, 0) - c64)
            ratio = max(float((em / np.maximum(bm, 1e-300)).max()), float((ec / bc).max()))
            worst = max(worst, ratio)
            print(f"case {name} t={t}: max mix err {em.max():.3e}, max cls err {ec.max():.3e}, max err/bound {ratio:.3f}")
            assert (em <= bm).all() and (ec <= bc).all(), (name, t)
            only = ds.mixed_tiles(ids, t, want=("mix",))                # any subset of the outputs
            assert sorted(only) == ["mix"] and torch.equal(only["mix"], out["mix"])
    print(f"case {name}: worst err/bound {worst:.3f}")
    # the base class (grid patches, host-table form) computes the same chain
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    if ch0.shape[1] == ch0.shape[2]:
        base = SplitDataset("Hagen", DataLocation(arrays=(ch0, ch1)), 32,
                            normalization_dict=_norm_dict(g[f"{name}_mean_target"], g[f"{name}_std_target"]))
        ids = [0, 5, 2]
        t0, t1 = _ref_tiles(base, ch0, ch1, ids)
        out = base.mixed_tiles(ids, 0.29, table)
        mix, cls = MR.chain_f32(t0, t1, 0.29, MR.rows(g[f"{name}_table_100"], 0.29))
        assert same_bits(out["cls"].cpu().numpy(), np.moveaxis(cls, 0, 1))


def test_time_predictor_dataset_items_equal_the_reference():
    from diffsplitting_amd.data.split_dataset import DataLocation
    from diffsplitting_amd.data.time_predictor_dataset import TimePredictorDataset
    g = load_golden("mix_range")
    nd = _norm_dict(g["ds_mean_target"], g["ds_std_target"])
    nd.update({k: g[f"ds_{k}"] for k in ("mean_input", "std_input", "target0_max", "target1_max", "input_max")})
    ds = TimePredictorDataset("Hagen", DataLocation(arrays=(g["c_ch0"], g["c_ch1"])), 32, max_qval=0.98,
                              normalization_dict=nd, step_size=0.25)
    assert same_bits(_table_array(ds.input_normalization_dict), g["c_table_100"])
    assert len(ds) == 8
    np.random.seed(int(g["item_seed"]))
    for k, idx in enumerate(g["item_indices"]):
        inp, t = ds[int(idx)]
        ref = g["item_inp"][k]
        assert t == float(g["item_t"][k]) and inp.shape == (1, 32, 32) and inp.dtype == np.float32
        if ref.dtype == np.float32:
            assert same_bits(inp, ref)
        else:                                                       # fixture made under numpy 2: see mixed_ref
            n, y, x = ds.patch_location(int(idx))
            t0 = MR.normalize(g["c_ch0"][n, y:y + 32, x:x + 32], nd["mean_target"][0], nd["std_target"][0])
            t1 = MR.normalize(g["c_ch1"][n, y:y + 32, x:x + 32], nd["mean_target"][1], nd["std_target"][1])
            row = g["c_table_100"][int(round(t * 100))]
            lohi = (row[0], row[1]) * 2
            _, cls = MR.chain_f32(t0, t1, t, lohi)
            assert same_bits(inp[0], cls[1])     # the float32 chain, bitwise
            _, bound = MR.chain_bound(t0, t1, t, lohi)
            err = np.abs(inp[0].astype(np.float64) - ref[0])
            print(f"item {idx}: max err {err.max():.3e} (bound there {bound[1].reshape(-1)[err.argmax()]:.3e})")
            assert (err <= bound[1]).all()
    img = np.linspace(-1, 1, 5)
    lo, hi = ds.input_normalization_dict[3]
    assert np.array_equal(ds.min_max_normalize(img, 3), 2 * (img - lo) / (hi - lo) - 1)


# ---- the drivers against the oracle ---------------------------------------------------------------------------------
def test_evaluate_time_predictor_against_the_oracle():
    """18 tiles of 32 x 32 in batches of 8 (the last one padded by overlap), 21 mixing ratios."""
    from diffsplitting_amd.data.tiled_predict import evaluate_time_predictor
    _, _, tp, sds, _ = MU.networks(1)
    ds, ch0, ch1 = MU.dataset((2, 64, 64), 5)
    n = 20
    all_pred, rmse = evaluate_time_predictor(ds, tp, num_timesteps=n, batch_tiles=8)
    assert all_pred.shape == (n + 1, len(ds)) and all_pred.dtype == np.float32 and len(ds) == 18
    table = MR.range_table(ch0, ch1, n, ds._mean_target.reshape(-1), ds._std_target.reshape(-1))
    t0, t1 = _ref_tiles(ds, ch0, ch1, range(len(ds)))
    gt = np.arange(0, 1.01, 1 / n)
    worst = 0.0
    for k, t in enumerate(gt):
        _, cls = MR.chain_f32(t0, t1, float(t), MR.rows(table, float(t)))
        ref = time_predictor_forward(sds["keys_tp"], cases.TIME_PRED_CFG, torch.from_numpy(cls[1][:, None])).numpy()
        worst = max(worst, maxabs(all_pred[k], ref))
        assert maxabs(all_pred[k], ref) <= FP32_TOL, (k, maxabs(all_pred[k], ref))
    print(f"evaluate_time_predictor: max |engine - oracle| over the sweep {worst:.3e}, rmse {rmse:.6f}")
    mse = ((all_pred - gt.reshape(-1, 1)) ** 2).mean(axis=1)
    assert rmse == float(np.sqrt(mse.mean()))


def test_predict_tiled_mixed_against_the_oracle():
    """2 x 96 x 96 frames, patch 32, grid 16 (50 tiles), one step, the reference's per-tile draw order."""
    from diffsplitting_amd.core.psnr import RangeInvariantPsnr
    from diffsplitting_amd.data.tiled_predict import predict_tiled_mixed
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    i1, i2, tp, sds, cfg = MU.networks(1)
    ds, ch0, ch1 = MU.dataset((2, 96, 96), 9)
    netG = types.SimpleNamespace(indi1=i1, indi2=i2, noise_source=None)
    mixing_t, T = 0.29, len(ds)
    assert T == 50
    torch.manual_seed(cases.LOOP_SEED)
    seq = {(name, b): [torch.randn(1, 1, 32, 32) for _ in range(2)] for b in range(T) for name in ("i1", "i2")}

    def source_for(name):
        it = iter([seq[(name, b)][k] for b in range(T) for k in range(2)])
        return lambda shape: next(it)

    table = compute_input_normalization_dict(ds._data_dict, 100, ds._mean_target, ds._std_target)

    def run():
        i1.noise_source, i2.noise_source = source_for("i1"), source_for("i2")
        return predict_tiled_mixed(netG, tp, ds, mixing_t, num_timesteps=1, mmse_count=1, batch_tiles=8, table=table)

    (canvas, psnr), pred_t = run()
    assert canvas.shape == (2, 96, 96, 2) and psnr.shape == (2, 2) and pred_t.shape == (T, 2)
    # the same pipeline from the oracle, tile by tile in the notebook's order (cells 59-64)
    tab = MR.range_table(ch0, ch1, 100, ds._mean_target.reshape(-1), ds._std_target.reshape(-1))
    assert same_bits(_table_array(table), tab)
    t0, t1 = _ref_tiles(ds, ch0, ch1, range(T))
    mix, cls = MR.chain_f32(t0, t1, mixing_t, MR.rows(tab, mixing_t))
    osd1, osd2 = sds["keys1"], sds["keys2"]                            # the samplers' keys: "denoise_fn." + the UNet's
    preds, ref_t = [], []
    for b in range(T):
        c0, c1 = torch.from_numpy(cls[0][b][None, None]), torch.from_numpy(cls[1][b][None, None])
        p0 = 1 - float(time_predictor_forward(sds["keys_tp"], cases.TIME_PRED_CFG, c0))
        p1 = float(time_predictor_forward(sds["keys_tp"], cases.TIME_PRED_CFG, c1))
        ref_t.append((p0, p1))
        d1, d2 = iter(seq[("i1", b)]), iter(seq[("i2", b)])
        o1 = samplers.indi_inference(osd1, cfg, torch.from_numpy(mix[0][b][None, None]), 1, 1, randn=lambda s: next(d1), t_float_start=p0)
        o2 = samplers.indi_inference(osd2, cfg, torch.from_numpy(mix[1][b][None, None]), 1, 1, randn=lambda s: next(d2), t_float_start=p1)
        preds.append(torch.cat([o1, o2], dim=1)[0].numpy())
    ref_canvas = tiling.stitch(np.stack(preds), tiling.TilePlan((2, 96, 96), (1, 16, 16), (1, 32, 32)))
    et, ec = maxabs(pred_t.cpu().numpy(), np.array(ref_t)), maxabs(canvas.cpu().numpy(), ref_canvas)
    ref_psnr = torch.stack([RangeInvariantPsnr(ds.normalized_target_frames()[..., c], canvas[..., c]) for c in range(2)], dim=1)
    ep = maxabs(psnr.cpu().numpy(), ref_psnr.cpu().numpy())
    print(f"predict_tiled_mixed: pred_t in [{np.min(ref_t):.3f}, {np.max(ref_t):.3f}], max |pred_t - oracle| {et:.3e}, "
          f"max |canvas - oracle| {ec:.3e}, max |fused PSNR - RangeInvariantPsnr| {ep:.3e} dB, PSNR {psnr.cpu().numpy().round(2).tolist()}")
    assert et <= FP32_TOL and ec <= FP32_TOL and ep <= 1e-3
    # same draws -> bitwise the same
    (canvas2, psnr2), pred_t2 = run()
    assert torch.equal(canvas, canvas2) and torch.equal(psnr, psnr2) and torch.equal(pred_t, pred_t2)
    # t_from="given": both samplers started at mixing_t, as running indi1 / indi2 directly on the mixed tiles
    i1.noise_source = i2.noise_source = None
    torch.manual_seed(3)
    (given, _), gt_t = predict_tiled_mixed(netG, None, ds, mixing_t, num_timesteps=1, batch_tiles=8, t_from="given")
    assert torch.equal(gt_t, torch.full((T, 2), float(mixing_t), device=gt_t.device))
    torch.manual_seed(3)
    direct = []
    for i in range(0, T, 8):
        m = ds.mixed_tiles(range(i, min(i + 8, T)), mixing_t, want=("mix",))["mix"]
        i1.inference(m[:, 0:1].contiguous(), num_timesteps=1, t_float_start=mixing_t)
        a = i1.last_full_batch.clone()
        i2.inference(m[:, 1:2].contiguous(), num_timesteps=1, t_float_start=mixing_t)
        direct.append(torch.cat([a, i2.last_full_batch], dim=1))
    assert torch.equal(given, ds.plan.stitch(torch.cat(direct)))
    # MMSE over repeats averages
    (m3, _), _ = predict_tiled_mixed(netG, tp, ds, mixing_t, num_timesteps=1, mmse_count=3, batch_tiles=8, table=table)
    assert torch.isfinite(m3).all() and maxabs(m3.cpu().numpy(), canvas.cpu().numpy()) < 0.2
