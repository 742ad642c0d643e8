"""The TimePredictor family on the MI355X (`-m gpu`): the per-item mixed gather (dsx_tiles_gather_mix_items) bitwise
against the fp32 restatement of tests/mixed_ref.py and against dsx_tiles_gather_mix item by item,
``TimePredictorDataset.batch`` against the items, ``validation_loss`` against the same loop built from the oracle, the
two command lines, and ``predict_tiled_mixed`` sharded over two ranks against one."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

from oracle import cases
from oracle.unet import time_predictor_forward
from tests import mixed_ref as MR
from tests import mixed_util as MU
from tests import nets
from tests.bits import same_bits
from tests.rank_worker import run_ranks
from tests.util import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FP32_TOL = 1e-3                                                     # the project's fp32 parity bound (test_gpu_mixed.py)
T_SET = [0.0, 0.01, 0.29, 0.5, 0.99, 1.0]


# ---- 1. the per-item gather ---------------------------------------------------------------------------------------
class _Frames:
    """Case b of mix_range.npz on the device: 2 x 37 x 53, an odd width, so that rows are misaligned."""

    def __init__(self):
        g = load_golden("mix_range")
        self.ch0, self.ch1 = g["b_ch0"], g["b_ch1"]
        self.mean, self.std, self.table = g["b_mean_target"], g["b_std_target"], g["b_table_100"]
        self.dev = [torch.from_numpy(c.astype(np.float32)).cuda() for c in (self.ch0, self.ch1)]
        self.shape = self.ch0.shape
        self.norm = nets.dbl(self.mean[0], self.std[0], self.mean[1], self.std[1])

    def starts(self, ph, pw):
        N, H, W = self.shape
        fixed = [(0, 0, 0), (N - 1, H - ph, W - pw), (0, 3, 1), (1, 0, W - pw), (0, H - ph, 7), (1, 5, 5)]
        rng = np.random.default_rng(ph * 100 + pw)
        more = [(int(rng.integers(N)), int(rng.integers(H - ph + 1)), int(rng.integers(W - pw + 1)) | 1) for _ in range(5)]
        more = [(n, y, min(x, W - pw)) for n, y, x in more]
        out = fixed + more
        assert len(out) == 11 and any(x % 2 for _, _, x in out)
        return out

    def reference(self, loc, ph, pw, t):
        n, y, x = loc
        t0 = MR.normalize(self.ch0[n, y:y + ph, x:x + pw], self.mean[0], self.std[0])
        t1 = MR.normalize(self.ch1[n, y:y + ph, x:x + pw], self.mean[1], self.std[1])
        mix, cls = MR.chain_f32(t0, t1, t, MR.rows(self.table, t))
        return {"target": np.stack([t0, t1]), "mix": mix, "cls": cls}

    def items(self, starts, ts, ph, pw, want=("target", "mix", "cls")):
        """One call of dsx_tiles_gather_mix_items into buffers with one poisoned item on either side."""
        from diffsplitting_amd._lib import check, lib
        count = len(starts)
        out = {k: torch.full((count + 2, 2, ph, pw), float("nan"), dtype=torch.float32, device="cuda") for k in want}
        ptr = lambda k: C.c_void_p(out[k][1:].data_ptr()) if k in out else None
        lohi = [v for t in ts for v in MR.rows(self.table, t)]
        check(lib.dsx_tiles_gather_mix_items(
            C.c_void_p(self.dev[0].data_ptr()), C.c_void_p(self.dev[1].data_ptr()), nets.i64(*self.shape), nets.i64(1, ph, pw),
            nets.i64(*[v for s in starts for v in s]), count, self.norm, nets.dbl(*ts), nets.dbl(*lohi) if "cls" in out else None,
            ptr("target"), ptr("mix"), ptr("cls"), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        res = {}
        for k, v in out.items():
            v = v.cpu().numpy()
            assert np.isnan(v[0]).all() and np.isnan(v[-1]).all(), f"{k}: written outside the {count} items"
            res[k] = v[1:-1]
        return res

    def one_by_one(self, loc, t, ph, pw):
        """The existing dsx_tiles_gather_mix for this one location."""
        from diffsplitting_amd._lib import check, lib
        out = {k: torch.empty((1, 2, ph, pw), dtype=torch.float32, device="cuda") for k in ("target", "mix", "cls")}
        check(lib.dsx_tiles_gather_mix(
            C.c_void_p(self.dev[0].data_ptr()), C.c_void_p(self.dev[1].data_ptr()), nets.i64(*self.shape), nets.i64(1, ph, pw),
            nets.i64(*loc), None, 1, self.norm, float(t), nets.dbl(*MR.rows(self.table, t)), C.c_void_p(out["target"].data_ptr()),
            C.c_void_p(out["mix"].data_ptr()), C.c_void_p(out["cls"].data_ptr()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return {k: v[0].cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("ph,pw", [(20, 20), (7, 5)])
def test_per_item_gather_bitwise(ph, pw):
    f = _Frames()
    starts = f.starts(ph, pw)
    ts = [T_SET[(5 * k + 1) % len(T_SET)] for k in range(len(starts))]     # every t of the set, mixed within the call
    assert set(ts) == set(T_SET)
    got = f.items(starts, ts, ph, pw)
    for k, (loc, t) in enumerate(zip(starts, ts)):
        ref, single = f.reference(loc, ph, pw, t), f.one_by_one(loc, t, ph, pw)
        for name in ("target", "mix", "cls"):
            assert same_bits(got[name][k], ref[name]), (name, k, loc, t)
            assert same_bits(got[name][k], single[name]), (name, k, loc, t)
    # count = 1 (the last valid corner), count = 0 (nothing is written)
    one = f.items(starts[1:2], ts[1:2], ph, pw)
    assert all(same_bits(one[name][0], got[name][1]) for name in got)
    none = f.items([], [], ph, pw)
    assert all(v.shape == (0, 2, ph, pw) for v in none.values())
    # each output pointer NULL in turn, and each alone
    for drop in ("target", "mix", "cls"):
        want = tuple(n for n in ("target", "mix", "cls") if n != drop)
        part = f.items(starts, ts, ph, pw, want=want)
        assert sorted(part) == sorted(want) and all(same_bits(part[n], got[n]) for n in want), drop
        alone = f.items(starts, ts, ph, pw, want=(drop,))
        assert same_bits(alone[drop], got[drop]), drop


# ---- 2. / 3. the dataset's batches and the validation loop --------------------------------------------------------
def _dataset():
    from diffsplitting_amd.data.split_dataset import DataLocation
    from diffsplitting_amd.data.time_predictor_dataset import TimePredictorDataset
    g = load_golden("mix_range")
    nd = {"mean_target": g["ds_mean_target"], "std_target": g["ds_std_target"]}
    nd.update({k: g[f"ds_{k}"] for k in ("mean_input", "std_input", "target0_max", "target1_max", "input_max")})
    ds = TimePredictorDataset("Hagen", DataLocation(arrays=(g["c_ch0"], g["c_ch1"])), 32, max_qval=0.98,
                              normalization_dict=nd, step_size=0.25)
    assert len(ds) == 8
    return ds, g, nd


def test_batch_equals_the_items():
    from diffsplitting_amd._lib import DsxError
    ds, _, _ = _dataset()
    for seed in (11, 12):
        np.random.seed(seed)
        inp, t = ds.batch(range(8))
        after_batch = np.random.randint(1 << 30)
        np.random.seed(seed)
        items = [ds[i] for i in range(8)]
        after_items = np.random.randint(1 << 30)
        assert inp.is_cuda and inp.shape == (8, 1, 32, 32) and inp.dtype == torch.float32 and inp.is_contiguous()
        assert isinstance(t, np.ndarray) and t.shape == (8,) and t.dtype == np.float64
        assert np.array_equal(t, np.array([it[1] for it in items]))
        assert same_bits(inp.cpu().numpy(), np.stack([it[0] for it in items]))
        assert after_batch == after_items
        assert len(set(t.tolist())) > 1                                  # the items do carry different t
    # given t_ints: the same items, no random number consumed
    np.random.seed(5)
    state = np.random.get_state()
    t_ints = [int(round(v * 100)) for v in t]
    again, t2 = ds.batch(range(8), t_ints=t_ints)
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    assert torch.equal(again, inp) and np.array_equal(t2, t)
    sub, t3 = ds.batch([6, 1], t_ints=np.array([0, 99]))
    assert np.array_equal(t3, [0.0, 0.99]) and sub.shape == (2, 1, 32, 32)
    empty, t0 = ds.batch([])
    assert empty.shape == (0, 1, 32, 32) and t0.shape == (0,)
    for bad in ([100], [-1], [0.5], [True], ["3"]):
        with pytest.raises(DsxError, match="t_ints"):
            ds.batch([0], t_ints=bad)
    with pytest.raises(DsxError, match="t_ints"):
        ds.batch([0, 1], t_ints=[3])


_REF = {}


def _oracle_loop(seed):
    """The reference's loop from the oracle: the seeded draws, the items from MR.chain_f32, the predictions from
    time_predictor_forward.  Computed once per seed, shared, never modified."""
    if seed not in _REF:
        ds, g, nd = _dataset()
        _, sd = MU.time_predictor()
        np.random.seed(seed)
        t_ints = [np.random.randint(0, 100) for _ in range(len(ds))]
        t = np.array([v / 100 for v in t_ints], dtype=np.float64)
        items = []
        for i, (tv, ti) in enumerate(zip(t, t_ints)):
            n, y, x = ds.patch_location(i)
            t0 = MR.normalize(g["c_ch0"][n, y:y + 32, x:x + 32], nd["mean_target"][0], nd["std_target"][0])
            t1 = MR.normalize(g["c_ch1"][n, y:y + 32, x:x + 32], nd["mean_target"][1], nd["std_target"][1])
            row = g["c_table_100"][ti]
            items.append(MR.chain_f32(t0, t1, float(tv), (row[0], row[1]) * 2)[1][1])
        pred = time_predictor_forward(sd, cases.TIME_PRED_CFG, torch.from_numpy(np.stack(items)[:, None])).numpy()
        pred = pred.reshape(-1).astype(np.float64)
        pred.setflags(write=False)
        t.setflags(write=False)
        _REF[seed] = (pred, t)
    return _REF[seed]


def _loop_means(pred, t, batch, loss_type):
    d = pred - t.astype(np.float32).astype(np.float64)
    d = np.abs(d) if loss_type == "l1" else d * d
    return float(np.mean([d[i:i + batch].mean() for i in range(0, len(d), batch)]))


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_validation_loss_against_the_oracle(loss_type):
    """8 items in batches of 3, 3 and 2 (the short last batch overlaps the one before it), then 8 and 1."""
    from diffsplitting_amd.time_prediction import validation_loss
    ds, _, _ = _dataset()
    tp, _ = MU.time_predictor()
    seed = 21
    ref_pred, ref_t = _oracle_loop(seed)
    y = ref_t.astype(np.float32).astype(np.float64)
    loss_bound = FP32_TOL if loss_type == "l1" else 2 * np.abs(ref_pred - y).max() * FP32_TOL + 1e-6
    first = None
    for batch in (3, 3, 8, 1):
        np.random.seed(seed)
        val_loss, per_batch, pred, t = validation_loss(tp, ds, batch, loss_type)
        assert pred.shape == (8,) and pred.dtype == np.float32 and t.dtype == np.float64 and np.array_equal(t, ref_t)
        assert len(per_batch) == -(-8 // batch) and val_loss == float(np.mean(per_batch))
        err = np.abs(pred - ref_pred).max()
        ref_loss = _loop_means(ref_pred, ref_t, batch, loss_type)
        print(f"{loss_type} batch {batch}: max |pred - oracle| {err:.3e}, val_loss {val_loss:.6e}, oracle {ref_loss:.6e}, "
              f"|diff| {abs(val_loss - ref_loss):.3e} (bound {loss_bound:.3e})")
        assert err <= FP32_TOL
        assert abs(val_loss - ref_loss) <= loss_bound
        if batch == 3:
            if first is None:
                first = (val_loss, per_batch, pred, t)
            else:                                                        # the same seed again: bitwise the same
                assert val_loss == first[0] and same_bits(per_batch, first[1]) and same_bits(pred, first[2]) and same_bits(t, first[3])


# ---- 4. the command lines -----------------------------------------------------------------------------------------
def _logged(caplog, prefix):
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith(prefix)]
    assert len(lines) == 1, (prefix, lines)
    return lines[0]


def test_time_prediction_command_line(tmp_path, caplog):
    from diffsplitting_amd import time_prediction as TP
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.tiled_predict import evaluate_time_predictor
    cfgs, pth = MU.write_configs(tmp_path)
    cfg, cfg_path = cfgs["tp"]
    caplog.set_level(logging.INFO, logger="base")
    res = TP.main(["-c", cfg_path, "--datapath", "--norm-from", "val", "--checkpoint", pth, "--seed", "3", "--sweep", "4"])
    # the same by hand
    opt = dict_to_nonedict(cfg)
    model = TP.build_time_predictor(opt, pth)
    train_set, val_set = TP.get_datasets(opt, norm_from="val")
    assert train_set is None and len(val_set) == 4
    np.random.seed(3)
    val_loss, per_batch, pred, t = TP.validation_loss(model, val_set, 3, "l2")
    assert len(per_batch) == 2 and res["val_loss"] == val_loss and same_bits(res["pred"], pred) and same_bits(res["t"], t)
    assert _logged(caplog, "val_loss: ") == "val_loss: {:.4e}".format(val_loss)
    tiled = TP.tiled_val_set(opt, val_set)
    assert len(tiled) == 9
    all_pred, rmse = evaluate_time_predictor(tiled, model, num_timesteps=4, batch_tiles=3)
    assert res["rmse"] == rmse and same_bits(res["all_pred"], all_pred) and all_pred.shape == (5, 9)
    assert _logged(caplog, "sweep RMSE: ") == "sweep RMSE: {:.4e}".format(rmse)
    assert sum(r.getMessage().startswith("ratio ") for r in caplog.records) == 5
    # with the training stack's statistics (here the same files): the same value; without a checkpoint: said so
    caplog.clear()
    res2 = TP.main(["-c", cfg_path, "--datapath", "--seed", "3", "--batch-size", "8"])
    assert "rmse" not in res2 and len(res2["per_batch"]) == 1 and np.isfinite(res2["val_loss"])
    assert any("random initial weights" in r.getMessage() for r in caplog.records)


def test_split_command_line_mixed_prediction(tmp_path, caplog):
    """The case of test_predict_tiled_mixed_against_the_oracle reduced to one frame of 64 x 64 (9 tiles), through the
    command line: the written file is the canvas predict_tiled_mixed returns, un-normalised."""
    from diffsplitting_amd import split
    from diffsplitting_amd import time_prediction as TP
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.tiled_predict import predict_tiled_mixed
    from diffsplitting_amd.model import create_model
    cfgs, pth = MU.write_configs(tmp_path)
    (cfg, cfg_path), (tp_cfg, tp_path) = cfgs["joint"], cfgs["tp"]
    out = str(tmp_path / "pred.npy")
    caplog.set_level(logging.INFO, logger="base")
    torch.manual_seed(1234)
    pred = split.main(["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--datapath", "--norm-from", "val",
                       "--steps", "1", "--batch-tiles", "8", "--mix-t", "0.29", "--time-predictor", tp_path,
                       "--time-predictor-checkpoint", pth, "--out", out])
    assert pred.shape == (1, 64, 64, 2) and torch.isfinite(pred).all()
    line = _logged(caplog, "mixed-input prediction at t = 0.29")
    assert "9 tiles of 32^2" in line and "classifier" in line
    assert sum("predicted start time min" in r.getMessage() for r in caplog.records) == 2
    # the same by hand, in the same order (initial weights and noise seeds come from torch's generator)
    torch.manual_seed(1234)
    opt = dict_to_nonedict(dict(cfg, phase="val"))
    diffusion = create_model(opt)
    diffusion.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    _, val_set = split.get_datasets(opt, tiled_pred=True, norm_from="val")
    tp = TP.build_time_predictor(dict_to_nonedict(tp_cfg), pth)
    (canvas, psnr), pred_t = predict_tiled_mixed(diffusion.netG, tp, val_set, 0.29, num_timesteps=1, mmse_count=1, batch_tiles=8)
    assert pred_t.shape == (9, 2) and torch.isfinite(pred_t).all()
    assert torch.equal(pred, canvas)
    nd = val_set.get_normalization_dict()
    mean = torch.as_tensor(np.asarray(nd["mean_target"]).reshape(-1), dtype=torch.float32, device=canvas.device)
    std = torch.as_tensor(np.asarray(nd["std_target"]).reshape(-1), dtype=torch.float32, device=canvas.device)
    saved = np.load(out)
    assert saved.dtype == np.float32 and np.array_equal(saved, (canvas * std + mean).cpu().numpy())
    # --t-from given needs no classifier
    given = split.main(["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--datapath", "--norm-from", "val",
                        "--steps", "1", "--mix-t", "0.29", "--t-from", "given"])
    assert given.shape == (1, 64, 64, 2) and torch.isfinite(given).all()


# ---- 5. the sharded mixed prediction ------------------------------------------------------------------------------
def test_two_ranks_mixed_prediction_equals_one_rank():
    """Two fresh ranks (parallel.self_launch) on the one GPU, gloo transport, as
    test_ranks_share_the_one_gpu_gloo_transport: canvas, PSNR and the gathered pred_t of the sharded run equal the
    one-rank run inside the same helper, bit for bit, on every rank."""
    import subprocess
    import sys
    r = run_ranks("multi_rank_predict_mixed.py", 2, backend="gloo", launch_timeout=500, timeout=600)
    assert r.returncode == 0 and "PREDICT_MIXED_OK 18 2" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
