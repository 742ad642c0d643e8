"""The validation report on the MI355X (`-m gpu`): dsx_val_report bit-exact against the fixtures the reference's own
validation block wrote (tools/gen_validation_golden.py) on both access paths, against int64 numpy on planes of several
workgroups, the undefined-pixel counter, and validate / split --validate end to end."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import nets
from tests.util import load_golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ND_KEYS = ("mean_input", "std_input", "mean_target", "std_target")


def _case(name, prefix):
    g = load_golden(name)
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)} if prefix else g


def _np(t):
    return t.cpu().numpy()


def _offset4(a):
    """The array on the device as a contiguous tensor that starts 4 bytes past a 16-byte boundary."""
    t = torch.cat([torch.zeros(1), torch.from_numpy(a).reshape(-1)]).cuda()[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _numpy_report(inp, tar, pred, nd):
    """The block's arithmetic in numpy (float64, truncating casts; NaN and out-of-range values as 0, counted), with
    the statistics and numerators in int64."""
    def cast(v, clamp):
        bad = np.isnan(v) if clamp else ~((v >= 0) & (v < 65536))
        v = np.where(bad, 0.0, v)
        if clamp:
            v = np.clip(v, 0, 65535)
        return v.astype(np.int64), int(bad.sum())
    mt, st = (np.asarray(nd[k], dtype=np.float64).reshape(1, -1, 1, 1) for k in ("mean_target", "std_target"))
    tq, u0 = cast(tar.astype(np.float64) * st + mt, False)
    pq, u1 = cast(pred.astype(np.float64) * st + mt, True)
    iq, u2 = cast((inp.astype(np.float64) * np.float64(nd["std_input"]) + np.float64(nd["mean_input"])) / 2, False)
    f = lambda a: a.reshape(a.shape[0], a.shape[1], -1)
    out = {"target_q": tq, "pred_q": pq, "input_q": iq, "undefined": u0 + u1 + u2,
           "ssd": ((f(tq) - f(pq)) ** 2).sum(axis=2), "tmin": f(tq).min(axis=2), "tmax": f(tq).max(axis=2),
           "imin": f(iq).min(axis=2), "imax": f(iq).max(axis=2)}
    tmin = out["tmin"][:, :, None, None]
    out["target_n"] = tq - tmin
    out["pred_n"] = np.minimum((pq - tmin) % 65536, (out["tmax"] - out["tmin"])[:, :, None, None])
    out["input_n"] = iq - out["imin"].min(axis=1)[:, None, None, None]
    return out


def _assert_equal(res, want, visuals):
    for k in ("input_q", "target_q", "pred_q"):
        got = _np(getattr(res, k))
        assert got.dtype == np.uint16 and np.array_equal(got.astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    for k in ("ssd", "tmin", "tmax", "imin", "imax"):
        assert getattr(res, k).dtype == np.int64 and np.array_equal(getattr(res, k), want[k]), k
    assert res.undefined == int(want["undefined"])
    if visuals:
        for k in ("input_n", "target_n", "pred_n"):
            got = _np(getattr(res, k))
            assert got.dtype == np.uint16 and np.array_equal(got.astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    else:
        assert res.target_n is None and res.target_img is None


# ----------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("name,prefix,offset", [
    ("validation_L", "p5x7_", False),        # H*W = 35: scalar path
    ("validation_L", "p64x64_", False),      # 16-byte path
    ("validation_L", "p64x64_", True),       # H*W a multiple of 4, bases 4 bytes past a 16-byte boundary: scalar path
    ("validation_RGB", "", False),           # three input channels: 'RGB' mode, groups of three, no images
])
def test_report_bit_equal_to_the_reference_fixture(name, prefix, offset):
    from diffsplitting_amd.core.validation import group_psnr, validation_report
    g = _case(name, prefix)
    up = _offset4 if offset else (lambda a: torch.from_numpy(a).cuda())
    res = validation_report(up(g["input"]), up(g["target"]), up(g["prediction"]), {k: g[k] for k in ND_KEYS})
    rgb = g["input"].shape[1] == 3
    assert res.mode == ("RGB" if rgb else "L") and res.undefined == 0
    _assert_equal(res, g, visuals=not rgb)
    grouped = group_psnr(res)
    assert sorted(grouped) == list(g["psnr_keys"])
    ours = np.array([grouped[k] for k in sorted(grouped)]).T
    assert np.abs(ours - g["psnr"]).max() <= 1e-3              # the reference's float32 PSNR; a bound, see the CPU test
    if not rgb:
        for k in ("input_img", "target_img", "pred_img"):
            assert getattr(res, k).dtype == np.float64 and np.array_equal(getattr(res, k), g[k]), k
        plain = validation_report(up(g["input"]), up(g["target"]), up(g["prediction"]), {k: g[k] for k in ND_KEYS},
                                  visuals=False)
        _assert_equal(plain, g, visuals=False)                # the statistics do not depend on the second launch's grid


# ----------------------------------------------------------------------------- several workgroups per plane
@pytest.mark.parametrize("H,W", [
    (96, 100),       # 9600 pixels: three workgroups of 4096 per plane with a ragged tail of 1408, 16-byte path
    (97, 99),        # 9603 pixels: the same on the scalar path, the last group of four incomplete
])
def test_planes_of_three_workgroups_against_int64_numpy(H, W):
    from diffsplitting_amd.core.validation import VAL_CHUNK, validation_report
    assert 2 * VAL_CHUNK < H * W < 3 * VAL_CHUNK and (H * W) % VAL_CHUNK != 0
    rng = np.random.default_rng(H * 1000 + W)
    nd = {"mean_input": np.float64(1246.59), "std_input": np.float64(1246.59),
          "mean_target": np.array([759.685, 486.905]).reshape(-1, 1, 1), "std_target": np.array([759.685, 486.905]).reshape(-1, 1, 1)}
    raw = rng.integers(40, 60000, size=(2, 2, H, W)).astype(np.float64)
    tar = ((raw - nd["mean_target"]) / nd["std_target"]).astype(np.float32)
    inp = ((raw.sum(axis=1, keepdims=True) - nd["mean_input"]) / nd["std_input"]).astype(np.float32)
    pred = (tar + rng.normal(0, 3.0, size=tar.shape)).astype(np.float32)
    # the extremes sit in different workgroups' chunks: first, middle, tail
    raw_min = np.array([7.0, 11.0]).reshape(1, 2, 1)
    tar.reshape(2, 2, -1)[:, :, 2 * VAL_CHUNK + 1400] = ((raw_min - nd["mean_target"].reshape(1, 2, 1)) / nd["std_target"].reshape(1, 2, 1))[..., 0]
    tar.reshape(2, 2, -1)[:, :, VAL_CHUNK + 5] = ((65500.0 - nd["mean_target"].reshape(2)) / nd["std_target"].reshape(2))
    want = _numpy_report(inp, tar, pred, nd)
    assert want["undefined"] == 0 and (want["pred_q"] == 0).any() and (want["pred_q"] < want["tmin"][:, :, None, None]).any()
    res = validation_report(torch.from_numpy(inp).cuda(), torch.from_numpy(tar).cuda(), torch.from_numpy(pred).cuda(), nd)
    _assert_equal(res, want, visuals=True)
    ssd = float(want["ssd"][1, 1])
    assert abs(res.psnr[1, 1] - 20 * np.log10((want["tmax"][1, 1] - want["tmin"][1, 1]) / np.sqrt(ssd / (H * W)))) < 1e-12


# ----------------------------------------------------------------------------- undefined pixels
@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)])
def test_undefined_pixels_are_counted_exactly_and_stored_as_zero(H, W):
    from diffsplitting_amd.core.validation import validation_report
    nd = {"mean_input": np.float64(100.0), "std_input": np.float64(50.0), "mean_target": np.array([100.0, 200.0]),
          "std_target": np.array([50.0, 25.0])}
    rng = np.random.default_rng(3)
    tar = rng.uniform(-1, 1, size=(2, 2, H, W)).astype(np.float32)
    pred = rng.uniform(-1, 1, size=(2, 2, H, W)).astype(np.float32)
    inp = rng.uniform(-1, 1, size=(2, 1, H, W)).astype(np.float32)
    tar[0, 0, 0, 1] = np.nan
    tar[1, 1, 2, 3] = -2.5            # 200 - 62.5 > 0: defined
    tar[1, 0, 4, 6] = -2.5            # 100 - 125 < 0: undefined
    tar[0, 1, 1, 1] = 3000.0          # 75200 >= 65536: undefined
    pred[0, 0, 0, 1] = np.nan         # the same pixel as the NaN target: both count
    pred[1, 1, 4, 0] = np.nan
    pred[0, 1, 3, 3] = np.inf         # clamped, defined
    pred[0, 1, 3, 4] = -np.inf
    inp[1, 0, 0, 0] = np.nan
    inp[0, 0, 4, 4] = -2.5            # (100 - 125) / 2 < 0
    inp[0, 0, 2, 2] = 2700.0          # (135100) / 2 >= 65536
    inp[1, 0, 2, 2] = 2600.0          # 130100 / 2 = 65050: defined
    want = _numpy_report(inp, tar, pred, nd)
    assert want["undefined"] == 8
    res = validation_report(torch.from_numpy(inp).cuda(), torch.from_numpy(tar).cuda(), torch.from_numpy(pred).cuda(), nd)
    assert res.undefined == 8
    _assert_equal(res, want, visuals=True)
    tq, pq, iq = _np(res.target_q), _np(res.pred_q), _np(res.input_q)
    assert tq[0, 0, 0, 1] == 0 and tq[1, 0, 4, 6] == 0 and tq[0, 1, 1, 1] == 0 and tq[1, 1, 2, 3] == 137
    assert pq[0, 0, 0, 1] == 0 and pq[0, 1, 3, 3] == 65535 and pq[0, 1, 3, 4] == 0
    assert iq[1, 0, 0, 0] == 0 and iq[0, 0, 4, 4] == 0 and iq[0, 0, 2, 2] == 0 and iq[1, 0, 2, 2] == 65050


def test_refuses_wrong_shapes_and_strided_tensors():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core.validation import validation_report
    nd = {"mean_input": 1.0, "std_input": 1.0, "mean_target": np.ones(2), "std_target": np.ones(2)}
    x, t = torch.zeros(2, 1, 8, 8, device="cuda"), torch.zeros(2, 2, 8, 8, device="cuda")
    with pytest.raises(DsxError, match="prediction must be"):
        validation_report(x, t, torch.zeros(2, 1, 8, 8, device="cuda"), nd)
    with pytest.raises(DsxError, match="strided"):
        validation_report(x, t.transpose(2, 3), t, nd)
    with pytest.raises(DsxError, match="one value per target channel"):
        validation_report(x, t, t, dict(nd, mean_target=np.ones(3)))


# ----------------------------------------------------------------------------- validate, split --validate
def _frames(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, h, w, 2), dtype=np.float32) * 1000.0).astype(np.float32)


def test_validate_equals_the_report_applied_by_hand(tmp_path, caplog):
    """A random-init InDI model (inner_channel 16), 32 x 32 items, 3 items in batches of 2: validate's values are those
    of validation_report on the very tensors the model produced, and the files are the images' 16-bit renderings."""
    from PIL import Image
    from diffsplitting_amd.core.validation import group_psnr, validate, validation_report
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    from diffsplitting_amd.model import create_model
    torch.manual_seed(11)
    model = create_model(nets.opt(nets.tiny_indi_section()))
    model.set_new_noise_schedule({"n_timestep": 2}, schedule_phase="val")
    fr = _frames(2, 64, 64)
    val_set = SplitDataset("Hagen", DataLocation(arrays=(fr[..., 0], fr[..., 1])), 32, device="cuda")
    seen, test = [], model.test

    def recording_test(*a, **k):
        test(*a, **k)
        seen.append((model.data["input"].clone(), model.data["target"].clone(), model.netG.last_full_batch.clone()))

    model.test = recording_test
    out_dir = str(tmp_path / "results" / "7")
    caplog.set_level(logging.WARNING, logger="base")
    avg, per_channel = validate(model, val_set, n_items=3, batch=2, result_path=out_dir, current_step=40)
    assert [s[0].shape[0] for s in seen] == [2, 1] and seen[0][2].shape == (2, 2, 32, 32)
    nd = val_set.get_normalization_dict()
    by_hand = {0: [], 1: []}
    reports = [validation_report(i, t, p, nd) for i, t, p in seen]
    for r in reports:
        for ch, vals in group_psnr(r).items():
            by_hand[ch].extend(vals)
    assert per_channel == by_hand and all(len(v) == 3 for v in per_channel.values())
    assert avg == float(np.mean([np.mean(v) for v in by_hand.values()])) and np.isfinite(avg)
    assert not [r for r in caplog.records if "uint16" in r.getMessage()] or sum(r.undefined for r in reports) > 0
    names = sorted(os.listdir(out_dir))
    assert names == sorted(f"40_{i}_{k}.png" for i in (1, 2, 3) for k in ("target", "input", "pred"))
    with Image.open(os.path.join(out_dir, "40_3_pred.png")) as im:    # item 3 = item 0 of the second batch
        px = np.array(im)
    img = np.nan_to_num(reports[1].pred_img[0], nan=0.0, posinf=1.0)
    assert px.shape == (32, 64) and np.array_equal(px[:, 32:], np.rint(65535.0 * np.clip(img[1], 0, 1)).astype(np.int64))


def _config(tmp_path):
    cfg = {"name": "tiny_hagen_indi", "phase": "train", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"val": {"name": "Hagen", "patch_size": 64, "datatype": "img"}}, "model": nets.tiny_indi_section()}
    p = tmp_path / "tiny.json"
    p.write_text(json.dumps(cfg, indent=2))
    return ["-c", str(p), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--synthetic", "2,64,64", "--steps", "2",
            "--batch-tiles", "4"]


def test_split_validate_logs_the_psnr_line_and_leaves_the_plain_run_alone(tmp_path, caplog):
    from diffsplitting_amd import split
    argv = _config(tmp_path)
    torch.manual_seed(5)
    plain = split.main(argv)
    caplog.set_level(logging.INFO, logger="base")
    torch.manual_seed(5)
    out_dir = str(tmp_path / "val_out")
    avg = split.main(argv + ["--validate", "--results", out_dir])
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("# Validation # PSNR: ")]
    assert len(lines) == 1 and lines[0] == "# Validation # PSNR: {:.4e}".format(avg)
    assert isinstance(avg, float) and np.isfinite(avg)
    assert len(os.listdir(out_dir)) == 6                             # two 64 x 64 items, three files each
    torch.manual_seed(5)
    again = split.main(argv)                                          # without the flag: as before
    assert torch.is_tensor(plain) and plain.shape == (2, 64, 64, 2) and torch.equal(plain, again)
