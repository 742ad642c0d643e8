"""The CIFAR data path on the MI355X (`-m gpu`): the items the reference's own SplitDataset('cifar10') wrote
(tests/golden/cifar_items.npz) bit for bit through dsx_tiles_gather_norm_planes, the entry point called directly
(Cc = 1 against the grey export, ragged shapes inside NaN-filled buffers, argument errors) and split.main from the
config's directories to the report, the RGB triples and the written predictions.  Nothing here reads the reference."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

from tests import nets
from tests import cifar_files as CF
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ERR_INVALID = -1                                                     # DSX_ERR_INVALID


def _f32(a):
    """a tensor or an array as a host array, which must be float32"""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return a


@pytest.fixture(scope="module")
def val_dir(tmp_path_factory):
    return CF.write_dir(tmp_path_factory.mktemp("cifar") / "all")


# ----------------------------------------------------------------------------- the reference's items
@pytest.mark.parametrize("tag,patch,kw", [
    ("p32_w11", 32, dict(channel_weights=[1, 1])),
    ("p16_w11", 16, dict(channel_weights=None)),
    ("p32_w103", 32, dict(channel_weights=[1, 0.3])),
    ("p16_w103", 16, dict(channel_weights=[1, 0.3])),
    ("first8", 32, dict()),
    ("custom", 32, dict(channel_weights=[1, 0.3], normalization_dict="custom_nd")),
    ("tci4", 16, dict(target_channel_idx=4)),
])
def test_items_bit_equal_to_the_reference(val_dir, tag, patch, kw):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    g = CF.fixture()
    if "normalization_dict" in kw:
        kw = dict(kw, normalization_dict=CF.normalization_dict(kw["normalization_dict"]))
    ds = SplitDataset("cifar10", DataLocation(directory=val_dir), patch, max_qval=1.0, **kw)
    assert ds._dev[0].is_cuda and ds._dev[0].dtype == torch.float32 and ds._dev[0].shape == (13, 3, 32, 32)
    idx = [int(i) for i in g[f"{tag}_indices"]]
    out = ds.tiles(idx)
    for k in ("input", "target"):
        want = g[f"{tag}_{k}"]
        assert tuple(out[k].shape) == want.shape and out[k].is_contiguous()
        assert same_bits(_f32(out[k]), _f32(want)), (tag, k)      # tolerance zero: same operations, same order
    item = ds[idx[-1]]
    assert item["input"].shape == g[f"{tag}_input"].shape[1:] and isinstance(item["target"], np.ndarray)
    assert same_bits(_f32(item["target"]), _f32(g[f"{tag}_target"][-1]))


# ----------------------------------------------------------------------------- the entry point, called directly
_call, _numpy_items = CF.gather_planes, CF.numpy_items


def test_one_plane_equals_the_grey_export():
    from diffsplitting_amd._lib import check, lib
    rng = np.random.default_rng(5)
    N, H, W, ph, pw = 3, 37, 53, 16, 24
    a = torch.from_numpy(rng.integers(0, 4000, size=(N, H, W)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.integers(0, 3000, size=(N, H, W)).astype(np.float32)).cuda()
    loc = np.array([(0, 0, 0), (2, H - ph, W - pw), (1, 5, 7), (1, 5, 7), (2, 0, W - pw), (0, H - ph, 0)], dtype=np.int64)
    w, norm = (1.0, 0.3), (1246.59, 1211.3, 759.685, 741.25, 486.905, 470.5)
    new_in = torch.empty((len(loc), 1, ph, pw), device="cuda")
    new_tar = torch.empty((len(loc), 2, ph, pw), device="cuda")
    old_in, old_tar = torch.empty_like(new_in), torch.empty_like(new_tar)
    check(_call(a, b, (N, 1, H, W), (ph, pw), loc, w, norm[0], norm[1], [norm[2], norm[4]], [norm[3], norm[5]], new_in, new_tar))
    check(lib.dsx_tiles_gather_norm(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), nets.i64(N, H, W), nets.i64(1, ph, pw),
                                    loc.ctypes.data_as(C.POINTER(C.c_int64)), None, len(loc), w[0], w[1],
                                    (C.c_double * 6)(*norm), 0, C.c_void_p(old_in.data_ptr()), C.c_void_p(old_tar.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert same_bits(_f32(new_in), _f32(old_in)) and same_bits(_f32(new_tar), _f32(old_tar))
    assert torch.isfinite(new_tar).all() and new_tar.std() > 0.1


def test_direct_call_writes_its_outputs_and_nothing_else():
    """Cc = 3, 37 x 53 frames, 16 x 24 patches at the four frame corners (and inside): the outputs are interior slices
    of NaN-filled buffers whose surroundings stay NaN; the values are the numpy expression of the reference's item."""
    from diffsplitting_amd._lib import check
    rng = np.random.default_rng(11)
    N, Cc, H, W, ph, pw = 2, 3, 37, 53, 16, 24
    a = rng.integers(0, 256, size=(N, Cc, H, W), dtype=np.uint8)
    b = rng.integers(0, 256, size=(N, Cc, H, W), dtype=np.uint8)
    loc = [(0, 0, 0), (1, 0, W - pw), (0, H - ph, 0), (1, H - ph, W - pw), (1, 9, 13)]
    w, mean_inp, std_inp = (1, 0.3), 171.25, 93.5
    mt = np.array([101.0, 117.5, 130.25, 99.0, 140.75, 122.125])
    st = np.array([61.0, 57.5, 70.25, 66.0, 52.75, 63.125])
    want_in, want_tar = _numpy_items(a, b, loc, ph, pw, w, mean_inp, std_inp, mt, st)
    fa, fb = (torch.from_numpy(x.astype(np.float32)).cuda() for x in (a, b))
    pad = 37                                                         # floats in front of and behind each output
    n_in, n_tar = want_in.size, want_tar.size
    buf_in = torch.full((pad + n_in + pad,), float("nan"), device="cuda")
    buf_tar = torch.full((pad + n_tar + pad,), float("nan"), device="cuda")
    check(_call(fa, fb, (N, Cc, H, W), (ph, pw), loc, w, mean_inp, std_inp, mt, st, buf_in.data_ptr() + 4 * pad,
                buf_tar.data_ptr() + 4 * pad))
    torch.cuda.synchronize()
    for buf, n, want in ((buf_in, n_in, want_in), (buf_tar, n_tar, want_tar)):
        host = buf.cpu().numpy()
        assert np.isnan(host[:pad]).all() and np.isnan(host[pad + n:]).all()
        assert same_bits(_f32(host[pad:pad + n].reshape(want.shape)), _f32(want))


def test_bad_arguments_are_refused_before_any_launch():
    from diffsplitting_amd._lib import lib
    N, Cc, H, W, ph, pw = 2, 3, 37, 53, 16, 24
    f = torch.zeros((N, 8, H, W), device="cuda")
    tin = torch.full((2, Cc, ph, pw), float("nan"), device="cuda")
    ttar = torch.full((2, 2 * Cc, ph, pw), float("nan"), device="cuda")
    ones = np.ones(18)
    ok = dict(f0=f, f1=f, shape4=(N, Cc, H, W), patch=(ph, pw), loc=[(0, 0, 0), (1, 1, 1)], w=(1, 1), mean_inp=0.0,
              std_inp=1.0, mt=ones, st=ones, tin=tin, ttar=ttar)
    bad = [
        (dict(shape4=(N, 0, H, W)), "colour planes"), (dict(shape4=(N, 9, H, W)), "colour planes"),
        (dict(patch=(H + 1, pw)), "does not fit"), (dict(patch=(ph, W + 1)), "does not fit"), (dict(patch=(0, pw)), "does not fit"),
        (dict(loc=[(0, 0, 0), (N, 0, 0)]), "item 1 at"), (dict(loc=[(0, H - ph + 1, 0)]), "outside the frames"),
        (dict(loc=[(0, 0, W - pw + 1)]), "outside the frames"), (dict(loc=[(0, -1, 0)]), "outside the frames"),
        (dict(loc=[(-1, 0, 0)]), "outside the frames"), (dict(loc=[(0, 0, 2 ** 32)]), "outside the frames"),
        (dict(f0=None), "null"), (dict(f1=None), "null"), (dict(tin=None), "null"), (dict(ttar=None), "null"),
        (dict(std_inp=0.0), "std"), (dict(st=np.r_[ones[:4], 0.0, ones[5:]]), "target plane 4"),
        (dict(mt=np.r_[np.nan, ones[1:]]), "target plane 0"), (dict(count=-1), "count"), (dict(count=65536), "count"),
    ]
    for change, what in bad:
        rc = _call(**dict(ok, **change))
        assert rc == ERR_INVALID and what in lib.dsx_last_error().decode(), (change, rc, lib.dsx_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(tin).all() and torch.isnan(ttar).all()        # nothing was launched
    assert _call(**dict(ok, count=0)) == 0 and _call(**ok) == 0
    torch.cuda.synchronize()
    assert (tin == 0).all() and (ttar == -1).all()                   # zero frames: (0 + 0 - 0) / 1 and (0 - 1) / 1


# ----------------------------------------------------------------------------- InDI on a colour input
def test_indi_repeats_a_colour_input_to_out_channel_channels():
    """C1 (UNet 6 -> 6) on the fixture's 3-plane inputs: the input is repeated to out_channel channels in all, so the
    objective and the start of the sampling loop see cat([input] * 2) -- the same as handing them that tensor."""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.model import create_model
    g = CF.fixture()
    torch.manual_seed(3)
    model = create_model(nets.opt(CF.model_section()))
    model.set_new_noise_schedule({"n_timestep": 20}, schedule_phase="val")
    model.netG.set_loss("cuda")
    inp, tar = (torch.from_numpy(g[f"first8_{k}"][:2].copy()).cuda() for k in ("input", "target"))
    t, noise = torch.tensor([0.25, 1.0]), torch.randn(tar.shape, device="cuda")
    twice = torch.cat([inp] * 2, dim=1)
    a = model.netG.get_prediction_during_training({"input": inp, "target": tar}, noise, t=t)
    b = model.netG.get_prediction_during_training({"input": twice, "target": tar}, noise, t=t)
    assert a.shape == (2, 6, 32, 32) and torch.isfinite(a).all() and torch.equal(a, b)
    loss = model.netG.p_losses({"input": inp, "target": tar}, noise, t=t)
    assert torch.isfinite(loss).all() and torch.equal(loss, model.netG.p_losses({"input": twice, "target": tar}, noise, t=t))
    torch.manual_seed(9)
    start = model.netG._start(inp, 1.0)
    torch.manual_seed(9)
    assert start.shape == (2, 6, 32, 32) and torch.equal(start, model.netG._start(twice, 1.0))
    with pytest.raises(DsxError, match="no multiple"):
        model.netG._start(torch.cat([inp, inp[:, :1]], dim=1), 1.0)


# ----------------------------------------------------------------------------- split.main on a cifar10 config
@pytest.mark.parametrize("which", ["indi", "ddpm"])
def test_split_main_scores_the_validation_set(tmp_path, caplog, monkeypatch, which):
    """BASELINE's C1 model (``indi``; ``ddpm``: config/splitting_cifar10.json's conditional DDPM, n = 3) with random
    initial weights over 8 items in ragged batches of 3, 3, 2.  Pins what the driver adds -- order, grouping, counts,
    un-normalisation -- not pixels (sampler and report have their own parity tests): the items fed are the fixture's,
    the returned PSNR is validation_report's on the very predictions the model produced, grouped per RGB triple, and
    ``--out`` holds those predictions un-normalised in float64 and rounded once.  (The PSNR is taken from the recorded
    predictions, not from the file: the report truncates the float64 counts, which their float32 rounding does not
    determine.)"""
    from diffsplitting_amd import split
    from diffsplitting_amd.core.validation import group_psnr, validation_report
    g = CF.fixture()
    _, cfg_path = CF.config(tmp_path, which)
    seen, create = [], split.create_model

    def recording_create(opt):
        model = create(opt)
        test = model.test

        def recording_test(*a, **k):
            test(*a, **k)
            seen.append((model.data["input"].clone(), model.data["target"].clone(), model.netG.last_full_batch.clone()))

        model.test = recording_test
        return model

    monkeypatch.setattr(split, "create_model", recording_create)
    out_dir, out_file = str(tmp_path / "triples"), str(tmp_path / "pred.npy")
    argv = ["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--datapath", "--items", "8",
            "--batch-tiles", "3", "--results", out_dir, "--out", out_file]
    with pytest.raises(SystemExit, match=".npy"):
        split.main(argv[:-1] + [str(tmp_path / "pred.tif")])
    assert not seen
    caplog.set_level(logging.INFO, logger="base")
    torch.manual_seed(7)
    avg = split.main(argv)
    assert [s[0].shape[0] for s in seen] == [3, 3, 2]
    fed_in, fed_tar, pred = (torch.cat([s[k] for s in seen]) for k in range(3))
    assert same_bits(_f32(fed_in), _f32(g["first8_input"])) and same_bits(_f32(fed_tar), _f32(g["first8_target"]))
    assert pred.shape == (8, 6, 32, 32) and torch.isfinite(pred).all()
    nd = CF.normalization_dict("nd_w11")
    per_triple = {0: [], 3: []}
    for i, t, p in seen:
        res = validation_report(i, t, p.contiguous(), nd, visuals=False)
        assert res.mode == "RGB"
        for ch, vals in group_psnr(res).items():
            per_triple[ch].extend(vals)
    assert all(len(v) == 8 for v in per_triple.values())
    assert isinstance(avg, float) and np.isfinite(avg) and avg == float(np.mean([np.mean(v) for v in per_triple.values()]))
    lines = [r.getMessage() for r in caplog.records]
    assert [m for m in lines if m.startswith("# Validation # PSNR: ")] == ["# Validation # PSNR: {:.4e}".format(avg)]
    for ch in (0, 3):
        assert "channel %d: PSNR %.4e over 8 items" % (ch, float(np.mean(per_triple[ch]))) in lines
    assert sorted(os.listdir(out_dir)) == sorted(f"0_{i}_{k}.png" for i in range(1, 9) for k in ("target", "input", "pred"))
    saved = np.load(out_file)
    assert saved.dtype == np.float32 and saved.shape == (8, 6, 32, 32)
    raw = (pred.cpu().numpy().astype(np.float64) * nd["std_target"].reshape(1, 6, 1, 1)
           + nd["mean_target"].reshape(1, 6, 1, 1)).astype(np.float32)
    assert same_bits(_f32(saved), _f32(raw))
