"""The SR3 image path on the MI355X: the resize kernels against PIL's own bytes (tests/golden/resize_pil.npz) and the
numpy restatement (tests/resize_ref.py) with 0 differing bytes, ToTensor bitwise against torch on the CPU, prepare(),
and the path end to end (image folder -> LRHRDataset -> DDPM.test / infer.main) against the oracle.  `-m gpu`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, samplers
from tests import resize_ref as R
from tests.gpu_util import maxabs
from tests.resize_cases import check_case, load_fixture, make_input
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FP32_TOL = 1e-3                      # the project's fp32 bar against the oracle (tests/test_gpu_boundary.py)


def _diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).sum())


def test_fixture_cases_through_resize_multiple():
    from diffsplitting_amd.data import prepare_data as P
    from PIL import Image
    z, meta = load_fixture()
    for i, m in enumerate(meta["cases"]):
        a = make_input(m["seed"], m["h"], m["w"], m["mode"])
        outs = P.resize_multiple(a, tuple(m["sizes"]), m["filter"])
        assert all(isinstance(o, np.ndarray) and o.dtype == np.uint8 for o in outs)
        check_case(z, i, m, outs)
        pil = P.resize_multiple(Image.fromarray(a), tuple(m["sizes"]), m["filter"])       # PIL in, PIL out
        assert all(isinstance(o, Image.Image) and o.mode == m["mode"] for o in pil)
        check_case(z, i, m, [np.asarray(o) for o in pil])


def test_batch_equals_one_image_at_a_time():
    from diffsplitting_amd.data import prepare_data as P
    rng = np.random.default_rng(21)
    for (h, w), sizes, kind in [((218, 178), (16, 128), R.BICUBIC), ((200, 300), (16, 128), R.BILINEAR),
                                ((64, 48), (8, 32), R.BICUBIC)]:
        a = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
        batch = [o.cpu().numpy() for o in P.resize_multiple(torch.from_numpy(a).cuda(), sizes, kind)]
        for b in range(5):
            one = P.resize_multiple(a[b], sizes, kind)
            ref = R.resize_multiple(a[b], sizes, kind)
            for k in range(3):
                assert _diff(batch[k][b], one[k]) == 0 and _diff(one[k], ref[k]) == 0, ((h, w), b, k)


def _run_plan(src, oh, ow, top, left, ch, cw, kind):
    """dsx_resize_u8 of a (B, H, W, C) uint8 array with an explicit output window."""
    from diffsplitting_amd._lib import check, lib
    B, H, W, Cn = src.shape
    h = C.c_void_p()
    check(lib.dsx_resize_plan_create(H, W, oh, ow, top, left, ch, cw, kind, Cn, C.byref(h)))
    try:
        t = torch.from_numpy(src).cuda()
        out = torch.empty((B, ch, cw, Cn), dtype=torch.uint8)
        guard = torch.full((B * ch * cw * Cn + 64,), 99, dtype=torch.uint8, device="cuda")     # the output sits inside it,
        view = guard[33:33 + out.numel()].view(out.shape)                                       # at an odd address
        ws = torch.empty((max(1, lib.dsx_resize_workspace_bytes(h, B)),), dtype=torch.uint8, device="cuda")
        check(lib.dsx_resize_u8(h, C.c_void_p(t.data_ptr()), B, C.c_void_p(view.data_ptr()), C.c_void_p(ws.data_ptr()), None))
        torch.cuda.synchronize()
        assert bool((guard[:33] == 99).all()) and bool((guard[33 + out.numel():] == 99).all())   # nothing outside it
        return view.cpu().numpy()
    finally:
        lib.dsx_resize_plan_destroy(h)


@pytest.mark.parametrize("kind", [R.BILINEAR, R.BICUBIC])
def test_crop_window_equals_slicing(kind):
    rng = np.random.default_rng(4)
    #            H    W   oh   ow  top left  ch  cw        (both passes, one pass skipped, none)
    for H, W, oh, ow, top, left, ch, cw in [(200, 300, 128, 192, 0, 32, 128, 128), (218, 178, 19, 16, 2, 0, 16, 16),
                                            (97, 131, 128, 172, 0, 22, 128, 128), (33, 47, 61, 20, 7, 3, 41, 13),
                                            (64, 48, 64, 20, 5, 2, 50, 11), (64, 48, 20, 48, 3, 7, 9, 30),
                                            (40, 24, 40, 24, 4, 5, 30, 10), (40, 24, 40, 24, 0, 5, 40, 10)]:
        for Cn in (1, 3):
            src = rng.integers(0, 256, (2, H, W, Cn), dtype=np.uint8)
            full = _run_plan(src, oh, ow, 0, 0, oh, ow, kind)
            win = _run_plan(src, oh, ow, top, left, ch, cw, kind)
            assert _diff(win, full[:, top:top + ch, left:left + cw]) == 0, (H, W, oh, ow, Cn)
            for b in range(2):
                assert _diff(full[b], R.resize(src[b], oh, ow, kind)) == 0, (H, W, oh, ow, Cn, b)


def test_u8_to_tensor_bitwise():
    from diffsplitting_amd.data import util as Util
    rng = np.random.default_rng(9)
    ramp = np.arange(256, dtype=np.uint8)
    inputs = [ramp.reshape(1, 16, 16, 1), np.stack([ramp, ramp[::-1], np.roll(ramp, 7)], -1).reshape(2, 8, 16, 3),
              rng.integers(0, 256, (3, 7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (2, 9, 3, 1), dtype=np.uint8)]
    for mm in [(0, 1), (-1, 1)]:
        for u in inputs:
            got = Util.u8_to_tensor(torch.from_numpy(u).cuda(), mm).cpu()
            exp = torch.from_numpy(u).permute(0, 3, 1, 2).to(torch.float32).div(255)            # ToTensor, on the CPU
            exp = exp * (mm[1] - mm[0]) + mm[0]                                                  # data/util.py:82
            assert got.shape == exp.shape and got.dtype == torch.float32
            assert torch.equal(got.view(torch.int32), exp.contiguous().view(torch.int32)), (mm, u.shape)
            for b in range(u.shape[0]):
                assert np.array_equal(got[b].numpy(), R.to_tensor(u[b], mm))
    one, two = Util.transform_augment([inputs[1][0], torch.from_numpy(inputs[2]).cuda()], split="val", min_max=(-1, 1))
    assert one.shape == (3, 8, 16) and two.shape == (3, 3, 7, 5) and one.is_cuda
    assert np.array_equal(one.cpu().numpy(), R.to_tensor(inputs[1][0], (-1, 1)))


def test_prepare_writes_the_fixture_bytes(tmp_path):
    from diffsplitting_amd.data import prepare_data as P
    from PIL import Image
    z, meta = load_fixture()
    picked = {}
    for i, m in enumerate(meta["cases"]):
        if m["how"] == "full" and m["mode"] == "RGB" and m["filter"] == R.BICUBIC:
            picked[str(len(picked) + 1)] = (i, m)
            sub = tmp_path / "src" / ("a" if len(picked) % 2 else "b")
            sub.mkdir(parents=True, exist_ok=True)
            Image.fromarray(make_input(m["seed"], m["h"], m["w"], m["mode"])).save(sub / f"{len(picked)}.png")
    assert len(picked) >= 4
    out = tmp_path / "out_16_128"
    assert P.prepare(str(tmp_path / "src"), str(out), 3, sizes=(16, 128), resample=P.BICUBIC) == len(picked)
    for name, (i, m) in picked.items():
        files = [out / "lr_16" / f"{name.zfill(5)}.png", out / "hr_128" / f"{name.zfill(5)}.png",
                 out / "sr_16_128" / f"{name.zfill(5)}.png"]
        check_case(z, i, m, [np.asarray(Image.open(f)) for f in files])
    # the folders are what LRHRDataset(datatype='img') reads: items are the fixture bytes through to_tensor
    from diffsplitting_amd.data.LRHR_dataset import LRHRDataset
    ds = LRHRDataset(str(out), "img", 16, 128, split="val", data_len=-1, need_LR=True)
    item = ds[1]
    i, m = picked["2"]
    assert set(item) == {"LR", "HR", "SR", "Index", "input", "target"} and item["Index"] == 1
    for key, name in (("LR", "lr"), ("HR", "hr"), ("SR", "sr")):
        assert np.array_equal(item[key].cpu().numpy(), R.to_tensor(z[f"c{i}_{name}"], (-1, 1)))
    assert item["input"] is item["SR"] and item["target"] is item["HR"]


def _sr3_section():
    return {"which_model_G": "sr3", "finetune_norm": False,
            "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": 32, "norm_groups": 32,
                     "channel_multiplier": [1, 2, 4], "attn_res": [16], "res_blocks": 2, "dropout": 0.2},
            "beta_schedule": {"train": dict(cases.SCHEDULES["lin_8"]), "val": dict(cases.SCHEDULES["lin_8"])},
            "diffusion": {"image_size": 32, "channels": 3, "conditional": True}}


def test_image_folder_to_samples_end_to_end(tmp_path):
    """A folder of 64 x 48 images -> hr_only dataset (8 / 32) -> create_dataloader -> DDPM.feed_data / test against the
    oracle's SR3 loop on the same SR tensors and the same injected draws; then infer.main on the same folder."""
    from diffsplitting_amd import data as Data
    from diffsplitting_amd import infer
    from diffsplitting_amd.core import metrics as Metrics
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.model import create_model
    from PIL import Image
    rng = np.random.default_rng(12)
    src = tmp_path / "src"
    src.mkdir()
    images = []
    for k in range(3):
        y, x = np.mgrid[0:64, 0:48]
        smooth = np.stack([127 + 100 * np.sin(x / (5.0 + k) + c) * np.cos(y / (7.0 + c)) for c in range(3)], -1)
        a = np.clip(smooth + rng.normal(0, 12, smooth.shape), 0, 255).astype(np.uint8)
        images.append(a)
        Image.fromarray(a).save(src / f"{k}.png")
    dataset_opt = dict_to_nonedict({"name": "tiny", "mode": "LRHR", "dataroot": str(src), "datatype": "hr_only",
                                    "l_resolution": 8, "r_resolution": 32, "data_len": -1})
    val_set = Data.create_dataset(dataset_opt, "val")
    loader = Data.create_dataloader(val_set, dataset_opt, "val")
    assert len(val_set) == 3 and loader.batch_size == 1 and loader.num_workers == 0
    sd, _ = golden_state_dict("loop_sr3_lin_8")
    osd = {"denoise_fn." + k: v for k, v in sd.items()}
    opt = dict_to_nonedict({"model": _sr3_section(), "phase": "val", "gpu_ids": [0], "distributed": False,
                            "path": {"resume_state": None, "checkpoint": str(tmp_path)}})
    model = create_model(opt)
    missing, unexpected = model.netG.load_state_dict(osd, strict=False)
    assert not unexpected and all(not k.startswith("denoise_fn.") for k in missing)
    model.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    sch = samplers.gaussian_schedule(cases.SCHEDULES["lin_8"])
    cfg = cases.UNET_CASES["sr3_tiny"]["cfg"]
    model.netG.noise_source = lambda shape: torch.randn(shape)
    seen = 0
    for k, data in enumerate(loader):
        lr, hr, sr = R.resize_multiple(images[k], (8, 32), R.BICUBIC)
        assert data["SR"].shape == (1, 3, 32, 32) and data["SR"].is_cuda and int(data["Index"][0]) == k
        assert np.array_equal(data["SR"][0].cpu().numpy(), R.to_tensor(sr, (-1, 1)))
        assert np.array_equal(data["HR"][0].cpu().numpy(), R.to_tensor(hr, (-1, 1)))
        assert np.array_equal(data["LR"][0].cpu().numpy(), R.to_tensor(lr, (-1, 1)))
        cond = data["SR"].cpu().clone()
        torch.manual_seed(cases.LOOP_SEED + k)
        model.feed_data(data)
        model.test(continuous=False)
        pred = model.get_current_visuals()["prediction"]
        torch.manual_seed(cases.LOOP_SEED + k)
        ref = samplers.sr3_p_sample_loop(osd, cfg, sch, cond, randn=lambda s: torch.randn(s))
        err = maxabs(pred.numpy(), ref.numpy())
        print(f"end to end image {k}: max|hip - oracle| = {err:.3e}")
        assert pred.shape == (3, 32, 32) and err <= FP32_TOL, err
        seen += 1
    assert seen == 3
    # the batched form of the dataset gives the same items
    b = val_set.batch([2, 0])
    assert b["SR"].shape == (2, 3, 32, 32) and b["Index"].tolist() == [2, 0]
    assert torch.equal(b["HR"][1], val_set[0]["HR"]) and torch.equal(b["SR"][0], val_set[2]["SR"])

    # infer.main on the same folder: a checkpoint in the reference's naming, a config JSON in its schema
    model.save_network(epoch=1, iter_step=10)
    cfg_json = {"name": "tiny_sr3", "phase": "val", "gpu_ids": [0],
                "path": {"log": str(tmp_path / "logs"), "results": str(tmp_path / "results"),
                         "checkpoint": str(tmp_path), "resume_state": str(tmp_path / "I10_E1")},
                "datasets": {"val": {"name": "tiny", "mode": "LRHR", "dataroot": "unused", "datatype": "hr_only",
                                     "l_resolution": 8, "r_resolution": 32, "data_len": -1}},
                "model": _sr3_section()}
    p = tmp_path / "tiny_sr3.json"
    p.write_text(json.dumps(cfg_json, indent=2).replace('"name": "tiny_sr3",', '"name": "tiny_sr3", // comment'))
    res = infer.main(["-c", str(p), "-p", "val", "-gpu", "0", "--dataroot", str(src), "--batch", "2", "--seed", "5"])
    psnrs, ssims = [], []
    for idx in range(1, 4):
        files = [tmp_path / "results" / f"0_{idx}_{kind}.png" for kind in ("hr", "sr", "inf")]
        assert all(f.exists() for f in files), files
        hr_png, sr_png, inf_png = (np.asarray(Image.open(f)) for f in files)
        assert hr_png.shape == sr_png.shape == inf_png.shape == (32, 32, 3)
        _, hr, sr = R.resize_multiple(images[idx - 1], (8, 32), R.BICUBIC)
        assert np.array_equal(hr_png[:, :, ::-1], hr) and np.array_equal(inf_png[:, :, ::-1], sr)   # save_img: cv2's order
        psnrs.append(Metrics.calculate_psnr(sr_png, hr_png))
        ssims.append(Metrics.calculate_ssim(sr_png, hr_png))
    assert len(res["files"]) == 3 and not (tmp_path / "results" / "0_4_hr.png").exists()
    print(f"infer: PSNR {res['psnr']:.6f} (files {np.mean(psnrs):.6f}), SSIM {res['ssim']:.8f} (files {np.mean(ssims):.8f})")
    # the same uint8 values and the same kernel on both sides: equal up to the order of the final mean
    assert abs(res["psnr"] - np.mean(psnrs)) <= 1e-9 and abs(res["ssim"] - np.mean(ssims)) <= 1e-9
    assert 5.0 < res["psnr"] < 60.0 and -1.0 <= res["ssim"] <= 1.0
