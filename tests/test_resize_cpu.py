"""The SR3 image path without a GPU: the numpy restatement of PIL's resampler (tests/resize_ref.py) against PIL itself
and against the fixture PIL wrote (tests/golden/resize_pil.npz, tools/gen_resize_golden.py), the host-side coefficient
tables of libdsx against the restatement, the size / crop arithmetic, the refusals, the folder helpers and the reference
import lines.  Every bar here is "0 differing bytes" / "equal integers": the resampler is integer arithmetic."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import resize_ref as R
from tests.resize_cases import check_case, load_fixture, make_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_pil_fixture():
    z, meta = load_fixture()
    assert re.match(r"\d+\.\d+", meta["pil_version"])
    names = [m["name"] for m in meta["cases"]]
    assert len(names) >= 10 and any(m["mode"] == "L" for m in meta["cases"])
    for i, m in enumerate(meta["cases"]):
        a = make_input(m["seed"], m["h"], m["w"], m["mode"])
        check_case(z, i, m, R.resize_multiple(a, tuple(m["sizes"]), m["filter"]))


def test_restatement_equals_pil_live():
    from PIL import Image
    rng = np.random.default_rng(0)
    for (h, w), (oh, ow) in [((33, 47), (20, 61)), ((178, 218), (16, 19)), ((64, 48), (8, 10)), ((1024, 16), (16, 16)),
                             ((300, 157), (157, 300)), ((40, 40), (40, 17))]:
        for kind in (R.BILINEAR, R.BICUBIC):
            for c in (1, 3):
                a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
                src = a[:, :, 0] if c == 1 else a
                got = R.resize(src, oh, ow, kind)
                exp = np.asarray(Image.fromarray(src).resize((ow, oh), kind))
                assert int((got != exp).sum()) == 0, ((h, w), (oh, ow), kind, c)


@pytest.mark.parametrize("kind", [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize("sizes", [(16, 128), (128, 16), (1024, 16), (178, 16), (300, 157), (64, 64), (7, 7)])
def test_library_coefficients_equal_the_restatement(kind, sizes):
    from diffsplitting_amd import _lib
    lib = _lib.lib
    n_in, n_out = sizes
    xmin, n, k = R.coeffs(n_in, n_out, kind)
    cap = lib.dsx_resize_coeffs(n_in, n_out, kind, None, None, None, 0)
    assert cap == k.shape[1]
    cap += 3                                              # a wider row: zero padded
    gx, gn, gk = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * (n_out * cap))()
    assert lib.dsx_resize_coeffs(n_in, n_out, kind, gx, gn, gk, cap) == k.shape[1]
    assert np.array_equal(np.array(gx), xmin) and np.array_equal(np.array(gn), n)
    gk = np.array(gk).reshape(n_out, cap)
    assert np.array_equal(gk[:, :k.shape[1]], k) and not gk[:, k.shape[1]:].any()
    assert (np.arange(cap)[None, :] >= n[:, None])[gk != 0].sum() == 0        # nothing past a row's taps
    if n_in == 1024 and kind == R.BICUBIC:
        assert k.shape[1] == 257 and int(n.max()) == 256   # tap counts are not bounded by a small constant


def test_size_and_crop_arithmetic():
    from diffsplitting_amd.data import prepare_data as P
    for h, w, size, exp in [(218, 178, 16, (19, 16, 2, 0)), (218, 178, 128, (156, 128, 14, 0)),
                            (200, 300, 16, (16, 24, 0, 4)), (200, 300, 128, (128, 192, 0, 32)),
                            (97, 131, 128, (128, 172, 0, 22)), (1024, 768, 64, (85, 64, 10, 0)),
                            (256, 256, 16, (16, 16, 0, 0)), (16, 40, 16, (16, 40, 0, 12))]:
        assert P.geometry(h, w, size) == exp, (h, w, size)
        assert R.resize_and_convert(np.zeros((h, w, 3), np.uint8), size, R.BILINEAR).shape == (size, size, 3)
    assert P.geometry(300, 16, 16) is None and P.geometry(16, 16, 16) is None     # img.size[0] == size: untouched
    assert P.resize_size(5, 3, 2) == (3, 2) and P.crop_offsets(19, 16, 16) == (2, 0)   # int() truncates, round() half-even
    assert P.crop_offsets(21, 16, 16) == (2, 0) and P.crop_offsets(23, 16, 16) == (4, 0)
    assert (P.BILINEAR, P.BICUBIC) == (R.BILINEAR, R.BICUBIC) == (2, 3)
    from PIL import Image
    assert (int(Image.BILINEAR), int(Image.BICUBIC)) == (2, 3)


def test_refusals():
    from diffsplitting_amd import _lib
    from diffsplitting_amd import data as Data
    from diffsplitting_amd.data import prepare_data as P
    from diffsplitting_amd.data import util as Util
    from diffsplitting_amd.data.LRHR_dataset import LRHRDataset
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    h = C.c_void_p()
    create = lambda *a: lib.dsx_resize_plan_create(*a, C.byref(h))
    assert lib.dsx_resize_coeffs(16, 128, 1, None, None, None, 0) == -1 and "filter id 1" in err()
    assert lib.dsx_resize_coeffs(0, 128, 3, None, None, None, 0) == -1 and "sizes" in err()
    buf = (C.c_int32 * 64)()
    assert lib.dsx_resize_coeffs(128, 16, 3, buf, buf, buf, 4) == -1 and "capacity" in err()
    assert create(64, 48, 10, 8, 0, 0, 8, 8, 7, 3) == -1 and "filter id 7" in err()
    assert create(64, 48, 10, 8, 3, 0, 8, 8, 3, 3) == -1 and "crop window" in err()
    assert create(64, 48, 10, 8, 0, -1, 8, 8, 3, 3) == -1 and "crop window" in err()
    assert create(64, 48, 10, 8, 0, 0, 8, 9, 3, 3) == -1 and "crop window" in err()
    assert create(64, 48, 10, 8, 0, 0, 8, 8, 3, 2) == -1 and "C = 2" in err()
    assert create(64, 0, 10, 8, 0, 0, 8, 8, 3, 3) == -1 and "sizes" in err()
    assert create(200000, 8, 1, 8, 0, 0, 1, 8, 3, 3) == -1 and "LDS" in err()
    assert create(64, 48, 10, 8, 1, 0, 8, 8, 3, 3) == 0 and h.value          # a valid plan needs no device
    assert lib.dsx_resize_workspace_bytes(h, 5) == 5 * 8 * 3 * (R.coeffs(64, 10, 3)[0][8] + R.coeffs(64, 10, 3)[1][8]
                                                              - R.coeffs(64, 10, 3)[0][1])
    lib.dsx_resize_plan_destroy(h)
    with pytest.raises(_lib.DsxError, match="lmdb"):
        LRHRDataset("/nonexistent", "lmdb")
    with pytest.raises(_lib.DsxError, match="lmdb"):
        P.prepare("/nonexistent", "/nonexistent_out", 1, lmdb_save=True)
    with pytest.raises(_lib.DsxError, match="lmdb"):
        P.main(["--path", "/nonexistent", "--out", "/nonexistent_out", "--lmdb"])
    with pytest.raises(_lib.DsxError, match="train"):
        Util.transform_augment([np.zeros((4, 4, 3), np.uint8)], split="train")
    with pytest.raises(_lib.DsxError, match="train"):
        Data.create_dataset({"mode": "HR"}, "train")
    with pytest.raises(_lib.DsxError, match="train"):
        Data.create_dataloader([], {}, "train")
    with pytest.raises(NotImplementedError):
        LRHRDataset("/nonexistent", "tif")


def _write_pngs(folder, names, size=8):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for k, n in enumerate(names):
        Image.fromarray(np.full((size, size, 3), k, np.uint8)).save(os.path.join(folder, n))


def test_image_folders(tmp_path):
    from diffsplitting_amd import _lib
    from diffsplitting_amd.data import prepare_data as P
    from diffsplitting_amd.data import util as Util
    from diffsplitting_amd.data.LRHR_dataset import LRHRDataset
    assert Util.is_image_file("a.PNG") and Util.is_image_file("b.jpeg") and not Util.is_image_file("c.txt")
    assert ".png" in Util.IMG_EXTENSIONS and len(Util.IMG_EXTENSIONS) == 10
    root = tmp_path / "imgs"
    _write_pngs(root / "b", ["2.png", "10.png"])
    _write_pngs(root / "a", ["z.png"])
    _write_pngs(root, ["m.png"])
    (root / "notes.txt").write_text("x")
    got = Util.get_paths_from_images(str(root))
    exp = sorted(os.path.join(str(root), p) for p in ("m.png", "a/z.png", "b/10.png", "b/2.png"))
    assert got == exp                                   # sorted full paths, as data/util.py:15-24
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("x")
    with pytest.raises(AssertionError, match="no valid image file"):
        Util.get_paths_from_images(str(empty))
    with pytest.raises(AssertionError, match="not a valid directory"):
        Util.get_paths_from_images(str(tmp_path / "missing"))
    with pytest.raises(_lib.DsxError, match="no valid image file"):
        P.prepare(str(empty), str(tmp_path / "out"), 1)
    # __len__ and data_len clipping need no GPU
    ds_root = tmp_path / "ds"
    names = [f"{i:05d}.png" for i in range(5)]
    for sub in ("lr_8", "hr_32", "sr_8_32"):
        _write_pngs(ds_root / sub, names)
    for data_len, exp_len in [(-1, 5), (0, 5), (3, 3), (9, 5)]:
        ds = LRHRDataset(str(ds_root), "img", l_resolution=8, r_resolution=32, split="val", data_len=data_len, need_LR=True)
        assert len(ds) == exp_len and ds.dataset_len == 5
    assert ds.hr_path[0].endswith("hr_32/00000.png") and ds.sr_path[4].endswith("sr_8_32/00004.png")
    assert ds.lr_path[1].endswith("lr_8/00001.png")
    assert len(LRHRDataset(str(root), "hr_only", 8, 32, "val", 2)) == 2
    with pytest.raises(AssertionError, match="not a valid directory"):
        LRHRDataset(str(ds_root), "img", l_resolution=16, r_resolution=128, split="val")


def test_reference_import_lines_resolve(tmp_path):
    code = ("import data as Data\n"
            "from data.LRHR_dataset import LRHRDataset\n"
            "import data.util as Util\n"
            "import diffsplitting_amd.data as real\n"
            "import diffsplitting_amd.data.LRHR_dataset as real_ds\n"
            "assert Data is real and Data.create_dataset is real.create_dataset and Data.create_dataloader\n"
            "assert LRHRDataset is real_ds.LRHRDataset and Util.transform_augment\n"
            "print('compat ok')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "diffsplitting_amd", "compat"), ROOT])
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compat ok" in r.stdout, r.stderr[-2000:]


def test_new_symbols_declared_bound_and_exported():
    from diffsplitting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in ("dsx_resize_coeffs", "dsx_resize_plan_create", "dsx_resize_plan_destroy", "dsx_resize_workspace_bytes",
                 "dsx_resize_u8", "dsx_u8_to_tensor"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "prepare_data.py:17-40" in hdr and "data/util.py:74-83" in hdr        # the reference lines they follow
    assert _lib.lib.dsx_abi_version() == 2 and "#define DSX_ABI_VERSION 2" in hdr


def test_to_tensor_reference_is_torch_cpu():
    """The float32 to_tensor of resize_ref is what torch computes on the CPU (the GPU test compares the kernel with it)."""
    import torch
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    for mm in [(0, 1), (-1, 1)]:
        t = torch.from_numpy(u).permute(2, 0, 1).to(torch.float32).div(255)
        t = t * (mm[1] - mm[0]) + mm[0]
        assert np.array_equal(R.to_tensor(u, mm).view(np.uint32), t.numpy().view(np.uint32))


def test_kernel_source_has_no_scalar_memory_writes():
    """dsx_resize.hip is plain C++: no inline assembly at all."""
    src = open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "dsx_resize.hip")).read()
    assert "asm" not in src.replace("k_resize", "") and "__builtin_amdgcn" not in src
    assert "dsx_resize.hip" in open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "build.sh")).read()
