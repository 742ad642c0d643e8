"""The validation report's host side (no GPU): the ABI symbol, PSNR and the [0, 1] images formed from the integer
statistics and numerators of the fixtures the reference's own validation block wrote (tools/gen_validation_golden.py),
the channel grouping, the refusals and the 16-bit 'L' file."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("validation_L", "p5x7_"), ("validation_L", "p64x64_"), ("validation_RGB", "")]


def _case(name, prefix):
    g = load_golden(name)
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)} if prefix else g


def _result(g, mode):
    """A ValidationResult built from the fixture's integers alone (what the device returns)."""
    from diffsplitting_amd.core.validation import ValidationResult, psnr_from_stats
    n = g["target"].shape[2] * g["target"].shape[3]
    return ValidationResult(mode=mode, input_q=None, target_q=None, pred_q=None, ssd=g["ssd"], tmin=g["tmin"],
                            tmax=g["tmax"], imin=g["imin"], imax=g["imax"],
                            psnr=psnr_from_stats(g["ssd"], g["tmin"], g["tmax"], n), undefined=int(g["undefined"]))


def test_val_report_symbol_declared_bound_exported():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    assert re.search(r"\bint\s+dsx_val_report\s*\(", header)
    assert "dsx_val_report" in _lib.SIGNATURES and getattr(_lib.lib, "dsx_val_report") is not None
    assert _lib.lib.dsx_abi_version() == 2 and "#define DSX_ABI_VERSION 2" in header
    from diffsplitting_amd.core import validation
    assert "#define DSX_VAL_CHUNK %d\n" % validation.VAL_CHUNK in header
    assert "#define DSX_VAL_MAX_CHANNELS %d\n" % validation.VAL_MAX_CHANNELS in header
    assert "dsx_validate.hip" in open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "build.sh")).read()


@pytest.mark.parametrize("name,prefix", CASES)
def test_psnr_from_integer_statistics_against_the_reference(name, prefix):
    """The reference's value is a float32 mean and log10 (about 5e-5 dB from the exact one); 1e-3 dB is a bound."""
    from diffsplitting_amd.core.validation import group_psnr
    g = _case(name, prefix)
    grouped = group_psnr(_result(g, "RGB" if g["input"].shape[1] == 3 else "L"))
    assert sorted(grouped) == list(g["psnr_keys"])
    ours = np.array([grouped[k] for k in sorted(grouped)]).T            # (B, keys)
    err = np.abs(ours - g["psnr"])
    print(f"{name} {prefix}: max |psnr - reference| = {err.max():.3e} dB")
    assert np.isfinite(ours).all() and err.max() <= 1e-3


def test_group_psnr_keys():
    from diffsplitting_amd.core.validation import group_psnr
    assert sorted(group_psnr(_result(_case("validation_L", "p5x7_"), "L"))) == [0, 1]
    rgb = _result(_case("validation_RGB", ""), "RGB")
    grouped = group_psnr(rgb)
    assert sorted(grouped) == [0, 3] and len(grouped[0]) == 2
    assert grouped[3][1] == float(np.mean(rgb.psnr[1, 3:6]))


@pytest.mark.parametrize("prefix", ["p5x7_", "p64x64_"])
def test_visuals_from_numerators_equal_the_reference_arrays(prefix):
    from diffsplitting_amd.core.validation import visuals_from_numerators
    g = _case("validation_L", prefix)
    inp, tar, pred = visuals_from_numerators(g["input_n"], g["target_n"], g["pred_n"], g["tmin"], g["tmax"], g["imin"],
                                             g["imax"])
    for ours, ref in ((inp, g["input_img"]), (tar, g["target_img"]), (pred, g["pred_img"])):
        assert ours.dtype == np.float64 and np.array_equal(ours, ref)
    below = g["pred_q"].astype(np.int64) < g["tmin"][:, :, None, None]
    assert below.any() and (pred[below] == 1.0).all()                   # the uint16 wrap, kept


def test_fixture_exercises_truncation_clamp_and_wrap():
    for name, prefix in CASES:
        g = _case(name, prefix)
        raw = np.rint(g["target"].astype(np.float64) * g["std_target"] + g["mean_target"]).astype(np.int64)
        assert (g["target_q"].astype(np.int64) == raw - 1).any()
        pv = g["prediction"] * g["std_target"] + g["mean_target"]
        assert (pv < 0).any() and (pv > 65535).any()
        assert (g["pred_q"] == 0).any() and (g["pred_q"] == 65535).any()
        assert int(g["undefined"]) == 0


def test_psnr_degenerate_planes():
    from diffsplitting_amd.core.validation import psnr_from_stats
    p = psnr_from_stats(np.array([0, 0, 35]), np.array([3, 7, 7]), np.array([9, 7, 7]), 35)
    assert p[0] == np.inf and np.isnan(p[1]) and p[2] == -np.inf


def test_refuses_cpu_tensors_and_bad_arguments():
    from diffsplitting_amd._lib import DsxError, lib
    from diffsplitting_amd.core.validation import validation_report
    g = _case("validation_L", "p5x7_")
    nd = {k: g[k] for k in ("mean_input", "std_input", "mean_target", "std_target")}
    t = lambda k: torch.from_numpy(g[k])
    with pytest.raises(DsxError, match="no CPU fallback"):
        validation_report(t("input"), t("target"), t("prediction"), nd)
    with pytest.raises(DsxError, match="no CPU fallback"):
        validation_report(g["input"], g["target"], g["prediction"], nd)
    fake, null = C.c_void_p(4096), C.c_void_p(0)
    two = (C.c_double * 2)(1.0, 1.0)
    err = lambda: lib.dsx_last_error().decode()

    def call(inp=fake, B=2, Cin=1, Cn=2, H=8, W=8, mean=two, tq=fake, nums=(null, null, null), part=fake):
        return lib.dsx_val_report(inp, fake, fake, B, Cin, Cn, H, W, 1.0, 1.0, mean, two, fake, tq, fake, *nums, part, fake,
                                  None)

    assert call(inp=null) < 0 and "null" in err()
    assert call(tq=null) < 0 and call(part=null) < 0 and call(mean=None) < 0
    assert call(B=0) < 0 and call(H=0) < 0 and call(Cin=0) < 0
    assert call(Cn=17) < 0 and "at most 16" in err()
    assert call(B=30000, Cn=2, Cin=1) < 0 and "65535" in err()
    assert call(nums=(fake, null, fake)) < 0 and "together" in err()


def test_l_mode_file_is_16_bit_side_by_side(tmp_path):
    from PIL import Image
    from diffsplitting_amd.core.validation import save_visual_l16
    g = _case("validation_L", "p5x7_")
    img = g["pred_img"][1]                                               # (2, 5, 7) float64 in [0, 1]
    path = str(tmp_path / "3_1_pred.png")
    save_visual_l16(img, path)
    with Image.open(path) as im:
        assert im.mode in ("I;16", "I") and im.size == (14, 5)
        px = np.array(im)
    assert px.dtype in (np.uint16, np.int32)
    want = np.rint(65535.0 * img).astype(np.int64)
    assert np.array_equal(px[:, :7], want[0]) and np.array_equal(px[:, 7:], want[1])
    assert px.max() == 65535                                             # a wrapped / clipped pixel is full scale
    one = str(tmp_path / "one.png")
    save_visual_l16(g["input_img"][0], one)                              # a single channel: H x W
    with Image.open(one) as im:
        assert im.size == (7, 5)
        assert np.array_equal(np.array(im), np.rint(65535.0 * g["input_img"][0, 0]).astype(np.int64))
