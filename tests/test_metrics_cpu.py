"""core.metrics on the host: the reference's import path, tensor2img against a numpy restatement of
core/metrics.py:8-34 (make_grid layout and rounding ties included), save_img's layouts and channel order
(core/metrics.py:37-59) through PIL, and the argument checks of the device entry points that need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.metrics_ref import np_tensor2img, tie_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_import_line_works():
    # split.py:7, infer.py, sample.py and eval.py: `import core.metrics as Metrics`
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "diffsplitting_amd", "compat"), ROOT]))
    code = ("import core.metrics as Metrics; import diffsplitting_amd.core.metrics as M; assert Metrics is M; "
            "[getattr(Metrics, n) for n in ('tensor2img', 'save_img', 'calculate_psnr', 'calculate_ssim')]")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("shape", [(13, 17), (3, 13, 17), (1, 13, 17), (4, 3, 13, 17), (5, 3, 13, 17),
                                   (9, 2, 13, 17), (6, 1, 13, 17), (1, 1, 3, 13, 17)])
@pytest.mark.parametrize("min_max", [(-1, 1), (0, 1), (-0.3, 2.7)])
def test_tensor2img_matches_restatement(shape, min_max):
    from diffsplitting_amd.core.metrics import tensor2img
    g = torch.Generator().manual_seed(len(shape) * 31 + shape[0])
    x = torch.randn(shape, generator=g) * 1.5 + 0.3          # a good share outside min_max
    got = tensor2img(x, min_max=min_max)
    want = np_tensor2img(x.numpy(), min_max)
    assert got.dtype == np.uint8 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_tensor2img_grid_layout():
    from diffsplitting_amd.core.metrics import tensor2img
    x = torch.ones((5, 3, 4, 6))                             # nrow = int(sqrt(5)) = 2: a 2 x 3 grid, one slot empty
    img = tensor2img(x, min_max=(0, 1))
    assert img.shape == (3 * (4 + 2) + 2, 2 * (6 + 2) + 2, 3)
    assert img[2:6, 2:8].min() == 255 and img[14:18, 10:16].max() == 0     # 5th image placed, 6th slot padding
    assert img[:2].max() == 0 and img[:, :2].max() == 0


@pytest.mark.parametrize("min_max", [(-1, 1), (0, 1), (0, 255)])
def test_tensor2img_rounds_ties_to_even(min_max):
    from diffsplitting_amd.core.metrics import tensor2img
    t = tie_values(min_max)
    assert len(t) >= 150
    t = np.resize(t, (len(t) // 10, 10))
    got = tensor2img(torch.from_numpy(t), min_max=min_max)
    np.testing.assert_array_equal(got, np_tensor2img(t, min_max))
    assert (got % 2 == 0).all()


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def test_save_img_rgb_is_written_as_cv2_would(tmp_path):
    from diffsplitting_amd.core.metrics import save_img
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (3, 9, 11), dtype=np.uint8)
    save_img(img, str(tmp_path / "a.png"))
    # cv2.imwrite takes an H x W x 3 array as B, G, R
    np.testing.assert_array_equal(_read(tmp_path / "a.png"), img.transpose(1, 2, 0)[:, :, ::-1])


def test_save_img_six_channel_pair_side_by_side(tmp_path):
    from diffsplitting_amd.core.metrics import save_img
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (6, 8, 5), dtype=np.uint8)      # CIFAR: two RGB images
    save_img(img, str(tmp_path / "b.png"))
    want = np.concatenate([img[0:3].transpose(1, 2, 0), img[3:6].transpose(1, 2, 0)], axis=1)[:, :, ::-1]
    np.testing.assert_array_equal(_read(tmp_path / "b.png"), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_save_img_two_channel_gray_side_by_side(tmp_path, dtype):
    from diffsplitting_amd.core.metrics import save_img
    rng = np.random.default_rng(2)
    img = rng.integers(0, np.iinfo(dtype).max, (2, 7, 10)).astype(dtype)  # Hagen: two channels
    save_img(img, str(tmp_path / "c.png"), mode="L")
    got = _read(tmp_path / "c.png")
    np.testing.assert_array_equal(got.astype(np.int64), np.concatenate([img[0], img[1]], axis=1).astype(np.int64))


def test_save_img_single_channel(tmp_path):
    from diffsplitting_amd.core.metrics import save_img
    img = np.arange(35, dtype=np.uint8).reshape(1, 5, 7)
    save_img(img, str(tmp_path / "d.png"))
    np.testing.assert_array_equal(_read(tmp_path / "d.png"), img[0])


def test_calculate_psnr_restates_reference():
    from diffsplitting_amd.core.metrics import calculate_psnr
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    import math
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    assert calculate_psnr(a, b) == 20 * math.log10(255.0 / math.sqrt(mse))
    assert calculate_psnr(a, a) == float("inf")


def test_metrics_argument_checks_without_device():
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core.metrics import calculate_ssim, image_metrics
    assert _lib.lib.dsx_image_metrics_blocks(11, 11) == 1
    assert _lib.lib.dsx_image_metrics_blocks(2048, 2048) == 64 * 64
    assert _lib.lib.dsx_image_metrics_blocks(10, 64) < 0
    assert b"11" in _lib.lib.dsx_last_error()
    with pytest.raises(ValueError):
        calculate_ssim(np.zeros((16, 16), np.uint8), np.zeros((16, 17), np.uint8))
    with pytest.raises(_lib.DsxError):
        image_metrics(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))


def test_calculate_ssim_has_no_cpu_fallback():
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core.metrics import calculate_ssim
    if _lib.lib.dsx_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.DsxError):
        calculate_ssim(np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8))


def test_range_invariant_psnr_from_sums_is_the_metric():
    """The closed form on float64 sums of 20 fp32 plane pairs against the metric itself restated in longdouble
    (core/psnr.py:28-39).  On these inputs the two differ by a few 1e-14 dB: float64 rounding of sums of 1517 terms."""
    from diffsplitting_amd.core.psnr import range_invariant_psnr_from_sums
    from tests.metrics_ref import range_invariant_psnr
    gen = torch.Generator().manual_seed(2024)
    g = torch.randn((20, 37, 41, 1), generator=gen) * 1.5 + 0.25
    p = 0.7 * g + 0.5 * torch.randn((20, 37, 41, 1), generator=gen) + 3.0
    g64, p64 = g.double().reshape(20, -1), p.double().reshape(20, -1)
    got = range_invariant_psnr_from_sums(p64.sum(1), (p64 * p64).sum(1), g64.sum(1), (g64 * g64).sum(1), (g64 * p64).sum(1),
                                         g64.amin(1), g64.amax(1), float(37 * 41))
    want = range_invariant_psnr(g.numpy(), p.numpy(), np.longdouble)[:, 0]
    err = np.abs(got.numpy().astype(np.longdouble) - want).max()
    print(f"\nlargest |closed form - longdouble metric| = {float(err):.3e} dB over PSNRs {float(want.min()):.2f} .. "
          f"{float(want.max()):.2f} dB")
    assert got.dtype == torch.float64 and err < 1e-10
