"""core.metrics on the MI355X (dsx_image_metrics): the fused tensor2img quantisation bit-equal to the host path, PSNR
bit-equal to calculate_psnr, SSIM within 1e-9 of the float64 scipy restatement of core/metrics.py:72-92
(tests/metrics_ref.py), bitwise-reproducible results, and the H, W >= 11 check."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _m():
    from diffsplitting_amd.core import metrics
    return metrics


def _images(shape, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g) * scale
    b = a + torch.randn(shape, generator=g) * 0.25           # correlated: SSIM well away from 0
    return a, b


@pytest.mark.parametrize("min_max", [(-1, 1), (0, 1), (-0.3, 2.7)])
def test_device_quantisation_bit_equal(min_max):
    M = _m()
    B, H, W = 8, 24, 24
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((B, 1, H, W), generator=g) * 1.5 + 0.3).numpy()    # many values outside min_max
    ties = ref.tie_values(min_max)
    flat = x.reshape(-1)
    flat[::3][:len(ties)] = ties[:len(flat[::3])]                         # values on .5 ties
    x = torch.from_numpy(x)
    q = np.stack([ref.np_tensor2img(x[i].numpy(), min_max) for i in range(B)]).astype(np.int64)
    for i in range(B):                                                   # the restatement is tensor2img itself
        np.testing.assert_array_equal(M.tensor2img(x[i], min_max=min_max), q[i])
    xd = x.to(DEV)
    lo = torch.full_like(xd, min_max[0] - 1.0)                          # quantises to 0
    hi = torch.full_like(xd, min_max[1] + 1.0)                          # quantises to 255
    _, s0 = M._run(xd, lo, True, min_max[0], min_max[1], 255.0)
    _, s1 = M._run(xd, hi, True, min_max[0], min_max[1], 255.0)
    # sum q^2 and sum (255 - q)^2 exact per image: any pixel off by one changes them
    np.testing.assert_array_equal(s0, (q ** 2).reshape(B, -1).sum(1).astype(np.float64))
    np.testing.assert_array_equal(s1, ((255 - q) ** 2).reshape(B, -1).sum(1).astype(np.float64))


def test_sr3_batch_psnr_bit_equal_and_ssim():
    M = _m()
    a, b = _images((16, 3, 128, 128), 11)
    psnr, ssim = M.image_metrics(a.to(DEV), b.to(DEV))
    assert psnr.dtype == torch.float64 and ssim.dtype == torch.float64 and psnr.shape == (16,)
    for i in range(16):
        ia, ib = M.tensor2img(a[i]), M.tensor2img(b[i])
        assert psnr[i].item() == ref.psnr(ia, ib) == M.calculate_psnr(ia, ib)
        assert abs(ssim[i].item() - ref.ssim(ia, ib)) <= 1e-9
        assert 0.2 < ssim[i].item() < 0.99


@pytest.mark.parametrize("shape", [(11, 11), (128, 128, 3), (512, 512, 1)])
def test_calculate_ssim_numpy_inputs(shape):
    M = _m()
    rng = np.random.default_rng(len(shape) + shape[0])
    a = rng.integers(0, 256, shape).astype(np.float64)
    a = np.clip(a * 0.5 + 64, 0, 255)
    b = np.clip(a + rng.normal(0, 20, shape), 0, 255)
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    got = M.calculate_ssim(a, b)
    want = ref.ssim(np.squeeze(a, 2) if a.ndim == 3 and a.shape[2] == 1 else a,
                    np.squeeze(b, 2) if b.ndim == 3 and b.shape[2] == 1 else b)
    assert abs(got - want) <= 1e-9, (got, want)


def test_float_frame_2048_data_range():
    M = _m()
    a, b = _images((1, 1, 2048, 2048), 23, scale=1.1)
    L = 3.7
    psnr, ssim = M.image_metrics(a.to(DEV), b.to(DEV), quantize=False, data_range=L)
    want = ref.ssim_map(a[0, 0].numpy(), b[0, 0].numpy(), L).mean()
    assert abs(ssim[0].item() - want) <= 1e-9, (ssim[0].item(), want)
    assert psnr[0].item() == pytest.approx(ref.psnr(a[0, 0].numpy(), b[0, 0].numpy(), L), rel=1e-12)


# (H, W) -> valid region (H - 10, W - 10): one-row and one-column tile grids (1 x 65, 65 x 1), an exact 32-pixel tile next
# to a one-pixel tile in both orientations (32 x 33, 33 x 32), 30 x 23, and 2 x 5 tiles (64 x 129)
UNEVEN = [(11, 75), (75, 11), (42, 43), (43, 42), (40, 33), (74, 139)]


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("hw", UNEVEN, ids=lambda s: f"{s[0]}x{s[1]}")
def test_uneven_tile_grids_against_the_restatement(hw, quantize):
    """k_image_metrics takes its tile from tiles_x and the SSD's owner from ty_last / tx_last: non-square grids against
    the float64 restatement, three planes each, at the tolerances of the square sizes above"""
    M = _m()
    H, W = hw
    a, b = _images((2, 3, H, W), 100 * H + W)
    if quantize:
        psnr, ssim = M.image_metrics(a.to(DEV), b.to(DEV))
    else:
        L = 3.7
        psnr, ssim = M.image_metrics(a.to(DEV), b.to(DEV), quantize=False, data_range=L)
    assert psnr.shape == (2,) and ssim.shape == (2,)
    for i in range(2):
        if quantize:
            ia, ib = M.tensor2img(a[i]), M.tensor2img(b[i])
            assert ia.shape == (H, W, 3)
            assert psnr[i].item() == ref.psnr(ia, ib) == M.calculate_psnr(ia, ib)
            want = ref.ssim(ia, ib)
        else:
            ia, ib = a[i].numpy(), b[i].numpy()
            assert psnr[i].item() == pytest.approx(ref.psnr(ia, ib, L), rel=1e-12)
            want = np.mean([ref.ssim_map(ia[c], ib[c], L) for c in range(3)])
        assert abs(ssim[i].item() - want) <= 1e-9, (ssim[i].item(), want)
        assert 0.0 < ssim[i].item() < 0.999                  # neither degenerate nor an identical pair


@pytest.mark.parametrize("quantize", [True, False])
def test_identical_inputs(quantize):
    M = _m()
    a, _ = _images((3, 3, 40, 33), 7)
    ad = a.to(DEV)
    psnr, ssim = M.image_metrics(ad, ad.clone(), quantize=quantize, data_range=255.0 if quantize else 2.0)
    assert (ssim == 1.0).all() and torch.isinf(psnr).all()


def test_bitwise_reproducible():
    M = _m()
    a, b = _images((2, 3, 700, 515), 29)
    ad, bd = a.to(DEV), b.to(DEV)
    for kw in ({}, {"quantize": False, "data_range": 5.0}):
        p0, s0 = M.image_metrics(ad, bd, **kw)
        p1, s1 = M.image_metrics(ad, bd, **kw)
        assert p0.numpy().tobytes() == p1.numpy().tobytes() and s0.numpy().tobytes() == s1.numpy().tobytes()


def test_small_images_rejected():
    from diffsplitting_amd._lib import DsxError
    M = _m()
    with pytest.raises(DsxError, match="11"):
        M.image_metrics(torch.zeros((1, 1, 10, 64), device=DEV), torch.zeros((1, 1, 10, 64), device=DEV))
    with pytest.raises(DsxError, match="11"):
        M.calculate_ssim(np.zeros((64, 10), np.uint8), np.zeros((64, 10), np.uint8))
