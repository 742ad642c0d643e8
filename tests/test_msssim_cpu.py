"""MS-SSIM without a GPU: the float64 restatement (tests/msssim_ref.py) against hand-checkable cases and against the
mistakes it must tell apart, every host-side refusal of core.metrics.msssim / calculate_msssim by name, the C entry
points' shape rule, and the `split --ms-ssim` refusals."""
import json

import numpy as np
import pytest
import torch

from tests import metrics_ref, msssim_ref as ref


@pytest.fixture(scope="module")
def pair():
    return ref.structured_pair((183, 203), 3)


def test_identical_planes_give_exactly_one(pair):
    t, _ = pair
    value, means = ref.msssim(t, t.copy(), data_range=3.7)
    assert value == 1.0 and (means == 1.0).all()
    value, means = ref.msssim(t, t.copy(), range_invariant=True, weights=(0.2, 0.3, 0.5))
    assert abs(value - 1.0) <= 1e-12                                     # alpha p~ is g' up to rounding only


def test_negated_prediction_is_clamped_to_exactly_zero(pair):
    t, _ = pair
    value, means = ref.msssim(-t, t, data_range=3.7)
    assert means[0, 0] < 0 and value == 0.0


def test_one_scale_is_the_single_scale_ssim(pair):
    t, p = pair
    value, means = ref.msssim(p, t, data_range=3.7, weights=(1.0,))
    want = metrics_ref.ssim_map(p, t, 3.7).mean()
    assert abs(value - want) <= 1e-14 and means.shape == (1, 2)


def test_pooling_rule_on_an_odd_sized_array():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 9))
    want = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            want[i, j] = ((x[2 * i, 2 * j] + x[2 * i, 2 * j + 1]) + (x[2 * i + 1, 2 * j] + x[2 * i + 1, 2 * j + 1])) * 0.25
    got = ref.pool2(x)
    assert got.shape == (3, 4) and (got == want).all()
    assert ref.pool2_keep_odd(x).shape == (4, 5)


def test_structured_images_separate_the_scales(pair):
    """What the GPU tests' tolerance derivation rests on: cs rises with the scale and never falls below 0.68."""
    t, p = pair
    value, means = ref.msssim(p, t, data_range=3.7)
    assert (np.diff(means[:, 0]) > 0).all() and means[0, 0] < 0.75 and means[4, 0] > 0.99
    assert (means[:, 0] >= 0.68).all() and 0.9 < value < 0.99


@pytest.mark.parametrize("mistake", [dict(pool=ref.pool2_keep_odd), dict(fine="ssim"), dict(c2_per_scale=True)])
def test_the_restatement_tells_typical_mistakes_apart(pair, mistake):
    t, p = pair
    good, _ = ref.msssim(p, t, data_range=3.7)
    bad, _ = ref.msssim(p, t, data_range=3.7, **mistake)
    assert abs(good - bad) > 1e-6, (good, bad)


def test_range_invariant_form_is_affine_invariant(pair):
    t, p = pair
    a, _ = ref.msssim(p, t, range_invariant=True)
    b, _ = ref.msssim(3.1 * p.astype(np.float64) + 7, 5 * t.astype(np.float64) - 2, range_invariant=True)
    assert abs(a - b) <= 1e-12
    p2, g2, L = ref.range_invariant_transform(p, t)
    from diffsplitting_amd.core.psnr import RangeInvariantPsnr
    want = RangeInvariantPsnr(torch.from_numpy(t)[None].double(), torch.from_numpy(p)[None].double()).item()
    got = 20 * np.log10(L / np.sqrt(np.mean((g2 - p2) ** 2)))
    assert abs(got - want) <= 1e-3                                       # RangeInvariantPsnr itself computes in fp32
    value, _ = ref.msssim(p, np.full_like(t, 2.5), range_invariant=True)
    assert np.isnan(value)


# ----------------------------------------------------------------------------- core.metrics, host side
def test_host_side_refusals_by_name():
    from diffsplitting_amd.core import metrics as M
    z = lambda *s: torch.zeros(s)
    with pytest.raises(ValueError, match=r"one shape.*\(1, 1, 176, 176\).*\(1, 1, 176, 177\)"):
        M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 177), data_range=1.0)
    with pytest.raises(ValueError, match="one shape"):
        M.msssim(z(1, 176, 176), z(1, 176, 176), data_range=1.0)
    with pytest.raises(ValueError, match=r"5 scales needs min\(H, W\) >= 176.*got 175 x 300"):
        M.msssim(z(1, 1, 175, 300), z(1, 1, 175, 300), data_range=1.0)
    with pytest.raises(ValueError, match=r"3 scales needs min\(H, W\) >= 44.*got 60 x 43"):
        M.msssim(z(1, 1, 60, 43), z(1, 1, 60, 43), data_range=1.0, weights=(0.2, 0.3, 0.5))
    for bad, match in (((), "1 to 5 of them, got 0"), ((0.1,) * 6, "1 to 5 of them, got 6"),
                       ((0.5, 0.0), "weights must be positive"), ((0.5, -0.5), "weights must be positive"),
                       ((float("nan"),), "weights must be positive")):
        with pytest.raises(ValueError, match=match):
            M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 176), data_range=1.0, weights=bad)
    with pytest.raises(ValueError, match="data_range and range_invariant both"):
        M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 176), data_range=1.0, range_invariant=True)
    with pytest.raises(ValueError, match="give data_range .* or range_invariant=True"):
        M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 176))
    with pytest.raises(ValueError, match="data_range must be positive"):
        M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 176), data_range=0.0)
    with pytest.raises(M.DsxError):                                       # CPU tensors: no CPU fallback
        M.msssim(z(1, 1, 176, 176), z(1, 1, 176, 176), data_range=1.0)
    with pytest.raises(ValueError, match=r"\(N, H, W, C\) of one shape"):
        M.calculate_msssim(np.zeros((1, 176, 176, 2), np.float32), np.zeros((1, 176, 176, 1), np.float32))
    with pytest.raises(ValueError, match=r"needs min\(H, W\) >= 176.*got 128 x 512"):
        M.calculate_msssim(np.zeros((1, 128, 512, 2), np.float32), np.zeros((1, 128, 512, 2), np.float32))
    assert M.MSSSIM_WEIGHTS == ref.WEIGHTS and M.msssim_min_side(5) == 176 and M.msssim_min_side(1) == 11


def test_host_product_from_means():
    from diffsplitting_amd.core import metrics as M
    rng = np.random.default_rng(1)
    means = rng.uniform(0.3, 1.0, (2, 3, 5, 2))
    means[0, 1, 2, 0] = -0.1                                              # a negative cs is clamped: the plane is 0
    means[1, 2, 4, 1] = np.nan
    got = M.msssim_from_means(means, M.MSSSIM_WEIGHTS)
    for b in range(2):
        for c in range(3):
            want = ref.from_means(means[b, c])
            assert got[b, c] == want or (np.isnan(got[b, c]) and np.isnan(want))
    assert got[0, 1] == 0.0 and np.isnan(got[1, 2])
    assert M.msssim_from_means(means[..., :3, :], (0.2, 0.3, 0.5))[0, 0] == ref.from_means(means[0, 0, :3], (0.2, 0.3, 0.5))


def test_library_shape_rule():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    assert lib.dsx_msssim_workspace(176, 176, 5) > 0 and lib.dsx_msssim_workspace(11, 11, 1) > 0
    assert lib.dsx_msssim_workspace(175, 400, 5) < 0
    msg = lib.dsx_last_error().decode()
    assert "5 scales" in msg and "176" in msg and "175 x 400" in msg
    assert lib.dsx_msssim_workspace(176, 176, 6) < 0 and lib.dsx_msssim_workspace(176, 176, 0) < 0
    # the pooled pyramids dominate: two double planes per scale >= 1
    pyr = sum(2 * 8 * (2048 >> s) ** 2 for s in range(1, 5))
    assert pyr < lib.dsx_msssim_workspace(2048, 2048, 5) < pyr * 1.02


# ----------------------------------------------------------------------------- split --ms-ssim
def _config(tmp_path, which, name="Hagen"):
    cfg = {"name": "tiny", "phase": "val", "gpu_ids": [0], "path": {"resume_state": None},
           "datasets": {"patch_size": 32, "max_qval": 0.98, "train": {"name": name, "batch_size": 3, "datapath": "none"},
                        "val": {"name": name, "datapath": "none"}},
           "model": {"which_model_G": which, "loss_type": "l2"}}
    p = tmp_path / f"{which}_{name}.json"
    p.write_text(json.dumps(cfg))
    return str(p)


def test_split_refuses_ms_ssim_where_it_does_not_apply(tmp_path, monkeypatch):
    """SystemExit by name, on the command line and the config alone: no rank is started, the device is not touched."""
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    indi = _config(tmp_path, "indi")
    with pytest.raises(SystemExit, match="--ms-ssim with --input.*no ground truth"):
        split.main(["-c", indi, "--ms-ssim", "--input", "stack.tif", "--norm", "n.json"])
    with pytest.raises(SystemExit, match="--ms-ssim.*not with --validate"):
        split.main(["-c", indi, "--ms-ssim", "--validate"])
    with pytest.raises(SystemExit, match="--ms-ssim.*colour items"):
        split.main(["-c", _config(tmp_path, "indi", "cifar10"), "--ms-ssim", "--datapath"])
    with pytest.raises(SystemExit, match=r"--ms-ssim: MS-SSIM with 5 scales needs min\(H, W\) >= 176.*got 128 x 512"):
        split.main(["-c", indi, "--ms-ssim", "--synthetic", "1,128,512"])
    # where it applies the checks pass: the run gets as far as starting (the stand-in above)
    for argv in (["--ms-ssim"], ["--ms-ssim", "--synthetic", "1,176,176"], ["--ms-ssim", "--frames", "f.npy"]):
        with pytest.raises(AssertionError, match="a rank was started"):
            split.main(["-c", indi] + argv)
