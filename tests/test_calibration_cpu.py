"""The spread calibration without a GPU: the entry points exist in the header, the binding and the library; every
refusal of dsx_calibration and of ``split --calibration`` / ``--apply-calibration`` by message; the JSON round trip; the
fit against numpy's least squares; ``apply``; and the sensitivity of tests/calibration_ref.py: its bound accepts the
kernel's order of additions and rejects the typical mistakes."""
import json
import os
import re

import numpy as np
import pytest
import torch

from diffsplitting_amd import _lib
from diffsplitting_amd._lib import DsxError, check, lib
from diffsplitting_amd.core import calibration as CAL
from tests import calibration_ref as REF
from tests.bits import same_bits
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsx_calibration_blocks", "dsx_calibration")


def test_the_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/dsx.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert hasattr(_lib._cdll, name), f"{name} is not exported by libdsx.so"
        assert callable(getattr(lib, name))
    srcs = open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "build.sh")).read()
    assert "dsx_calib.hip" in srcs and "dsx_calib.cpp" in srcs


def _span():
    """pixels up to which the canvases are one workgroup, read from dsx_calibration_blocks (no device needed)"""
    lo, hi = 1, 1 << 24
    assert lib.dsx_calibration_blocks(lo) == 1 and lib.dsx_calibration_blocks(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.dsx_calibration_blocks(mid) == 1 else (lo, mid)
    assert lib.dsx_calibration_blocks(2 * lo) == 2 and lib.dsx_calibration_blocks(2 * lo + 1) == 3
    return lo


def test_blocks_are_a_function_of_n_alone():
    s = _span()
    assert s % 4 == 0 and lib.dsx_calibration_blocks(1 << 40) >= lib.dsx_calibration_blocks(1 << 30) > 3
    for bad in (0, -1, (1 << 40) + 1):
        with pytest.raises(DsxError, match=r"calibration: n = .* must be in 1\.\.2\^40"):
            check(lib.dsx_calibration_blocks(bad))


def test_every_refusal_comes_before_any_device_work():
    """Addresses that are never dereferenced stand in for device memory: a call that got past its checks would launch."""
    P = 4096                                                     # a non-NULL "device" address
    edges, z = np.array([[0.1, 0.2, 0.2]]), np.array([1.0, 2.0])

    def refused(match, mean=P, std=P, target=P, n=100, Cn=1, e=edges, nbins=4, zz=z, nz=2, part=P, out=P):
        with pytest.raises(DsxError, match=match):
            check(lib.dsx_calibration(mean, std, target, n, Cn, e, nbins, zz, nz, part, out, None))

    for slot in ("mean", "std", "target", "part", "out"):
        refused("calibration: null argument", **{slot: None})
    refused("calibration: null argument", e=None)
    refused("calibration: null argument", zz=None)
    refused(r"n = 0 pixels, must be in 1\.\.2\^40", n=0)
    refused(r"n = 1099511627777 pixels, must be in 1\.\.2\^40", n=(1 << 40) + 1)
    refused(r"C = 0 channels, must be in 1\.\.4", Cn=0)
    refused(r"C = 5 channels, must be in 1\.\.4", Cn=5)
    refused(r"nbins = 0, must be in 1\.\.64", nbins=0)
    refused(r"nbins = 65, must be in 1\.\.64", nbins=65)
    refused(r"nz = -1, must be in 0\.\.8", nz=-1)
    refused(r"nz = 9, must be in 0\.\.8", nz=9)
    refused("edge 1 of channel 0 is not finite", e=np.array([[0.1, np.inf, 0.3]]))
    refused("edge 0 of channel 0 is not finite", e=np.array([[np.nan, 0.2, 0.3]]))
    refused("edges of channel 1 descend at 2", e=np.array([[0.1, 0.2, 0.3], [0.1, 0.3, 0.2]]), Cn=2)
    refused(r"z\[1\] = -1, must be finite and not negative", zz=np.array([1.0, -1.0]))
    refused(r"z\[0\] = (nan|-nan), must be finite", zz=np.array([np.nan, 1.0]))
    refused(r"z\[1\] = inf, must be finite", zz=np.array([1.0, np.inf]))


def test_python_refuses_what_is_no_cuda_fp32_canvas():
    x = torch.zeros(4, 4, 2)
    with pytest.raises(DsxError, match="std must be a CUDA float32 tensor"):
        CAL.calibration_stats(x, x, x)
    with pytest.raises(DsxError, match="std must be a CUDA float32 tensor"):
        CAL.bin_edges(x.double(), 4)
    with pytest.raises(DsxError, match="std must be a CUDA float32 tensor"):
        CAL.bin_edges(np.zeros((4, 2), np.float32), 4)


def _cal(C=2, bins=5, samples=3, seed=0):
    rng = np.random.default_rng(seed)
    sums = np.zeros((C, 3 * bins + 3))
    cnt = rng.integers(1, 1000, (C, bins)).astype(np.float64)
    cnt[0, 1] = 0                                                  # an empty bin: NaN rmv / rmse
    sums[:, 0:3 * bins:3] = cnt
    sums[:, 1:3 * bins:3] = cnt * rng.random((C, bins)) * 3
    sums[:, 2:3 * bins:3] = cnt * rng.random((C, bins)) * 3
    n = int(cnt.sum(axis=1).max())
    sums[:, 3 * bins:] = rng.integers(0, n, (C, 3))
    edges = np.sort(rng.random((C, bins - 1)) * np.pi, axis=1)
    stats = CAL.stats_from_sums(sums, edges, (1, 2, 3), n)
    return CAL.Calibration.from_stats(stats, samples, std_target=rng.random(C) * 1e3 + 1 / 3)


def test_json_round_trip_is_exact(tmp_path):
    cal = _cal()
    assert np.isnan(cal.stats.rmv[0, 1]) and np.isnan(cal.stats.rmse[0, 1])
    path = str(tmp_path / "cal.json")
    cal.save(path)
    json.load(open(path))                                          # strict JSON (no NaN literal)
    back = CAL.Calibration.load(path)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    for k in ("a", "c", "scale", "std_target"):
        assert same_bits(f64(getattr(back, k)), f64(getattr(cal, k))), k
    for k in ("edges", "z", "sv", "se", "rmv", "rmse", "coverage"):
        assert same_bits(f64(getattr(back.stats, k)), f64(getattr(cal.stats, k))), k
    for k in ("count", "covered"):
        assert np.array_equal(getattr(back.stats, k), getattr(cal.stats, k)) and getattr(back.stats, k).dtype == np.int64
    assert (back.samples, back.channels, back.stats.n) == (3, 2, cal.stats.n)
    # what is no calibration file is refused by name
    (tmp_path / "text.json").write_text("not json")
    with pytest.raises(DsxError, match="not a calibration file"):
        CAL.Calibration.load(str(tmp_path / "text.json"))
    doc = json.load(open(path))
    for change, match in ((dict(format="other"), "format 'other'"), (dict(version=2), "version 2"),
                          (dict(samples=1), "samples = 1"), (dict(curve={}), "not a complete calibration file")):
        (tmp_path / "bad.json").write_text(json.dumps(dict(doc, **change)))
        with pytest.raises(DsxError, match=match):
            CAL.Calibration.load(str(tmp_path / "bad.json"))


def test_fit_is_the_weighted_least_squares_line():
    cal = _cal(C=3, bins=12, seed=4)
    s = cal.stats
    for ch in range(3):
        ok = s.count[ch] > 0
        w = np.sqrt(s.count[ch][ok].astype(np.float64))
        A = np.stack([s.rmv[ch][ok], np.ones(ok.sum())], axis=1) * w[:, None]
        (a, c), *_ = np.linalg.lstsq(A, s.rmse[ch][ok] * w, rcond=None)
        assert abs(cal.a[ch] - a) <= 1e-12 * abs(a) and abs(cal.c[ch] - c) <= 1e-12 * max(abs(c), abs(a))
        assert abs(cal.scale[ch] / np.sqrt(s.se[ch].sum() / s.sv[ch].sum()) - 1) <= 1e-12
    # degenerate: one non-empty bin; rmv values that do not differ
    one = CAL.stats_from_sums(np.array([[0, 0, 0, 10, 2.5, 10.0, 0, 0, 0]], dtype=np.float64), np.zeros((1, 2)), (), 10)
    line = CAL.fit(one)
    assert line["a"][0] == line["scale"][0] == 2.0 and line["c"][0] == 0.0
    same = CAL.stats_from_sums(np.array([[10, 2.5, 10.0, 20, 5.0, 5.0, 0, 0, 0]], dtype=np.float64), np.zeros((1, 2)), (), 30)
    assert same.rmv[0, 0] == same.rmv[0, 1] and np.isnan(same.rmv[0, 2])
    line = CAL.fit(same)
    assert line["a"][0] == line["scale"][0] == np.sqrt(15.0 / 7.5) and line["c"][0] == 0.0


def test_apply_is_the_line_clamped_at_zero():
    cal = _cal()
    cal.a[:], cal.c[:] = (2.0, 0.5), (-1.0, 0.25)
    std = torch.tensor([[[0.0, 0.0], [0.25, 0.25], [1.5, 1.5], [0.5, -1.0]]])
    got = cal.apply(std)
    assert got.dtype == torch.float32 and got.shape == std.shape
    assert got.tolist() == [[[0.0, 0.25], [0.0, 0.375], [2.0, 1.0], [0.0, 0.0]]]
    expect = (std.double() * torch.tensor(cal.a) + torch.tensor(cal.c)).clamp_min(0).float()
    assert torch.equal(got, expect)
    with pytest.raises(DsxError, match="the spread has 3 channels, the calibration 2"):
        cal.apply(torch.zeros(4, 3))


def test_quantile_ranks_restate_np_quantile():
    """bin_edges on the host side: the order statistics it asks for and its interpolation give np.quantile's bits."""
    rng = np.random.default_rng(1)
    for n, bins in ((1, 4), (2, 3), (7, 7), (4099, 32), (1000, 64), (129, 2)):
        x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        x[rng.random(n) < 0.3] = 0.5                               # ties
        ranks, lo, hi, frac = CAL.quantile_ranks(n, bins)
        assert ranks.size <= 2 * (bins - 1) and (np.diff(ranks) > 0).all() and 0 <= ranks.min() and ranks.max() < n
        got = CAL.edges_from_order_stats(np.sort(x)[ranks], lo, hi, frac)
        ref = np.quantile(x, np.arange(1, bins) / bins)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (n, bins)


# ----------------------------------------------------------------------------- the reference and its bound
def test_plain_numpy_bins_are_equal_count_and_all_equal_std_fills_the_last_bin():
    m, s, t = REF.cases(4099, 1, seed=2)["random"]
    ref = REF.stats(m, s, t, REF.edges_of(s, 32), ())
    assert set(ref[0, 0::3].astype(int)) <= {128, 129} and ref[0, 0::3].sum() == 4099
    m, s, t = REF.cases(257, 2, seed=2)["equal"]
    ref = REF.stats(m, s, t, REF.edges_of(s, 7), (1.0,))
    assert (ref[:, 0:18:3] == 0).all() and (ref[:, 18] == 257).all()


@pytest.mark.parametrize("n_of", ["257", "2 span + 1"])
def test_the_bound_accepts_the_kernels_order_and_rejects_the_typical_mistakes(n_of):
    span = _span()
    n = 257 if n_of == "257" else 2 * span + 1
    C, nbins, z = 2, 7, REF.Z_OF[8]
    m, s, t = REF.cases(n, C, seed=5)["ties"]
    edges = REF.edges_of(s, nbins)
    assert np.isin(edges, s.astype(np.float64)).any()             # values sit exactly on an edge
    ref, bnd = REF.stats(m, s, t, edges, z, with_bounds=True)
    emu = REF.emulate(m, s, t, edges, z, span)
    assert REF.agrees(emu, ref, bnd, nbins, len(z))
    err = np.abs(emu - ref)
    print(f"n = {n}: the kernel's order against the exact sums: max err / bound "
          f"{np.nanmax(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0)):.3f}")
    ints = REF.is_integer_slot(nbins, len(z))
    for which in ("left", "strict", "e32", "acc32", "nosquare"):
        bad = REF.mistaken(m, s, t, edges, z, which)
        assert not REF.agrees(bad, ref, bnd, nbins, len(z)), which
        if which == "left":
            assert not np.array_equal(bad[:, :3 * nbins:3], ref[:, :3 * nbins:3])          # the counts move
        if which == "strict":
            assert (bad[:, 3 * nbins:] <= ref[:, 3 * nbins:]).all() and (bad[:, 3 * nbins:] != ref[:, 3 * nbins:]).any()
        if which in ("e32", "acc32", "nosquare"):
            assert np.array_equal(bad[:, ints], ref[:, ints])                            # only the sums leave the bound
    # on the boundary case '<' loses exactly the pixels with |e| = z std
    m, s, t = REF.cases(n, C, seed=5)["boundary"]
    edges = REF.edges_of(s, 2)
    ref, strict = REF.stats(m, s, t, edges, (1.0, 2.0)), REF.mistaken(m, s, t, edges, (1.0, 2.0), "strict")
    e = np.abs(t.astype(np.float64) - m.astype(np.float64))
    assert np.array_equal(ref[:, 6] - strict[:, 6], (e == 0.5).sum(axis=0))
    assert np.array_equal(ref[:, 7] - strict[:, 7], (e == 1.0).sum(axis=0)) and (e == 1.0).any()


# ----------------------------------------------------------------------------- command line
def test_split_refuses_the_calibration_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    """Every refusal is a SystemExit that names the flag, raised on the command line, the config and the calibration file
    alone: no rank is started and nothing touches the device."""
    from diffsplitting_amd import parallel, split
    from diffsplitting_amd.data.normalization import save_normalization

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    indi, joint = write_config(tmp_path, "indi"), write_config(tmp_path, "joint_indi")
    one = write_config(tmp_path, "indi", target_channel_idx=1)
    norm = str(tmp_path / "n.json")
    nd = {"mean_input": 1.0, "std_input": 2.0, "target0_max": 3.0, "target1_max": 4.0, "input_max": 5.0,
          "mean_target": [1.0, 2.0], "std_target": [3.0, 4.0]}
    save_normalization(norm, nd, data_type="Hagen", channel_weights=None, max_qval=0.98, upper_clip=False, target_channel_idx=None)
    stack = str(tmp_path / "s.npy")
    np.save(stack, np.zeros((1, 32, 32), np.uint16))
    cal2 = str(tmp_path / "cal2.json")
    _cal(C=2, samples=3).save(cal2)
    out, std_out = str(tmp_path / "cal.json"), str(tmp_path / "std.npy")

    def refused(argv, match, config=indi):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", config] + argv)

    refused(["--calibration", out, "--samples", "3", "--input", stack, "--norm", norm], "--calibration with --input.*no ground truth")
    refused(["--calibration", out, "--samples", "3", "--validate"], "--calibration .*not with --validate")
    refused(["--calibration", out, "--samples", "3", "--mix-t", "0.3"], "--calibration: not with --mix-t", config=joint)
    refused(["--calibration", out], "--calibration: the spread needs --samples 2 or more")
    refused(["--calibration", out, "--samples", "1"], "--calibration: the spread needs --samples 2 or more")
    refused(["--calibration", out, "--samples", "3", "--calibration-bins", "65"], "--calibration-bins 65")
    refused(["--calibration", out, "--samples", "3", "--calibration-bins", "1"], "--calibration-bins 1")
    refused(["--calibration-bins", "8"], "--calibration-bins: only with --calibration")
    refused(["--apply-calibration", cal2, "--samples", "3"], "--apply-calibration .*--std-out")
    refused(["--apply-calibration", str(tmp_path / "none.json"), "--samples", "3", "--std-out", std_out],
            "--apply-calibration .*none.json")
    refused(["--apply-calibration", norm, "--samples", "3", "--std-out", std_out], "--apply-calibration .*format")
    refused(["--apply-calibration", cal2, "--samples", "3", "--std-out", std_out],
            "--apply-calibration .*a calibration of 2 channels, the prediction has 1", config=one)
    refused(["--apply-calibration", cal2, "--samples", "4", "--std-out", std_out],
            "--apply-calibration .*fitted at --samples 3, this run draws 4")
    assert not os.path.exists(out) and not os.path.exists(std_out)
