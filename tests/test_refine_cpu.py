"""Refining the mixing time from the split itself, the parts that need no GPU: the restatement of tests/comoments_ref.py
against a direct float64 RangeInvariantPsnr scan within its derived bound, that bound's sensitivity, the curve of
core/psnr.py against the restatement, the new entry points' symbols and host-side refusals, the `split` refusals."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import comoments_ref as CR

T_LIST = np.arange(0, 1.0, 0.05)
SHAPES = [(3, 7, 9), (2, 64, 64), (4, 33, 130)]


@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_against_the_direct_scan(shape):
    g, p1, p2 = CR.planted(shape, seed=0)
    m, mb = CR.moments(g, p1, p2, with_bounds=True)
    c, t_star = CR.curve(m, T_LIST, 1 - T_LIST)
    bound = CR.curve_bound(m, mb, T_LIST, 1 - T_LIST)
    direct = CR.direct_curve(g, (p1, p2), [(t, 1 - t) for t in T_LIST])
    diff = np.abs(c - direct)
    print(f"{shape}: max |closed form - direct| = {diff.max():.3e} dB, bound {bound.max():.3e} dB, "
          f"t* in [{t_star.min():.4f}, {t_star.max():.4f}]")
    assert np.isfinite(bound).all() and (diff <= bound).all(), (diff.max(), bound.max())
    assert (c.argmax(axis=1) == 6).all() and (direct.argmax(axis=1) == 6).all()
    top = np.sort(c, axis=1)
    assert (top[:, -1] - top[:, -2] > 2 * bound.max()).all()
    # the continuous maximiser: on the planted weight up to the noise, and where a fine scan peaks
    fine = np.arange(0.25, 0.35, 1e-4)
    cf, _ = CR.curve(m, fine, 1 - fine)
    assert np.abs(t_star - 0.3).max() < 0.02
    assert np.abs(fine[cf.argmax(axis=1)] - t_star).max() <= 1e-4


def test_the_bound_rejects_what_the_contract_forbids():
    """Raw fp32 moments, a dropped cross term and ddof = 0 each leave the bound on at least one hostile input."""
    seen = {"raw fp32": 0, "no cross term": 0, "ddof 0": 0}
    for name, (g, p1, p2) in CR.hostile().items():
        m, mb = CR.moments(g, p1, p2, with_bounds=True)
        c, _ = CR.curve(m, T_LIST, 1 - T_LIST)
        bound = CR.curve_bound(m, mb, T_LIST, 1 - T_LIST)
        if name == "constant":
            assert np.isnan(c).all() and np.isnan(bound).all()
            continue
        assert np.isfinite(c).all() and np.isfinite(bound).all(), name
        raw = CR.moments_raw_fp32(g, p1, p2)
        wrong = {"raw fp32": CR.curve(raw, T_LIST, 1 - T_LIST)[0],
                 "no cross term": CR.curve(m, T_LIST, 1 - T_LIST, cross=False)[0],
                 "ddof 0": CR.curve(m, T_LIST, 1 - T_LIST, ddof=0)[0]}
        seen["raw fp32"] += int((np.abs(raw[:, 6:] - m[:, 6:]) > mb[:, 6:]).any())
        for what, cw in wrong.items():
            d = np.abs(cw - c)
            seen[what] += int((~(d <= bound)).any())
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["raw fp32"] >= 2                                       # both the moments and the curve show it on 'counts'


def test_hostile_cases_behave_as_their_names_say():
    H = CR.hostile()
    m = CR.moments(*H["equal"])
    c, t = CR.curve(m, T_LIST, 1 - T_LIST)
    assert np.isnan(t).all() and np.isfinite(c).all() and np.ptp(c, axis=1).max() < 1e-6      # p1 == p2: a flat curve
    m = CR.moments(*H["constant"])
    assert (m[:, 1] == m[:, 2]).all() and (m[:, 6] == 0).all()
    m, mb = CR.moments(*H["counts"], with_bounds=True)
    assert (mb[:, 6:] < 1e-9 * np.abs(m[:, [6, 7, 8]]).max()).all()    # shifted sums keep 1e4-mean planes harmless


def test_core_curve_is_the_restatement():
    from diffsplitting_amd.core.psnr import MOMENT_NAMES, range_invariant_psnr_curve
    assert MOMENT_NAMES == CR.NAMES
    for name, (g, p1, p2) in list(CR.hostile(n=257).items()) + [("planted", CR.planted((3, 7, 9)))]:
        m, mb = CR.moments(g, p1, p2, with_bounds=True)
        c, t = CR.curve(m, T_LIST, 1 - T_LIST)
        ct, tt = range_invariant_psnr_curve(torch.from_numpy(m), T_LIST, 1 - T_LIST)
        assert ct.dtype == torch.float64 and ct.shape == (3, 20) and tt.shape == (3,)
        ct, tt = ct.numpy(), tt.numpy()
        assert (np.isnan(ct) == np.isnan(c)).all() and (np.isnan(tt) == np.isnan(t)).all(), name
        ok = ~np.isnan(c)
        assert (np.abs(ct - c)[ok] <= CR.curve_bound(m, mb, T_LIST, 1 - T_LIST)[ok]).all(), name
        assert np.allclose(tt[~np.isnan(t)], t[~np.isnan(t)], rtol=1e-12, atol=0)


def test_choose_times_is_the_argmax_of_the_nanmean_per_unit():
    from diffsplitting_amd.data.tiled_predict import choose_times
    t_list = np.arange(0, 1.0, 0.25)
    nan = np.nan
    curves = np.array([[9.0, 1.0, 2.0, 3.0],        # peaks at 0: not startable, the best of the rest is 0.75
                       [nan, 5.0, 1.0, 1.0],        # 0.25
                       [nan, nan, nan, nan],        # no curve
                       [7.0, nan, nan, nan],        # a value at 0 only: nothing to start from
                       [0.0, 0.0, 8.0, np.inf]])    # an exact fit wins
    prev = np.arange(10, dtype=np.float32).reshape(5, 2)
    out, chosen, means = choose_times(curves, np.arange(5), t_list, prev)
    assert out.dtype == np.float32 and np.array_equal(chosen[[0, 1, 4]], [0.75, 0.25, 0.75]) and np.isnan(chosen[[2, 3]]).all()
    assert np.array_equal(out[[0, 1, 4]], [[0.75] * 2, [0.25] * 2, [0.75] * 2]) and np.array_equal(out[[2, 3]], prev[[2, 3]])
    assert np.array_equal(np.isnan(means), np.isnan(curves))
    # frames: tiles 0-2 and 3-4; NaN rows do not enter the mean
    out, chosen, means = choose_times(curves, np.array([0, 0, 0, 1, 1]), t_list, prev)
    assert np.array_equal(means[0], [9.0, 3.0, 1.5, 2.0]) and np.array_equal(chosen, [0.25, 0.75])
    assert (out[:3] == 0.25).all() and (out[3:] == 0.75).all()
    out, chosen, _ = choose_times(curves[2:4], np.zeros(2, dtype=int), t_list, prev[2:4])
    assert np.isnan(chosen).all() and np.array_equal(out, prev[2:4])


def test_new_symbols_exported_and_abi_unchanged():
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core import psnr, psnr_based_t_refinement as R
    from diffsplitting_amd.data import tiled_predict
    for name in ("dsx_comoments_blocks", "dsx_comoments"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert _lib.lib.dsx_abi_version() == 2
    blocks = _lib.lib.dsx_comoments_blocks
    assert blocks(1) == 1 and blocks(64) == 1
    span = max(n for n in (1 << k for k in range(25)) if blocks(n) == 1)
    assert blocks(span + 1) == 2 and blocks(2 * span) == 2 and blocks(2 * span + 1) == 3
    assert 1 <= blocks(2048 * 2048) <= 65535 and 1 <= blocks(1 << 40) <= 65535
    for fn in (psnr.comoments, psnr.range_invariant_psnr_curve, R.estimate_time_from_estimates,
               tiled_predict.predict_tiled_refined):
        assert callable(fn)


def test_host_side_refusals():
    """Every refusal of dsx_comoments comes with a message before any device work (fake non-null device pointers)."""
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core.psnr import comoments
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    fake = C.c_void_p(4096)
    s6 = lambda *v: (C.c_int64 * 6)(*v)
    ok = s6(100, 1, 100, 1, 100, 1)
    assert lib.dsx_comoments_blocks(0) < 0 and "n = 0" in err()
    for k in range(3):
        ptrs = [fake, fake, fake]
        ptrs[k] = None
        assert lib.dsx_comoments(*ptrs, 2, 100, ok, fake, fake, None) < 0 and "null" in err()
    assert lib.dsx_comoments(fake, fake, fake, 2, 100, None, fake, fake, None) < 0 and "null" in err()
    assert lib.dsx_comoments(fake, fake, fake, 2, 100, ok, None, fake, None) < 0 and "null" in err()
    assert lib.dsx_comoments(fake, fake, fake, 2, 100, ok, fake, None, None) < 0 and "null" in err()
    for n in (0, -5):
        assert lib.dsx_comoments(fake, fake, fake, 2, n, ok, fake, fake, None) < 0 and "must be positive" in err()
    for planes in (-1, 65536):
        assert lib.dsx_comoments(fake, fake, fake, planes, 100, ok, fake, fake, None) < 0 and "0..65535" in err()
    for k in range(6):
        for bad in (0, -1):
            st = [100, 1, 100, 1, 100, 1]
            st[k] = bad
            assert lib.dsx_comoments(fake, fake, fake, 2, 100, s6(*st), fake, fake, None) < 0
            assert "at least 1" in err() and ("g", "p1", "p2")[k // 2] in err()
    for k, name in enumerate(("g", "p1", "p2")):
        st = [199, 2, 199, 2, 199, 2]                                  # a plane spans 99 * 2 + 1 = 199 elements
        assert lib.dsx_comoments(fake, fake, fake, 0, 100, s6(*st), fake, fake, None) == 0
        st[2 * k] = 198
        assert lib.dsx_comoments(fake, fake, fake, 2, 100, s6(*st), fake, fake, None) < 0
        assert "overlap" in err() and f"of {name} " in err()
    assert lib.dsx_comoments(fake, fake, fake, 0, 100, ok, fake, fake, None) == 0       # no planes: nothing to do
    # the Python face: CPU tensors are refused, as elsewhere
    x = torch.zeros(2, 8, 8)
    with pytest.raises(_lib.DsxError, match="comoments: g must be a CUDA float32 tensor"):
        comoments(x, x, x)


def _config(tmp_path, which):
    path = tmp_path / f"{which}.json"
    path.write_text(json.dumps({"name": "t", "model": {"which_model_G": which}}))
    return str(path)


def test_split_refuses_the_refine_flags_where_they_do_not_apply(tmp_path):
    from diffsplitting_amd import split
    indi, joint = _config(tmp_path, "indi"), _config(tmp_path, "joint_indi")
    flags = (("--refine-rounds", "2"), ("--refine-scope", "tile"), ("--refine-step", "0.1"))
    for flag, value in flags:
        with pytest.raises(SystemExit, match=f"{flag}.*joint_indi"):
            split.main(["-c", indi, flag, value])
        with pytest.raises(SystemExit, match=f"{flag}.*--mix-t"):
            split.main(["-c", joint, flag, value])
        for t_from in ("given", "classifier"):
            with pytest.raises(SystemExit, match=f"{flag}.*--t-from refined"):
                split.main(["-c", joint, "--mix-t", "0.3", "--t-from", t_from, "--time-predictor", joint, flag, value])
    with pytest.raises(SystemExit, match="--t-from.*joint_indi"):
        split.main(["-c", indi, "--t-from", "refined"])
    with pytest.raises(SystemExit, match="--t-from.*--mix-t"):
        split.main(["-c", joint, "--t-from", "refined"])
    base = ["-c", joint, "--mix-t", "0.3", "--t-from", "refined"]
    with pytest.raises(SystemExit, match="--refine-rounds -1"):
        split.main(base + ["--refine-rounds", "-1"])
    for bad in ("0", "1.5", "nan"):
        with pytest.raises(SystemExit, match="--refine-step"):
            split.main(base + ["--refine-step", bad])
    with pytest.raises(SystemExit):                                    # argparse's own: not one of the three scopes
        split.main(base + ["--refine-scope", "batch"])
    for extra, word in ((["--stitch", "blend"], "--stitch blend"), (["--validate"], "--validate"),
                        (["--sample-seed", "1", "--noise-field"], "--noise-field")):
        with pytest.raises(SystemExit, match=word):
            split.main(base + extra)
