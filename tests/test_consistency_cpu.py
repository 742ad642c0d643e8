"""dsx_consistency without a device: the header and the binding, every refusal of the entry point, the properties of
the restatement (tests/consistency_ref.py) that the feature rests on, the mistakes its contract rejects, and the command
line's refusals (before any rank is started, before anything touches the device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import consistency_ref as ref
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_carry_the_entry_points():
    from diffsplitting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    assert re.search(r"#define DSX_ABI_VERSION 2\b", hdr) and _lib.lib.dsx_abi_version() == 2
    assert re.search(r"^int dsx_consistency_blocks\(int64_t plane\);", hdr, flags=re.M)
    assert re.search(r"^int dsx_consistency\(const void\* input_dev, int pix, const float\* mean_dev,", hdr, flags=re.M)
    assert "dsx_consistency_blocks" in _lib.SIGNATURES and len(_lib.SIGNATURES["dsx_consistency"][1]) == 18
    assert _lib.lib.dsx_consistency_blocks(1) == 1 and _lib.lib.dsx_consistency_blocks(37 * 41) == 1
    assert _lib.lib.dsx_consistency_blocks(130 * 129) == 5 and _lib.lib.dsx_consistency_blocks(1 << 30) == 1024
    from diffsplitting_amd import engine
    from diffsplitting_amd.core import consistency
    assert callable(engine.consistency) and callable(consistency.consistency)


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    """Fake non-null device pointers, far apart: a call that got past its checks would not come back with these
    messages."""
    from diffsplitting_amd import _lib
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    P = lambda k: C.c_void_p(k << 32)                      # 4 GiB apart: nothing overlaps by accident
    vec = lambda *v: np.asarray(v, dtype=np.float64)
    base = dict(inp=P(1), pix=_lib.PIX_U16, mean=P(2), std=P(3), frames=2, plane=100, C=2, a=vec(2.0, 3.0), b=vec(0.0, 1.0),
                w=vec(1.0, 1.0), clip=-1.0, nv=0.0, map=P(4), om=P(5), os=P(6), out=P(7), part=P(8))

    def call(**kw):
        a = dict(base, **kw)
        return lib.dsx_consistency(a["inp"], a["pix"], a["mean"], a["std"], a["frames"], a["plane"], a["C"], a["a"], a["b"],
                                   a["w"], a["clip"], a["nv"], a["map"], a["om"], a["os"], a["out"], a["part"], None)

    for k in ("inp", "mean", "a", "b", "w"):
        assert call(**{k: None}) < 0 and "null" in err(), k
    assert call(part=None) < 0 and "out_dev needs partial_dev" in err()
    for frames in (0, -1, 65536):
        assert call(frames=frames) < 0 and f"{frames} frames, must be in 1..65535" in err()
    for plane in (0, -7):
        assert call(plane=plane) < 0 and f"plane = {plane} pixels" in err()
        assert lib.dsx_consistency_blocks(plane) < 0 and f"plane = {plane} pixels" in err()
    for ch in (0, 5):
        assert call(C=ch, a=vec(1, 1, 1, 1, 1), b=vec(0, 0, 0, 0, 0), w=vec(1, 1, 1, 1, 1)) < 0 and f"C = {ch} channels" in err()
    for pix in (_lib.PIX_U32, 4, -1):
        assert call(pix=pix) < 0 and f"pix = {pix}" in err()
    for bad in (0.0, -2.0):
        assert call(a=vec(2.0, bad)) < 0 and "scale[1]" in err() and "must be > 0" in err()
    for k in ("a", "b", "w"):
        for bad in (np.nan, np.inf):
            assert call(**{k: vec(bad, 1.0)}) < 0 and "channel 0 is not finite" in err(), k
    assert call(clip=np.inf) < 0 and "clip" in err() and "not finite" in err()
    assert call(clip=np.nan) < 0 and "clip" in err()
    assert call(nv=np.nan) < 0 and "noise_var" in err() and "not finite" in err()
    assert call(nv=-1e-300) < 0 and "noise_var" in err() and "must not be negative" in err()
    assert call(w=vec(0.0, 0.0)) < 0 and "every weight is 0" in err()
    assert call(std=None) < 0 and "out_std_dev without std_dev" in err()
    assert call(map=None, om=None, os=None, out=None) < 0 and "no output" in err()
    # aliasing: nothing but in place
    assert call(map=base["inp"]) < 0 and "map_dev overlaps input_dev" in err()
    assert call(om=base["std"]) < 0 and "out_mean_dev overlaps std_dev" in err()
    assert call(os=base["mean"]) < 0 and "out_std_dev overlaps mean_dev" in err()
    assert call(om=C.c_void_p((2 << 32) + 4)) < 0 and "out_mean_dev overlaps mean_dev" in err()      # shifted: not in place
    assert call(om=P(5), os=P(5)) < 0 and "out_mean_dev overlaps out_std_dev" in err()
    assert call(out=base["part"]) < 0 and "out_dev overlaps partial_dev" in err()


# ----------------------------------------------------------------------------- the restatement's own properties
def _truth_case(std, rho, seed=0, n=3000):
    """integer x = w0 t0 + w1 t1 from uint16 truths, a prediction equal to the truth plus noise, normalised to fp32"""
    rng = np.random.default_rng(seed)
    w = np.array([2.0, 3.0])
    a, b = np.array(ref.A[:2]), np.array(ref.B[:2])
    t = rng.integers(0, 8000, (1, n, 2)).astype(np.uint16).astype(np.float64)
    x = (w * t).sum(-1)
    assert (x == np.round(x)).all() and x.max() < 65536
    sd = None
    if std:
        sd = ((2.0 + 6.0 * rng.random(t.shape)) / a).astype(np.float32)
    mean = ((t + 5.0 * rng.standard_normal(t.shape) - b) / a).astype(np.float32)
    return dict(x=x.astype(np.uint16), mean=mean, std=sd, a=a, b=b, w=w, clip=-1.0, noise_var=rho * rho), t


def _raw(norm, k):
    return norm.astype(np.float64) * k["a"] + k["b"]


def test_the_orthogonal_projection_meets_the_constraint_and_cannot_hurt():
    k, t = _truth_case(std=False, rho=0.0)
    got = ref.restate(**k)
    x = k["x"].astype(np.float64)
    # in double, before the result is rounded to fp32: recompute p' as the contract does
    p = got["p"]
    den = (k["w"] * k["w"]).sum()
    pp = p + (k["w"] * got["r"][..., None]) / den
    resid = x - (k["w"] * pp).sum(-1)
    assert (np.abs(resid) <= 8 * np.spacing(x.max())).all()              # a few ulps of |x|
    before, after = ((p - t) ** 2).sum(-1), ((pp - t) ** 2).sum(-1)
    assert (after <= before * (1 + 2.0 ** -40)).all() and (after < before).mean() > 0.99
    # the fp32 outputs are that projection, rounded once
    assert ref.same_bits(got["out_mean"], ((pp - k["b"]) / k["a"]).astype(np.float32))
    assert got["out_std"] is None                                        # no spread in, none out


def test_conditioning_on_the_sum_shrinks_the_spread_and_removes_its_variance_along_w():
    k, t = _truth_case(std=True, rho=0.0)
    got = ref.restate(**k)
    v = got["v"]
    den = got["den"]
    vw = v * k["w"]
    vp = v - (vw * vw) / den[..., None]
    assert (vp <= v).all() and (vp >= 0).all()
    # The conditioned posterior has no variance left along w: w' V' w = 0 with V' = V - V w w' V / den.  The contract keeps
    # the DIAGONAL of V' only (the marginal spreads), so for two channels sum w^2 v' alone is not 0 -- it is what the
    # off-diagonal terms -2 (w0^2 v0)(w1^2 v1) / den cancel.  With one channel it is 0 by itself (checked below).
    s = k["w"] * k["w"] * v
    along = (k["w"] * k["w"] * vp).sum(-1) - 2 * s[..., 0] * s[..., 1] / den
    assert (np.abs(along) <= 8 * np.spacing(den)).all()
    one = dict(k, mean=k["mean"][..., :1], std=k["std"][..., :1], a=k["a"][:1], b=k["b"][:1], w=k["w"][:1])
    got1 = ref.restate(**one)
    v1 = got1["v"][..., 0]
    w1 = one["w"][0]
    vp1 = v1 - ((v1 * w1) * (v1 * w1)) / got1["den"]
    assert (np.abs(w1 * w1 * vp1) <= 8 * np.spacing(got1["den"])).all()
    assert (got1["out_std"].astype(np.float64) * one["a"] <= 8 * np.sqrt(np.spacing(got1["den"]))[..., None] / w1).all()
    assert (_raw(got["out_std"], dict(a=k["a"], b=0.0)) <= _raw(k["std"], dict(a=k["a"], b=0.0)) * (1 + 2.0 ** -20)).all()
    # an honest spread: chi2 of this synthetic case is the noise we added (5 counts per channel) against sd of 2..8
    rows = got["rows"]
    assert rows[0, 6] == rows[0, 0] == v.shape[1] and rows[0, 7] > 0


def test_with_unbounded_noise_nothing_moves():
    k, _ = _truth_case(std=True, rho=1e160)
    got = ref.restate(**k)
    assert ref.same_bits(got["out_mean"], k["mean"])
    # the spread is re-rounded through double; it moves by at most one fp32 ulp and never grows
    assert (np.abs(got["out_std"].astype(np.float64) - k["std"]) <= np.spacing(k["std"])).all()
    assert np.isfinite(got["rows"]).all() and got["rows"][0, 7] < 1e-290


def test_saturated_pixels_are_left_alone_and_counted():
    k = ref.case("u16", 2, 37 * 41, 2, clip="all", std="given")
    got = ref.restate(**k)
    sat = k["x"] >= k["clip"]
    assert sat[1].all() and 0 < sat[0].sum() < sat[0].size
    assert ref.same_bits(got["out_mean"][sat], k["mean"][sat]) and ref.same_bits(got["out_std"][sat], k["std"][sat])
    assert got["rows"][1].tolist() == [0, sat[1].sum(), 0, 0, 0, 0, 0, 0, np.inf, -np.inf]
    assert got["rows"][0, 1] == sat[0].sum() and got["rows"][0, 0] == (~sat[0]).sum()
    zero = ref.restate(**ref.case("u8", 1, 96, 3, std="zero"))
    assert zero["rows"][0, 6] == 0 and zero["rows"][0, 7] == 0 and not zero["out_std"].any()
    assert ref.same_bits(zero["out_mean"], ref.case("u8", 1, 96, 3, std="zero")["mean"])


@pytest.mark.parametrize("which", ["fma_m", "sat_summed", "vw2", "acc32", "no_noise"])
def test_the_contract_rejects_typical_mistakes(which):
    """Each mistake is injected into a copy of the restatement; what it produces must fall outside the contract (bits of
    the fp32 outputs, exact counts, sums within the derived bound) on the shared cases.  'fma_m' shows where r is
    rounding noise: the `tight` case, whose prediction equals its truth up to the fp32 rounding of the mean."""
    k = ref.case("u16", 2, 37 * 41, 2, clip="on", std="given", tight=which == "fma_m")
    good = ref.restate(**k)
    assert ref.agrees(dict(good), good)
    bad = ref.mistaken(**k, which=which)
    assert not ref.agrees(dict(bad), good)
    if which != "vw2":                                  # the correction's numerator enters no sum: the outputs show it
        assert not ref.agrees({"rows": bad["rows"]}, good), "the row alone must show it"
    if which in ("vw2", "no_noise"):
        assert not ref.agrees({n: bad[n] for n in ("map", "out_mean", "out_std")}, good)


def test_the_host_side_report_folds_the_rows():
    from diffsplitting_amd.core.consistency import fold_rows, report_of_row
    k = ref.case("u16", 3, 96, 2, clip="all", std="given")
    rows = ref.restate(**k)["rows"]
    tot = fold_rows(rows)
    assert tot[0] == rows[:, 0].sum() and tot[1] == rows[:, 1].sum() and tot[8] == rows[:, 8].min()
    rep = report_of_row(tot, True)
    assert rep["pixels"] == int(tot[0]) and rep["rms"] == np.sqrt(tot[3] / tot[0]) and rep["bias"] == tot[2] / tot[0]
    assert rep["relative"] == np.sqrt(tot[3] / tot[5]) and rep["chi2"] == tot[7] / tot[6]
    assert rep["explained"] == 1.0 - tot[3] / (tot[5] - tot[4] * tot[4] / tot[0])
    empty = report_of_row(rows[2], True)                                 # the saturated frame
    assert empty["pixels"] == 0 and empty["saturated"] == 96
    assert all(empty[n] is None for n in ("rms", "bias", "relative", "explained", "min", "max", "chi2"))
    assert "chi2" not in report_of_row(tot, False)


# ----------------------------------------------------------------------------- drivers and command line
def test_the_drivers_refuse_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd import _lib
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tile_predict

    def touched(*a, **k):
        raise AssertionError("the refusal came too late")
    monkeypatch.setattr(_lib, "require_gpu", touched)

    class Other:
        _target_channel_idx = None

    class Stack(Other):
        def acquisition(self):
            touched()
    chk = lambda *a, **k: tile_predict._check_consistency("predict_stack", *a, **k)
    assert chk(False, 0.0, None, Other(), 2) is None
    with pytest.raises(DsxError, match="consistency_noise= / consistency_weights= without consistency="):
        chk(False, 1.0, None, Stack(), 2)
    with pytest.raises(DsxError, match="consistency = 'map': False, True"):
        chk("map", 0.0, None, Stack(), 2)
    with pytest.raises(DsxError, match="predict_stack: consistency=.*Other does not expose one"):
        chk(True, 0.0, None, Other(), 2)
    with pytest.raises(DsxError, match="3 channel weights for a prediction of 2 channels"):
        chk(True, 0.0, (1, 1, 1), Stack(), 2)
    with pytest.raises(DsxError, match="noise = -1"):
        chk(True, -1, None, Stack(), 2)
    with pytest.raises(DsxError, match="consistency='project' with quantiles= / ranks=.*not projected"):
        chk("project", 0.0, None, Stack(), 2, q=(0.5,))
    one = Stack()
    one._target_channel_idx = 1
    with pytest.raises(DsxError, match="target_channel_idx = 1"):
        chk(True, 0.0, None, one, 1)
    project, rho, w = chk("project", 2.0, (1, 2), Stack(), 2)
    assert project is True and rho == 2.0 and w.tolist() == [1.0, 2.0]


def test_split_refuses_the_consistency_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    from diffsplitting_amd import parallel, split
    from diffsplitting_amd.data.normalization import save_normalization

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    indi = write_config(tmp_path, "indi")
    one = write_config(tmp_path, "indi", target_channel_idx=1)
    nd = {"mean_input": 2000.0, "std_input": 900.0, "target0_max": 3000.0, "target1_max": 2201.0, "input_max": 5201.0,
          "mean_target": np.array([1500.0, 1100.5]),
          "std_target": np.array([1234.5, 987.25])}
    norm, norm1 = str(tmp_path / "n.json"), str(tmp_path / "n1.json")
    save_normalization(norm, nd, data_type="Hagen", channel_weights=[1, 1], max_qval=0.98, upper_clip=False,
                       target_channel_idx=None)
    save_normalization(norm1, nd, data_type="Hagen", channel_weights=[1, 1], max_qval=0.98, upper_clip=False,
                       target_channel_idx=1)
    stack = str(tmp_path / "s.npy")
    np.save(stack, np.zeros((1, 32, 32), np.uint16))
    inp = ["--input", stack, "--norm", norm]
    R = ["--consistency-report", str(tmp_path / "c.json")]

    def refused(argv, match, config=indi):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", config] + argv)

    refused(["--project"], "--project: only with --input FILE.*synthetic frames")
    refused(["--project", "--frames", "f.npy"], "--project: only with --input FILE.*--frames")
    refused(R + ["--datapath"], "--consistency-report: only with --input FILE.*--datapath")
    refused(["--consistency-map", "m.npy"], "--consistency-map: only with --input FILE")
    refused(["--consistency-noise", "1"], "--consistency-noise: only with --input FILE")
    refused(["--channel-weights", "1,1"], "--channel-weights: only with --input FILE")
    refused(inp + ["--consistency-noise", "1"], "--consistency-noise: only with --consistency-report, --consistency-map or")
    refused(["--input", stack, "--norm", norm1, "--project"], "--project: the config predicts one channel", config=one)
    refused(inp + ["--project", "--channel-weights", "1,2,3"], "--channel-weights 1,2,3: 3 weights, the split has two")
    refused(inp + ["--project", "--channel-weights", "1"], "--channel-weights 1: 1 weights")
    refused(inp + ["--project", "--channel-weights", "a,b"], "--channel-weights a,b: W0,W1")
    refused(inp + ["--project", "--channel-weights", "0,0"], "--channel-weights 0,0: finite, and not both zero")
    refused(inp + ["--project", "--consistency-noise", "-1"], "--consistency-noise -1.0: rho in raw counts")
    refused(inp + ["--consistency-report", "c.txt"], "--consistency-report c.txt: a .json file")
    refused(inp + ["--consistency-map", "m.png"], "--consistency-map m.png: a .npy or .tif file")
    refused(inp + ["--project", "--samples", "4", "--quantiles", "0.5", "--quantile-out", "q.npy"],
            "--project with --quantile-out")
    refused(inp + ["--project", "--samples", "1", "--std-out", "s.npy"], "--std-out.*--samples 2")
