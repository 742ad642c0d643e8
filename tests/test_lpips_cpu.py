"""LPIPS without a GPU: the C ABI's new exports, weight-key handling and every refusal, the sensitivity of the float64
restatement (tests/lpips_ref.py) to deliberate defects at the tolerance the GPU suite uses, and the yardstick that
tolerance is derived from.  `-m "not gpu"`."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from tests import lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_lpips_create", "dsx_lpips_destroy", "dsx_lpips_forward", "dsx_lpips_frames", "dsx_lpips_layers",
       "dsx_lpips_copy_workspace")
torch.set_grad_enabled(False)


def test_new_symbols_declared_bound_and_exported():
    from diffsplitting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    declared = set(re.findall(r"\b(dsx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.dsx_abi_version() == 2


def test_both_key_layouts_give_a_handle():
    from diffsplitting_amd.core.lpips import LPIPS, split_state_dict
    sd = R.synth_state_dict()
    assert LPIPS(net='alex', state_dict=sd)._h
    assert LPIPS(state_dict=R.to_split_layout(sd))._h
    t1, l1 = split_state_dict(sd)
    t2, l2 = split_state_dict(R.to_split_layout(sd))
    assert all(torch.equal(a, b) for a, b in zip(t1 + l1, t2 + l2))
    assert [tuple(t.shape) for t in t1[::2]] == [s for _, _, s in R.TRUNK]


def test_weights_from_a_local_file_and_from_the_environment(tmp_path, monkeypatch):
    from diffsplitting_amd.core.lpips import ENV, LPIPS
    sd = R.synth_state_dict()
    split = R.to_split_layout(sd)
    f_trunk, f_lin, f_all = tmp_path / "alexnet.pth", tmp_path / "alex.pth", tmp_path / "all.pth"
    torch.save({k: v for k, v in split.items() if k.startswith("features.")}, f_trunk)
    torch.save({k: v for k, v in split.items() if k.startswith("lin")}, f_lin)
    torch.save(sd, f_all)
    assert LPIPS(weights_path=str(f_all))._h
    assert LPIPS(weights_path=[str(f_trunk), str(f_lin)])._h
    monkeypatch.setenv(ENV, os.pathsep.join([str(f_trunk), str(f_lin)]))
    assert LPIPS(net='alex')._h


def test_refusals_by_name(monkeypatch, tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core import lpips as L
    monkeypatch.delenv(L.ENV, raising=False)
    sd = R.synth_state_dict()
    for kw, word in ((dict(net='vgg'), "vgg"), (dict(net='squeeze'), "squeeze"), (dict(version='0.0'), "0.0"),
                     (dict(spatial=True), "spatial")):
        with pytest.raises(DsxError, match=re.escape(word)):
            L.LPIPS(state_dict=sd, **kw)
    # no weights: says which two files to supply, and never tries to get them
    with pytest.raises(DsxError) as e:
        L.LPIPS(net='alex')
    msg = str(e.value)
    assert "features." in msg and "alex.pth" in msg and L.ENV in msg and "never fetches" in msg
    with pytest.raises(DsxError, match="does not exist"):
        L.LPIPS(weights_path=str(tmp_path / "missing.pth"))
    # wrong shape, missing key, unknown key, wrong scaling constants: by key name
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(DsxError, match=r"net\.slice2\.3\.weight has shape \(192, 64, 3, 3\), expected \(192, 64, 5, 5\)"):
        L.LPIPS(state_dict=bad)
    bad = dict(sd)
    bad["lin2.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(DsxError, match=r"lin2\.model\.1\.weight"):
        L.LPIPS(state_dict=bad)
    bad = dict(sd)
    del bad["net.slice4.8.bias"]
    with pytest.raises(DsxError, match=r"missing net\.slice4\.8\.bias"):
        L.LPIPS(state_dict=bad)
    bad = dict(sd)
    bad["net.slice6.12.weight"] = torch.zeros(1)
    with pytest.raises(DsxError, match=r"unexpected key 'net\.slice6\.12\.weight'"):
        L.LPIPS(state_dict=bad)
    bad = dict(sd)
    bad["scaling_layer.scale"] = torch.tensor([.5, .5, .5]).view(1, 3, 1, 1)
    with pytest.raises(DsxError, match=r"scaling_layer\.scale"):
        L.LPIPS(state_dict=bad)


def _raw_create(numel_override=None):
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core.lpips import split_state_dict
    trunk, lin = split_state_dict(R.synth_state_dict())
    tn = [t.numel() for t in trunk]
    ln = [t.numel() for t in lin]
    for (which, i), n in (numel_override or {}).items():
        (tn if which == "trunk" else ln)[i] = n
    h = C.c_void_p()
    rc = _lib.lib.dsx_lpips_create((C.c_void_p * 10)(*[t.data_ptr() for t in trunk]), (C.c_int64 * 10)(*tn),
                                   (C.c_void_p * 5)(*[t.data_ptr() for t in lin]), (C.c_int64 * 5)(*ln), C.byref(h))
    return rc, h, _lib.lib.dsx_last_error().decode()


def test_library_validates_counts_and_sizes_by_name():
    """The C ABI itself refuses (host side, before any device work): wrong element counts by key name, inputs for which
    a stage of the trunk would be empty, and batches whose largest tensor passes 32-bit byte offsets."""
    from diffsplitting_amd import _lib
    rc, _, msg = _raw_create({("trunk", 4): 5})
    assert rc == -1 and "net.slice3.6.weight" in msg and "(384, 192, 3, 3)" in msg
    rc, _, msg = _raw_create({("trunk", 1): 63})
    assert rc == -1 and "net.slice1.0.bias" in msg
    rc, _, msg = _raw_create({("lin", 4): 255})
    assert rc == -1 and "lin4.model.1.weight" in msg
    rc, h, _ = _raw_create()
    assert rc == 0 and h
    dummy = C.c_void_p(256)                        # never dereferenced: the refusals come first
    try:
        for (H, W) in ((30, 64), (64, 30), (8, 8)):
            rc = _lib.lib.dsx_lpips_forward(h, dummy, dummy, 1, H, W, dummy, None, None)
            assert rc == -1 and "H, W >= 31" in _lib.lib.dsx_last_error().decode()
        rc = _lib.lib.dsx_lpips_forward(h, dummy, dummy, 40, 2048, 2048, dummy, None, None)
        assert rc == -1 and "2 GiB" in _lib.lib.dsx_last_error().decode()
        rc = _lib.lib.dsx_lpips_frames(h, dummy, dummy, 3, 64, 64, 2, 2, 0, dummy, None)
        assert rc == -1 and "channel" in _lib.lib.dsx_last_error().decode()
        rc = _lib.lib.dsx_lpips_frames(h, dummy, dummy, 3, 20, 64, 2, 0, 0, dummy, None)
        assert rc == -1 and "H, W >= 31" in _lib.lib.dsx_last_error().decode()
    finally:
        _lib.lib.dsx_lpips_destroy(h)


def test_forward_fails_loudly_without_gpu():
    from diffsplitting_amd import _lib
    from diffsplitting_amd.core.lpips import LPIPS
    from diffsplitting_amd.core.metrics import calculate_lpips
    if _lib.lib.dsx_device_count() > 0:
        pytest.skip("GPU present")
    m = LPIPS(state_dict=R.synth_state_dict())
    a, b = R.make_pair(1, 64, 64, 1)
    with pytest.raises(_lib.DsxError):
        m(a, b)
    with pytest.raises(_lib.DsxError):
        m.frames(torch.zeros(1, 64, 64, 2), torch.zeros(1, 64, 64, 2), 0)
    with pytest.raises(_lib.DsxError):
        calculate_lpips(*R.make_frames(), m)
    rc, h, _ = _raw_create()
    dummy = C.c_void_p(256)
    try:
        assert _lib.lib.dsx_lpips_forward(h, dummy, dummy, 1, 64, 64, dummy, None, None) == -2
        assert "no HIP device" in _lib.lib.dsx_last_error().decode()
    finally:
        _lib.lib.dsx_lpips_destroy(h)


def test_nothing_in_the_module_reaches_for_the_network():
    from diffsplitting_amd.core import lpips as L
    src = inspect.getsource(L).lower()
    for word in ("http", "urlopen", "urlretrieve", "download", "load_state_dict_from_url", "pretrained=true", "hub."):
        assert word not in src, word


def test_yardstick_is_a_float32_rounding_figure():
    """The GPU tolerance = MARGIN x this + ABS_FLOOR.  float32 has a 6e-8 unit roundoff and the longest sum has 3456
    terms: the restatement in float32 must sit between one rounding and a few thousand of them."""
    y = R.fp32_yardstick()
    print(f"fp32 yardstick (max relative error of the float32 restatement vs float64): {y:.3e}; "
          f"GPU bound = {R.MARGIN:g} x that, relative, + {R.ABS_FLOOR:g}")
    assert 6e-8 <= y <= 3456 * 6e-8


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_restatement_is_sensitive_to_each_defect(defect):
    """Each deliberate defect moves the float64 result by more than the bound the GPU test allows, on inputs of the
    GPU suite: the 97 x 131 pair (131 -> 32 columns after conv1: floor and ceil pooling differ), and for the dropped
    1e-10 the constant image whose tap-1 features are all zero (0 / 0 without it)."""
    sd = R.synth_state_dict()
    if defect == "no_eps":
        in0, in1 = R.constant_image(1, 64, 64), R.make_pair(1, 64, 64, 9)[1]
    else:
        in0, in1 = R.make_pair(*R.CASES["b1_97x131"])
    good = R.lpips_ref(sd, in0, in1)
    assert torch.isfinite(good).all() and (good > 0).all()
    moved = (R.lpips_ref(sd, in0, in1, defect=defect) - good).abs()
    print(f"{defect}: moved {moved.max().item():.3e}, bound {R.bound(good).max().item():.3e}")
    assert not bool((moved <= 10 * R.bound(good)).any())      # NaN (no_eps) counts as moved


def test_restatement_basics():
    sd = R.synth_state_dict()
    in0, in1 = R.make_pair(2, 64, 64, 1)
    assert torch.equal(R.lpips_ref(sd, in0, in0), torch.zeros(2, dtype=torch.float64))
    tot, taps = R.lpips_ref(sd, in0, in1, per_layer=True)
    assert taps.shape == (2, 5) and torch.allclose(taps.sum(1), tot) and (taps > 0).all()
    # symmetric in its arguments; each pair on its own
    assert torch.allclose(R.lpips_ref(sd, in1, in0), tot, rtol=1e-12)
    assert torch.allclose(R.lpips_ref(sd, in0[1:], in1[1:]), tot[1:], rtol=1e-12)
    tgt, prd = R.make_frames()
    fr = R.frames_ref(sd, tgt, prd)
    assert sorted(fr) == [0, 1] and all(v.shape == (3,) and (v > 0).all() for v in fr.values())


def test_restatement_against_the_lpips_package():
    """Only where the `lpips` package and a local weight file exist; otherwise parity against the package stays
    unpinned (DESIGN.md says so)."""
    lp = pytest.importorskip("lpips", reason="the lpips package is not installed: parity against it stays unpinned")
    if not hasattr(lp, "pretrained_networks"):
        pytest.skip("`lpips` resolves to this project's alias, not the package")
    path = os.environ.get("DSX_LPIPS_WEIGHTS")
    if not path or not os.path.isfile(path):
        pytest.skip("no local LPIPS weight file (DSX_LPIPS_WEIGHTS): parity against the package stays unpinned")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    model = lp.LPIPS(net='alex', pretrained=False, pnet_rand=True, verbose=False)
    model.load_state_dict(sd, strict=False)
    model.eval()
    in0, in1 = R.make_pair(2, 97, 131, 3)
    want = model(in0, in1).flatten().double()
    got = R.lpips_ref(sd, in0, in1)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-7)
