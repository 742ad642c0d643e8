"""Input-only stacks and N-sample moments, the parts that need no GPU: the normalisation file's round trip and its
refusals, the command line's refusals (before any rank is started, before anything touches the device), the argument
checks of dsx_tileplan_gather_input / dsx_moments_update / dsx_moments_finish, and the file checks of
InputStackTiledPred."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsx_tileplan_gather_input", "dsx_moments_update", "dsx_moments_finish")


def test_new_exports_are_declared_and_additive():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert len(_lib.SIGNATURES["dsx_tileplan_gather_input"][1]) == 11
    assert len(_lib.SIGNATURES["dsx_moments_update"][1]) == 6 and len(_lib.SIGNATURES["dsx_moments_finish"][1]) == 7
    assert "#define DSX_ABI_VERSION 2" in header and _lib.lib.dsx_abi_version() == 2


# ----------------------------------------------------------------------------- normalisation file
AWKWARD = [
    dict(mean_input=0.1 + 0.2, std_input=1e-300, mean_target=np.array([float(np.float32(1.1))]),
         std_target=np.array([2.0 / 3.0]), target0_max=np.float64(1993.0000000000002), target1_max=5e-324,
         input_max=1.7976931348623157e308),
    dict(mean_input=np.float64(-123.456789012345678), std_input=np.float32(0.1), mean_target=np.array([0.1 + 0.2, -0.0]),
         std_target=np.array([1e-300, float(np.float32(1e-3))]).reshape(2, 1, 1), target0_max=None, target1_max=None,
         input_max=None),
]


@pytest.mark.parametrize("nd", AWKWARD)
@pytest.mark.parametrize("idx", [None, 1])
def test_normalization_round_trip_is_exact(tmp_path, nd, idx):
    from diffsplitting_amd.data.normalization import FORMAT, VERSION, load_normalization, save_normalization
    path = str(tmp_path / "norm.json")
    save_normalization(path, nd, data_type="Hagen", channel_weights=[1, 0.3], max_qval=0.98, upper_clip=True,
                       target_channel_idx=idx)
    back, meta = load_normalization(path)
    assert sorted(back) == sorted(nd)
    for k, v in nd.items():
        if k in ("mean_target", "std_target"):
            want = np.asarray(v, dtype=np.float64).reshape(-1)
            assert isinstance(back[k], np.ndarray) and back[k].dtype == np.float64 and back[k].shape == want.shape
            assert np.array_equal(back[k].view(np.int64), want.view(np.int64)), k      # bit for bit (also -0.0)
        elif v is None:
            assert back[k] is None
        else:
            assert type(back[k]) is np.float64 and back[k] == np.float64(v), k
            assert np.float64(back[k]).tobytes() == np.float64(v).tobytes(), k
    assert meta["format"] == FORMAT and meta["version"] == VERSION
    assert meta["data_type"] == "Hagen" and meta["channel_weights"] == [1.0, 0.3] and meta["max_qval"] == 0.98
    assert meta["upper_clip"] is True and meta["target_channel_idx"] == idx
    # the normalisation arithmetic of the datasets is float64 with these values: the strong type survives the file
    assert (np.float32(3.0) - back["mean_input"]).dtype == np.float64


def _good(tmp_path):
    from diffsplitting_amd.data.normalization import save_normalization
    path = str(tmp_path / "good.json")
    save_normalization(path, AWKWARD[0], data_type="Hagen", channel_weights=None, max_qval=0.98, upper_clip=False,
                       target_channel_idx=None)
    return path, json.load(open(path))


def test_normalization_refuses_malformed_files_by_name(tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.normalization import load_normalization, save_normalization
    path, doc = _good(tmp_path)

    def refused(change, match):
        d = json.loads(json.dumps(doc))
        change(d)
        bad = str(tmp_path / "bad.json")
        with open(bad, "w") as f:
            json.dump(d, f)                                           # (allow_nan: writes NaN / Infinity literals)
        with pytest.raises(DsxError, match=match):
            load_normalization(bad)

    refused(lambda d: d.update(format="something.else"), "format 'something.else'")
    refused(lambda d: d.pop("format"), "format None")
    refused(lambda d: d.update(version=2), "version 2")
    for k in ("data_type", "channel_weights", "max_qval", "upper_clip", "target_channel_idx", "normalization"):
        refused(lambda d, k=k: d.pop(k), f"'{k}' is missing")
    for k in ("mean_input", "std_input", "mean_target", "std_target", "target0_max", "target1_max", "input_max"):
        refused(lambda d, k=k: d["normalization"].pop(k), f"normalization.{k}' is missing")
    refused(lambda d: d["normalization"].update(std_input=0.0), "std_input = 0.0 must be positive")
    refused(lambda d: d["normalization"].update(std_input=-1.0), "std_input = -1.0 must be positive")
    refused(lambda d: d["normalization"].update(std_input=float("inf")), "std_input = inf is not finite")
    refused(lambda d: d["normalization"].update(std_target=[float("nan")]), "std_target = nan is not finite")
    refused(lambda d: d["normalization"].update(std_target=[0.0]), "std_target = 0.0 must be positive")
    refused(lambda d: d["normalization"].update(mean_target=[float("-inf")]), "mean_target = -inf is not finite")
    refused(lambda d: d["normalization"].update(mean_input=None), "mean_input = None is not a number")
    refused(lambda d: d["normalization"].update(std_target=[1.0, 2.0]), "one pair per target channel")
    refused(lambda d: d["normalization"].update(mean_target=3.0), "mean_target must be a list")
    with open(str(tmp_path / "text.json"), "w") as f:
        f.write("not json")
    with pytest.raises(DsxError, match="not a normalisation file"):
        load_normalization(str(tmp_path / "text.json"))
    # what could not be loaded is not written either
    for k, v, match in (("std_input", 0.0, "must be positive"), ("mean_input", float("nan"), "not finite")):
        with pytest.raises(DsxError, match=match):
            save_normalization(str(tmp_path / "w.json"), dict(AWKWARD[0], **{k: v}), data_type="Hagen", channel_weights=None,
                               max_qval=0.98, upper_clip=False, target_channel_idx=None)
    with pytest.raises(DsxError, match="no 'input_max'"):
        save_normalization(str(tmp_path / "w.json"), {k: v for k, v in AWKWARD[0].items() if k != "input_max"},
                           data_type="Hagen", channel_weights=None, max_qval=0.98, upper_clip=False, target_channel_idx=None)


# ----------------------------------------------------------------------------- command line
def test_split_refuses_the_new_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    """Every refusal of the issue's section 4 is a SystemExit that names the flag, raised on the command line, the config
    and the normalisation file alone: no rank is started and the process group (the first thing that touches the
    device) is never initialised."""
    from diffsplitting_amd import parallel, split
    from diffsplitting_amd.data.normalization import save_normalization

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    indi, joint = write_config(tmp_path, "indi"), write_config(tmp_path, "joint_indi")
    norm, cifar = str(tmp_path / "n.json"), str(tmp_path / "cifar.json")
    for path, dt in ((norm, "Hagen"), (cifar, "cifar10")):
        save_normalization(path, AWKWARD[1], data_type=dt, channel_weights=None, max_qval=0.98, upper_clip=False,
                           target_channel_idx=None)
    stack = str(tmp_path / "s.npy")
    np.save(stack, np.zeros((1, 32, 32), np.uint16))

    def refused(argv, match, config=indi):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", config] + argv)

    refused(["--input", stack], "--input needs --norm")
    refused(["--input", stack, "--norm", norm, "--datapath"], "--input with --datapath")
    refused(["--input", stack, "--norm", norm, "--frames", "f.npy"], "--input with --frames")
    refused(["--input", stack, "--norm", norm, "--validate"], "--input with --validate")
    refused(["--input", stack, "--norm", norm, "--mix-t", "0.3", "--t-from", "given"], "--input with --mix-t", config=joint)
    refused(["--input", stack, "--norm", norm], "--input with a joint_indi config.*NORMALISED", config=joint)
    refused(["--input", stack, "--norm", cifar], "--norm .*cifar10")
    refused(["--samples", "0"], "--samples 0")
    refused(["--samples", "-2"], "--samples -2")
    refused(["--samples", "3", "--mix-t", "0.3", "--t-from", "given"], "--samples.*--mix-t.*--mmse", config=joint)
    refused(["--samples", "3", "--validate"], "--samples.*--validate")
    refused(["--std-out", "c.tif"], "--std-out.*--samples 2")
    refused(["--std-out", "c.tif", "--samples", "1"], "--std-out.*--samples 2")
    refused(["--input", stack, "--norm", norm, "--out", "b.tif", "--std-out", "c.tif", "--samples", "1"], "--std-out.*--samples 2")
    # the neighbours of those: flags that only mean something next to another one, and unreadable files
    refused(["--std-out", "c.png", "--samples", "2"], "--std-out: a .npy or .tif")
    refused(["--std-out", "c.tif", "--samples", "2", "--validate"], "--validate")
    refused(["--norm", norm], "--norm: only with --input")
    refused(["--input-clip", "100"], "--input-clip: only with --input")
    refused(["--input", stack, "--norm", norm, "--input-clip", "-1"], "--input-clip -1")
    refused(["--save-norm", "x.json"], "--save-norm.*--datapath or --frames")
    refused(["--input", stack, "--norm", norm, "--save-norm", "x.json"], "--save-norm.*--datapath or --frames")
    refused(["--input", stack, "--norm", str(tmp_path / "missing.json")], "--norm .*missing.json")
    refused(["--input", stack, "--norm", norm], "--norm .*target_channel_idx = None, the config says 1",
            config=write_config(tmp_path, "indi", target_channel_idx=1))
    # --mmse keeps its meaning and its refusals
    refused(["--mmse", "2"], "--mmse.*joint_indi")


# ----------------------------------------------------------------------------- entry points: argument validation
def _plan():
    from diffsplitting_amd.data.tiling import TilePlan
    return TilePlan((2, 40, 57), (1, 8, 8), (1, 16, 16))


def test_gather_input_refuses_bad_arguments_without_a_device():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    plan = _plan()
    assert plan.total == 2 * 4 * 7
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every call below is refused
    err = lambda: lib.dsx_last_error().decode()

    def call(p=plan.handle, frames=fake, pix=_lib.PIX_U16, first=0, stride=1, count=4, mean=10.0, std=2.0, clip=-1.0,
             out=fake):
        return lib.dsx_tileplan_gather_input(p, frames, pix, first, stride, count, mean, std, clip, out, None)

    assert call(pix=_lib.PIX_U32) == -1 and "pixel type 2" in err()
    assert call(pix=7) == -1 and "pixel type 7" in err()
    for kw in (dict(p=None), dict(frames=None), dict(out=None)):
        assert call(**kw) == -1 and "null argument" in err(), kw
    for count in (0, -1, 65536):
        assert call(count=count) == -1 and "1..65535" in err(), count
    for kw in (dict(first=-1), dict(first=plan.total), dict(first=plan.total - 3, count=4), dict(first=1, stride=2, count=29),
               dict(stride=0), dict(stride=-1), dict(first=0, stride=2 ** 62, count=3)):
        assert call(**kw) == -1 and "leave the plan (56 tiles)" in err(), kw
    for std in (0.0, -1.0, float("inf"), float("nan")):
        assert call(std=std) == -1 and "std_input must be finite and positive" in err(), std
    assert call(mean=float("nan")) == -1 and "mean_input must be finite" in err()
    assert call(clip=float("nan")) == -1 and "upper_clip is NaN" in err()


def test_moments_refuse_bad_arguments_without_a_device():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    fake = C.c_void_p(0x1000)
    err = lambda: lib.dsx_last_error().decode()
    up = lambda x=fake, mean=fake, m2=fake, count=8, r=0: lib.dsx_moments_update(x, mean, m2, count, r, None)
    fin = lambda mean=fake, m2=fake, count=8, n=2, mo=fake, so=fake: lib.dsx_moments_finish(mean, m2, count, n, mo, so, None)
    for kw in (dict(x=None), dict(mean=None), dict(m2=None)):
        assert up(**kw) == -1 and "moments_update: null argument" in err(), kw
    for count in (0, -5):
        assert up(count=count) == -1 and "count" in err()
        assert fin(count=count) == -1 and "count" in err()
    for r in (-1, 1 << 24):
        assert up(r=r) == -1 and f"r = {r}" in err()
    for kw in (dict(mean=None), dict(m2=None), dict(mo=None)):
        assert fin(**kw) == -1 and "moments_finish: null argument" in err(), kw
    for n in (0, -1, (1 << 24) + 1):
        assert fin(n=n) == -1 and f"n = {n}" in err()


# ----------------------------------------------------------------------------- the dataset's file checks
def test_input_stack_refuses_what_is_not_one_superimposed_stack(tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.input_stack import InputStackTiledPred, read_stack
    from diffsplitting_amd.data.tiff import imwrite
    nd = AWKWARD[1]
    two = str(tmp_path / "two.npy")
    np.save(two, np.zeros((2, 32, 32, 2), np.uint16))
    with pytest.raises(DsxError, match=r"two.npy.*\(N,H,W,2\).*--frames"):
        InputStackTiledPred(two, 16, nd)
    with pytest.raises(DsxError, match=r"\(N,H,W\), got \(32, 32\)"):
        read_stack(np.zeros((32, 32), np.uint8))
    for dt in (np.float64, np.int16, np.uint32):
        with pytest.raises(DsxError, match=f"pixel type {np.dtype(dt)}"):
            read_stack(np.zeros((1, 32, 32), dt))
    with pytest.raises(DsxError, match="unsupported frame file"):
        read_stack(str(tmp_path / "s.png"))
    with pytest.raises(DsxError, match="must provide 'std_input'"):
        InputStackTiledPred(np.zeros((1, 32, 32), np.uint8), 16, {k: v for k, v in nd.items() if k != "std_input"})
    with pytest.raises(DsxError, match="input_clip = -1"):
        InputStackTiledPred(np.zeros((1, 32, 32), np.uint8), 16, nd, input_clip=-1)
    # a .tif keeps its pixel type: what is uploaded is the file's width
    tif = str(tmp_path / "s.tif")
    imwrite(tif, (np.arange(2 * 24 * 40) % 60000).astype(np.uint16).reshape(2, 24, 40))
    back = read_stack(tif)
    assert back.dtype == np.uint16 and back.shape == (2, 24, 40) and back.flags.c_contiguous
