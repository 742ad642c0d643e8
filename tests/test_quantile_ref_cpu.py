"""Posterior quantiles and rank histograms without a GPU: the numpy restatement of dsx_sample_quantiles' contract
(tests/quantile_ref.py) against np.quantile bit for bit and against the typical mistakes; the entry point in the header,
the binding and the library; every refusal of the C entry point on fake pointers; the refusals of
``engine.sample_quantiles``, ``predict_stack``, ``predict_stack_frames`` and ``split`` by message, before any launch and
with no rank started; ``rank_histogram`` and ``interval_coverage`` on a hand-written canvas; the JSON round trip."""
import json
import os
import re

import numpy as np
import pytest
import torch

from diffsplitting_amd import _lib
from diffsplitting_amd._lib import DsxError, check, lib
from diffsplitting_amd.core import calibration as CAL
from tests import quantile_ref as REF
from tests.bits import same_bits
from tests.host_checks import cpu_samplers, tile_plan
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = (0.0, 0.01, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.8, 0.975, 1.0)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", range(1, 65))
def test_the_restatement_is_np_quantile_bit_for_bit(n):
    x, _ = REF.stack(n, 257, seed=1)
    assert not (np.signbit(x) & (x == 0)).any()                     # no -0: np.sort leaves the order of the zeros open
    want = np.quantile(x.astype(np.float64), NINE, axis=0).astype(np.float32)
    assert same_bits(REF.quantiles(x, NINE), want)


def test_the_integer_image_orders_minus_zero_before_plus_zero():
    x = np.array([[0.0], [-0.0], [1.0], [-1.0], [-0.0]], dtype=np.float32)
    v = REF.sort_samples(x)[:, 0]
    assert v.tolist() == [-1.0, 0.0, 0.0, 0.0, 1.0] and np.signbit(v).tolist() == [True, True, True, False, False]
    assert REF.ranks(x, np.array([0.0], dtype=np.float32)).tolist() == [1.0]       # -0 < +0 is false on fp32 values
    # the order of the zeros shows in the sign: v[1] = v[2] = -0 give b - d (1 - t) = -0 - (+0) = -0 at position 1.5;
    # at position 2 (t = 0) a + d t = -0 + (+0) = +0, and v[3] = +0 at position 3
    q = REF.quantiles(x, (0.375, 0.5, 0.75))[:, 0]
    assert (q == 0).all() and np.signbit(q).tolist() == [True, False, False]


@pytest.mark.parametrize("n", [2, 3, 7, 33, 64])
def test_the_restatement_rejects_the_typical_mistakes(n):
    x, t = REF.stack(n, 1031, seed=2)
    want = REF.quantiles(x, REF.Q6)
    for which in ("lerp32", "padded_pos", "last_unsorted"):
        if which == "padded_pos" and n & (n - 1) == 0:
            continue                                                # n is its own padded length
        assert not same_bits(REF.mistaken(x, REF.Q6, which), want), which
    xt, tt = REF.tied(n, 1031, seed=2)
    assert (xt == tt[None]).any()
    le, lt = REF.ranks_le(xt, tt), REF.ranks(xt, tt)
    assert (le >= lt).all() and (le > lt).any()
    assert lt.min() >= 0 and lt.max() <= n and np.array_equal(lt, np.round(lt))


def test_the_witnesses_tell_a_fused_or_single_branch_lerp_from_the_contract():
    """A one-ulp difference in double shows after the cast to fp32 only next to a rounding boundary of fp32: random
    inputs do not find one, tests/quantile_ref.py constructs them (the GPU test runs the same inputs)."""
    assert set(REF.MISTAKES) == {"lerp32", "padded_pos", "last_unsorted", "fma", "single_branch"}
    x = REF.witnesses(1031)
    want = REF.quantiles(x, REF.WITNESS_Q)
    assert same_bits(want, np.quantile(x.astype(np.float64), REF.WITNESS_Q, axis=0).astype(np.float32))
    fma, single = REF.mistaken(x, REF.WITNESS_Q, "fma"), REF.mistaken(x, REF.WITNESS_Q, "single_branch")
    share = lambda bad, k: float((bad[k] != want[k]).mean())
    shares = (share(fma, 0), share(single, 1), share(single, 0))
    assert shares[0] > 0.2 and shares[1] > 0.2 and shares[2] == 0.0, \
        (f"share of differing elements: fma at t < 0.5 {shares[0]:.3f}, single branch at t >= 0.5 {shares[1]:.3f} and at "
         f"t < 0.5 {shares[2]:.3f}")


# ----------------------------------------------------------------------------- the entry point
def test_the_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    name = "dsx_sample_quantiles"
    assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/dsx.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 10, f"{name} is not bound in _lib.py"
    assert hasattr(_lib._cdll, name), f"{name} is not exported by libdsx.so"
    assert callable(getattr(lib, name))
    srcs = open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "build.sh")).read()
    assert "dsx_quantiles.hip" in srcs and "dsx_quantiles.cpp" in srcs
    assert lib.dsx_abi_version() == 2 and re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", hdr)


def test_every_refusal_comes_before_any_device_work():
    """Addresses that are never dereferenced stand in for device memory: a call that got past its checks would launch."""
    X, OUT, T, R = 1 << 20, 1 << 24, 1 << 25, 1 << 26              # far apart: nothing overlaps unless a case says so
    q = np.array([0.1, 0.5])

    def refused(match, x=X, stride=100, n=3, count=100, qq=q, nq=2, out=OUT, target=T, rank=R):
        with pytest.raises(DsxError, match=match):
            check(lib.dsx_sample_quantiles(x, stride, n, count, qq, nq, out, target, rank, None))

    refused("sample_quantiles: x_dev is NULL", x=None)
    refused(r"n = 0 samples, must be in 1\.\.64", n=0)
    refused(r"n = 65 samples, must be in 1\.\.64", n=65)
    refused(r"nq = -1 quantiles, must be in 0\.\.8", nq=-1)
    refused(r"nq = 9 quantiles, must be in 0\.\.8", nq=9)
    refused("nq = 0 and no rank output", nq=0, target=None, rank=None)
    refused("nq = 0 and no rank output", nq=0, qq=None, out=None, target=None, rank=None)
    refused("nq = 2 needs q_host and out_dev", out=None)
    refused("nq = 2 needs q_host and out_dev", qq=None)
    refused("count = 0 elements, must be at least 1", count=0)
    refused("count = -5 elements, must be at least 1", count=-5)
    refused("sample_stride = 99 is below count = 100", stride=99)
    refused(r"q\[1\] = 1\.5, must be finite and in \[0, 1\]", qq=np.array([0.1, 1.5]))
    refused(r"q\[0\] = -0\.1, must be finite and in \[0, 1\]", qq=np.array([-0.1, 0.5]))
    refused(r"q\[0\] = (nan|-nan), must be finite", qq=np.array([np.nan, 0.5]))
    refused(r"q\[1\] = inf, must be finite", qq=np.array([0.5, np.inf]))
    refused("target_dev and rank_dev are given together, or neither", target=None)
    refused("target_dev and rank_dev are given together, or neither", rank=None)
    # the samples span [X, X + 4 * (2 * 120 + 100)) bytes with stride 120: the gaps belong to the range too
    span = 4 * (2 * 120 + 100)
    refused("out_dev overlaps the samples", stride=120, out=X + span - 4)
    refused("out_dev overlaps the samples", stride=120, out=X - 4 * 200 + 4)
    refused("out_dev overlaps the samples", stride=120, out=X + 4 * 105)
    refused("rank_dev overlaps the samples", stride=120, rank=X + span - 4)
    refused("rank_dev overlaps the samples", stride=120, rank=X - 4 * 100 + 4)
    refused("rank_dev overlaps the samples", stride=120, nq=0, qq=None, out=None, rank=X)


def test_sample_quantiles_refuses_what_is_no_cuda_fp32_stack():
    from diffsplitting_amd import engine
    with pytest.raises(DsxError, match="stack must be a CUDA tensor"):
        engine.sample_quantiles(torch.zeros(3, 8), (0.5,))
    with pytest.raises(DsxError, match="stack must be a CUDA tensor"):
        engine.sample_quantiles(np.zeros((3, 8), np.float32), (0.5,))


# ----------------------------------------------------------------------------- the drivers' refusals, no launch
def _stands_in(monkeypatch):
    from diffsplitting_amd import engine, parallel
    from diffsplitting_amd.data import tile_predict

    def touched(*a, **k):
        raise AssertionError("the refusal came too late")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(tile_predict, "TileExchange", touched)
    monkeypatch.setattr(parallel, "all_gather_flat", touched)
    monkeypatch.setattr(engine, "sample_quantiles", touched)
    monkeypatch.setattr(engine, "moments_update", touched)
    monkeypatch.setattr(engine, "randn_samples", touched)

    class Stack:                                                     # an input-only stack: no ground truth
        plan = tile_plan((2, 40, 57), 32, 16)
        device = "cpu"

        def tiles(self, ids):
            touched()

    class Scored(Stack):                                             # a ground truth of the prediction's two channels
        def normalized_target_frames(self):
            return torch.zeros(2, 40, 57, 2)

    class Other(Stack):                                              # a ground truth of other channels
        def normalized_target_frames(self):
            return torch.zeros(2, 40, 57, 3)
    return Stack, Scored, Other


def test_predict_stack_refuses_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd.data.tiled_predict import predict_stack
    Stack, Scored, Other = _stands_in(monkeypatch)
    g, i, _ = cpu_samplers()
    what = "predict_stack: "
    for kw, match in ((dict(quantiles=(0.5,)), "quantiles= and ranks= .*samples = 1, give 2 or more"),
                      (dict(ranks=True), "quantiles= and ranks= .*samples = 1, give 2 or more"),
                      (dict(quantiles=(0.5,), samples=65), "quantiles= and ranks= sort the samples in registers: samples = 65, "
                                                           "at most 64"),
                      (dict(quantiles=(0.5, 1.5), samples=3), r"quantiles = \(0\.5, 1\.5\): 1 to 8 numbers in \[0, 1\]"),
                      (dict(quantiles=(), samples=3), r"quantiles = \(\): 1 to 8 numbers"),
                      (dict(quantiles=(float("nan"),), samples=3), ".*1 to 8 numbers"),
                      (dict(quantiles=tuple(k / 8 for k in range(9)), samples=3), ".*1 to 8 numbers"),
                      (dict(quantiles="half", samples=3), ".*1 to 8 numbers"),
                      (dict(ranks=True, samples=3, stitch="blend"), "ranks=True with stitch='blend': a blend of per-tile "
                                                                    "ranks is not a rank"),
                      (dict(ranks=True, samples=3), "ranks=True: the dataset holds no ground truth")):
        for smp in (g, i):
            with pytest.raises(DsxError, match=what + match):
                predict_stack(smp, Scored() if "blend" in match else Stack(), **kw)
    with pytest.raises(DsxError, match=what + "ranks=True: the dataset holds no ground truth with the prediction's"):
        predict_stack(i, Other(), ranks=True, samples=3)
    # per-step frame fusion keeps the states: quantile_bytes, and the same refusals
    fuse = dict(solver=dict(solver="ddim", steps=4, eta=0.0, spacing=None), noise="field", seed=3, fuse=True)
    need = 3 * 2 * 40 * 57 * 2 * 4
    for kw in (dict(quantiles=(0.5,)), dict(ranks=True)):
        with pytest.raises(DsxError, match=what + f"quantiles= / ranks= keep the 3 frame states .*{need} bytes, "
                                                  f"quantile_bytes = {need - 1}"):
            predict_stack(g, Scored(), samples=3, quantile_bytes=need - 1, **fuse, **kw)
    with pytest.raises(DsxError, match=what + "quantiles= and ranks= .*samples = 1"):
        predict_stack(g, Scored(), quantiles=(0.5,), **fuse)
    with pytest.raises(DsxError, match=what + "ranks=True: the dataset holds no ground truth"):
        predict_stack(g, Stack(), ranks=True, samples=2, **fuse)


def test_predict_stack_frames_refuses_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd.data.tiled_predict import predict_stack_frames
    Stack, Scored, _ = _stands_in(monkeypatch)
    _, i, j = cpu_samplers()
    what = "predict_stack_frames: "
    need = 2 * 2 * 40 * 57 * 2 * 4
    for smp in (i, j):
        with pytest.raises(DsxError, match=what + "quantiles= and ranks= .*samples = 1, give 2 or more"):
            predict_stack_frames(smp, Scored(), seed=3, quantiles=(0.5,))
        with pytest.raises(DsxError, match=what + "quantiles= and ranks= .*samples = 1, give 2 or more"):
            predict_stack_frames(smp, Scored(), seed=3, ranks=True)
        with pytest.raises(DsxError, match=what + "quantiles= and ranks= .*samples = 65, at most 64"):
            predict_stack_frames(smp, Scored(), seed=3, ranks=True, samples=65)
        with pytest.raises(DsxError, match=what + r"quantiles = \[2\]: 1 to 8 numbers in \[0, 1\]"):
            predict_stack_frames(smp, Scored(), seed=3, quantiles=[2], samples=2)
        with pytest.raises(DsxError, match=what + "ranks=True: the dataset holds no ground truth"):
            predict_stack_frames(smp, Stack(), seed=3, ranks=True, samples=2)
        with pytest.raises(DsxError, match=what + f".*keep the 2 frame states of 2 x 40 x 57 x 2: {need} bytes, "
                                                  f"quantile_bytes = {need - 1}"):
            predict_stack_frames(smp, Scored(), seed=3, quantiles=(0.1, 0.9), samples=2, quantile_bytes=need - 1)


# ----------------------------------------------------------------------------- rank histogram
def test_rank_histogram_and_interval_coverage_on_a_hand_written_canvas():
    # 2 x 2 x 2 pixels of two channels, n = 4 samples: channel 0 holds every rank but 3, channel 1 only the extremes
    rank = torch.tensor([[[[0., 0.], [1., 4.]], [[2., 4.], [4., 0.]]],
                         [[[2., 0.], [2., 4.]], [[1., 4.], [0., 0.]]]])
    hist = CAL.rank_histogram(rank, 4)
    assert hist.dtype == np.int64 and hist.tolist() == [[2, 2, 3, 0, 1], [4, 0, 0, 0, 4]]
    assert np.array_equal(CAL.rank_histogram(rank.numpy(), 4), hist)
    cov = CAL.interval_coverage(hist)
    assert cov.m.tolist() == [1, 2] and cov.nominal.tolist() == [3 / 5, 1 / 5] and (cov.pixels, cov.samples) == (8, 4)
    assert cov.observed.tolist() == [[5 / 8, 3 / 8], [0.0, 0.0]]
    odd = CAL.interval_coverage(np.array([[1, 2, 3, 4]]))           # n = 3: one band, between the extremes
    assert odd.m.tolist() == [1] and odd.nominal.tolist() == [0.5] and odd.observed.tolist() == [[0.5]]
    for bad, n in ((torch.tensor([[0.5]]), 4), (torch.tensor([[5.0]]), 4), (torch.tensor([[-1.0]]), 4)):
        with pytest.raises(DsxError, match=r"rank_histogram: every rank must be an integer in 0\.\.4"):
            CAL.rank_histogram(bad, n)
    with pytest.raises(DsxError, match="rank_histogram: n = 0"):
        CAL.rank_histogram(rank, 0)
    with pytest.raises(DsxError, match="interval_coverage: every channel must hold the same positive pixel count"):
        CAL.interval_coverage(np.array([[1, 2, 3], [1, 2, 4]]))
    with pytest.raises(DsxError, match=r"interval_coverage: a histogram \(C, n \+ 1\)"):
        CAL.interval_coverage(np.array([1, 2, 3]))


def test_the_rank_histogram_file_round_trips(tmp_path):
    hist = np.array([[2, 2, 3, 0, 1], [4, 0, 0, 0, 4]], dtype=np.int64)
    path = str(tmp_path / "h.json")
    CAL.save_rank_histogram(path, hist)
    doc = json.load(open(path))
    assert set(doc) == {"format", "version", "channels", "samples", "pixels", "hist", "intervals"}
    assert (doc["format"], doc["version"], doc["channels"], doc["samples"], doc["pixels"]) == \
        ("diffsplitting_amd.rank_histogram", 1, 2, 4, 8)
    assert doc["hist"] == hist.tolist()
    assert doc["intervals"] == [{"m": 1, "nominal": 3 / 5, "observed": [5 / 8, 0.0]},
                                {"m": 2, "nominal": 1 / 5, "observed": [3 / 8, 0.0]}]
    back = CAL.load_rank_histogram(path)
    assert back.dtype == np.int64 and np.array_equal(back, hist)
    (tmp_path / "text.json").write_text("not json")
    with pytest.raises(DsxError, match="not a rank histogram file"):
        CAL.load_rank_histogram(str(tmp_path / "text.json"))
    for change, match in ((dict(format="other"), "format 'other'"), (dict(version=2), "version 2"),
                          (dict(pixels=9), "not a complete rank histogram file"),
                          (dict(hist=[[1, 2]]), "not a complete rank histogram file")):
        (tmp_path / "bad.json").write_text(json.dumps(dict(doc, **change)))
        with pytest.raises(DsxError, match=match):
            CAL.load_rank_histogram(str(tmp_path / "bad.json"))


# ----------------------------------------------------------------------------- command line
def test_split_refuses_the_quantile_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    """Every refusal is a SystemExit that names the flag, raised on the command line and the config alone: no rank is
    started and nothing touches the device."""
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    indi, joint, sr3 = (write_config(tmp_path, w) for w in ("indi", "joint_indi", "sr3"))
    colour = write_config(tmp_path, "indi", train={"name": "cifar10", "batch_size": 3, "datapath": "none"},
                          val={"name": "cifar10", "datapath": "none"})
    qo, rh = str(tmp_path / "q.npy"), str(tmp_path / "h.json")
    Q = ["--quantiles", "0.05,0.5,0.95", "--quantile-out", qo]
    H = ["--rank-histogram", rh]

    def refused(argv, match, config=indi):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", config] + argv)

    refused(Q, "--quantile-out: .*--samples 2 or more")
    refused(Q + ["--samples", "1"], "--quantile-out: .*--samples 2 or more")
    refused(H, "--rank-histogram: .*--samples 2 or more")
    refused(Q + ["--samples", "65"], "--quantile-out: .*--samples 65, at most 64")
    refused(H + ["--samples", "65"], "--rank-histogram: .*--samples 65, at most 64")
    refused(["--quantile-out", qo, "--samples", "3"], "--quantile-out: give --quantiles")
    refused(["--quantiles", "0.5", "--samples", "3"], "--quantiles: give --quantile-out FILE")
    refused(H + ["--samples", "3", "--input", "stack.tif", "--norm", "n.json"], "--rank-histogram with --input.*no ground truth")
    refused(H + ["--samples", "3", "--stitch", "blend"], "--rank-histogram with --stitch blend: a blend of per-tile ranks")
    refused(Q + ["--samples", "3", "--validate"], "--quantile-out .*not with --validate")
    refused(H + ["--samples", "3", "--validate"], "--rank-histogram .*not with --validate")
    refused(Q + ["--samples", "3", "--mix-t", "0.3"], "--quantile-out: not with --mix-t", config=joint)
    refused(H + ["--samples", "3", "--mix-t", "0.3"], "--rank-histogram: not with --mix-t", config=joint)
    refused(Q + ["--samples", "3", "--datapath"], "--quantile-out .*colour items", config=colour)
    refused(H + ["--samples", "3", "--datapath"], "--rank-histogram .*colour items", config=colour)
    refused(["--quantiles", "0.5", "--quantile-out", str(tmp_path / "q.png"), "--samples", "3"], "--quantile-out .*q.png: a .npy or .tif file")
    refused(["--rank-histogram", str(tmp_path / "h.txt"), "--samples", "3"], "--rank-histogram .*h.txt: a .json file")
    for bad in ("1.5", "0.5,-0.1", "a,b", "0.5,", ",".join(["0.5"] * 9), "nan"):
        refused(["--quantiles", bad, "--quantile-out", qo, "--samples", "3"], "--quantiles .*1 to 8 comma-separated numbers")
    assert not os.path.exists(qo) and not os.path.exists(rh)
    # where the flags apply the checks pass: the run gets as far as starting (the stand-in above)
    seeded = ["--sample-seed", "3"]
    for argv, config in ((Q + ["--samples", "2"], indi), (Q + H + ["--samples", "64"], indi),
                         (Q + ["--samples", "3", "--stitch", "blend"], indi),
                         (H + ["--samples", "3", "--frame-steps"] + seeded, indi),
                         (H + ["--samples", "3", "--stitch", "blend", "--frame-steps"] + seeded, joint),
                         (Q + H + ["--samples", "3", "--solver", "ddim", "--solver-steps", "4", "--noise-field", "--fuse-steps"]
                          + seeded, sr3)):
        with pytest.raises(AssertionError, match="a rank was started"):
            split.main(["-c", config] + argv)
