"""Posterior quantiles and ranks on the MI355X (`-m gpu`): dsx_sample_quantiles bit for bit against the numpy
restatement of its contract (tests/quantile_ref.py) for every n in 1..64 on both load paths, ragged counts, a strided
stack inside NaN-filled memory with canaries around both outputs, an unaligned base, heavily tied inputs with both
zeros, the constructed witnesses of a fused or single-branch lerp, nq = 8 and ranks alone; then ``predict_stack`` and
``predict_stack_frames`` with ``quantiles=`` / ``ranks=`` against their restatements, and one ``split`` run.

The cap.  The launch goes through grid_for (dsx_kernels.h): 4096 workgroups of 256 threads, each thread one group of
elements per trip.  On the 4-byte path a group is one element: the loop repeats from 2^20 elements on; on the wide path
a group is four elements up to n = 32 (two beyond): from 2^22 elements on.  test_past_the_grid_cap crosses both at
n = 3, with count = (elements of the first trip) + 4099 on the 4-byte path and + 4100 (a multiple of four) on the
wide one; every other count here stays inside the first trip."""
import json

import numpy as np
import pytest
import torch

from tests import nets
from tests import quantile_ref as REF
from tests import tiled_util as T
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CAP = 4096 * 256                          # groups of the first trip of a grid_for launch


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(x, q, t=None, stack=None):
    """the call on ``x`` (n, count) -- or on the device tensor ``stack`` that holds it -- against the restatement"""
    from diffsplitting_amd import engine
    got_q, got_r = engine.sample_quantiles(_dev(x) if stack is None else stack, q, _dev(t))
    if q is not None and len(q):
        assert got_q.shape == (len(q),) + x.shape[1:] and same_bits(got_q.cpu().numpy(), REF.quantiles(x, q))
    else:
        assert got_q is None
    if t is not None:
        assert got_r.shape == x.shape[1:] and same_bits(got_r.cpu().numpy(), REF.ranks(x, t))
    else:
        assert got_r is None
    return got_q, got_r


# ----------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("n", range(1, 65))
def test_every_sample_count_is_its_restatement(n):
    """count 1031 (odd: the 4-byte path) and 1032 (the wide path): every padding of every network on either path"""
    for count in (1031, 1032):
        x, t = REF.stack(n, count, seed=3)
        _check(x, REF.Q6, t)


@pytest.mark.parametrize("n", [7, 64])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_ragged_counts(n, count):
    x, t = REF.stack(n, count, seed=4)
    _check(x, REF.Q6, t)


def test_a_strided_stack_between_nans_and_canaries():
    """sample_stride = count + 5 with NaN in the gaps; both outputs inside canary-filled buffers, through the C entry
    point itself; everything around the outputs and the whole input stay as they were"""
    from diffsplitting_amd._lib import check, lib
    n, count, pad, q = 7, 1031, 64, np.array(REF.Q6)
    x, t = REF.stack(n, count, seed=5)
    for off in (0, 1):                                               # an aligned base and one 4 bytes off
        buf = torch.full((off + n * (count + 5),), float("nan"), device="cuda")
        view = buf[off:].view(n, count + 5)[:, :count]
        view.copy_(_dev(x))
        before = buf.clone()
        _check(x, REF.Q6, t, stack=view)                             # the Python face takes the view as it is
        out = torch.full((pad + len(q) * count + pad,), -7.25, device="cuda")
        rank = torch.full((pad + count + pad,), -7.25, device="cuda")
        tgt = _dev(t)
        check(lib.dsx_sample_quantiles(view.data_ptr(), count + 5, n, count, q, len(q), out.data_ptr() + 4 * pad, tgt,
                                       rank.data_ptr() + 4 * pad, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert same_bits(buf, before)
        assert same_bits(out[pad:-pad].view(len(q), count).cpu().numpy(), REF.quantiles(x, REF.Q6))
        assert same_bits(rank[pad:-pad].cpu().numpy(), REF.ranks(x, t))
        for edge in (out[:pad], out[-pad:], rank[:pad], rank[-pad:]):
            assert bool((edge == -7.25).all())


@pytest.mark.parametrize("n", [3, 16, 33, 64])
def test_the_load_path_does_not_change_the_bits(n):
    """the same samples one element off a 16-byte boundary (4-byte loads) and on an aligned copy (wide loads)"""
    from diffsplitting_amd import engine
    count = 1032
    x, t = REF.stack(n, count, seed=6)
    big = torch.empty(n * count + 1, device="cuda")
    off = big[1:].view(n, count)
    off.copy_(_dev(x))
    assert off.data_ptr() % 16 == 4 and _dev(x).data_ptr() % 16 == 0
    a_q, a_r = _check(x, REF.Q6, t)
    o_q, o_r = _check(x, REF.Q6, t, stack=off)
    assert same_bits(a_q, o_q) and same_bits(a_r, o_r)
    s_q, _ = engine.sample_quantiles(torch.cat([_dev(x), torch.zeros(n, 4, device="cuda")], dim=1)[:, :count], REF.Q6)
    assert same_bits(a_q, s_q)                                       # another stride, still wide


@pytest.mark.parametrize("n", [2, 5, 8, 31, 64])
def test_heavily_tied_inputs_with_both_zeros(n):
    for count in (1031, 1032):
        x, t = REF.tied(n, count, seed=7)
        zero = x == 0
        assert (np.signbit(x) & zero).any() and (~np.signbit(x) & zero).any() and (x == t[None]).any()
        _, rank = _check(x, REF.Q6, t)
        assert not same_bits(rank.cpu().numpy(), REF.ranks_le(x, t))


def test_the_witnesses_of_a_fused_or_single_branch_lerp():
    """inputs on which an fma or the single-branch lerp changes the fp32 result (tests/quantile_ref.py constructs them,
    tests/test_quantile_ref_cpu.py shows that they do)"""
    for count in (1031, 1032):
        x = REF.witnesses(count)
        got, _ = _check(x, REF.WITNESS_Q)
        for which in ("fma", "single_branch"):
            assert not same_bits(got.cpu().numpy(), REF.mistaken(x, REF.WITNESS_Q, which)), which


def test_eight_quantiles_and_ranks_alone():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    x, t = REF.stack(13, 515, seed=8)
    _check(x, REF.Q8, t)
    _check(x, REF.Q8)
    _check(x, None, t)
    _check(x, (), t)
    shaped = x.reshape(13, 5, 103)                                   # any trailing shape
    got_q, got_r = engine.sample_quantiles(_dev(shaped), (0.5,), _dev(t.reshape(5, 103)))
    assert got_q.shape == (1, 5, 103) and got_r.shape == (5, 103)
    assert same_bits(got_q.cpu().numpy().reshape(1, 515), REF.quantiles(x, (0.5,)))
    with pytest.raises(DsxError, match="nq = 0 and no rank output"):
        engine.sample_quantiles(_dev(x), None)
    with pytest.raises(DsxError, match=r"nq = 9 quantiles, must be in 0\.\.8"):
        engine.sample_quantiles(_dev(x), np.linspace(0, 1, 9))
    with pytest.raises(DsxError, match=r"n = 65 samples, must be in 1\.\.64"):
        engine.sample_quantiles(torch.zeros(65, 8, device="cuda"), (0.5,))
    with pytest.raises(DsxError, match=r"q\[0\] = 1\.5"):
        engine.sample_quantiles(_dev(x), (1.5,))


def test_python_refusals():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    x = torch.zeros(3, 8, device="cuda")
    with pytest.raises(DsxError, match="stack must be a CUDA tensor"):
        engine.sample_quantiles(x.cpu(), (0.5,))
    with pytest.raises(DsxError, match="target must be a CUDA tensor"):
        engine.sample_quantiles(x, (0.5,), torch.zeros(8))
    with pytest.raises(DsxError, match=r"target must be \(8,\), got \(7,\)"):
        engine.sample_quantiles(x, (0.5,), torch.zeros(7, device="cuda"))
    with pytest.raises(DsxError, match="stack must be a non-empty float32 tensor"):
        engine.sample_quantiles(x.double(), (0.5,))
    with pytest.raises(DsxError, match="stack must hold contiguous samples"):
        engine.sample_quantiles(torch.zeros(3, 8, 2, device="cuda")[:, :, 0], (0.5,))
    with pytest.raises(DsxError, match="stack must hold contiguous samples"):
        engine.sample_quantiles(torch.zeros(8, 3, device="cuda").t(), (0.5,))


@pytest.mark.parametrize("path", ["4-byte", "wide"])
def test_past_the_grid_cap(path):
    """the second trip of the grid-stride loop at n = 3, with a ragged tail inside it"""
    n = 3
    count = CAP + 4099 if path == "4-byte" else 4 * CAP + 4100
    assert (count % 4 == 0) == (path == "wide")
    rng = np.random.default_rng(9)
    x, t = rng.standard_normal((n, count)).astype(np.float32), rng.standard_normal(count).astype(np.float32)
    _check(x, (0.0, 0.5, 0.9), t)


# ----------------------------------------------------------------------------- 2. predict_stack
SHAPE, PATCH, GRID, BATCH, STEPS, SEED, SAMPLES, Q3 = (3, 96, 160), 64, 32, 4, 2, 11, 5, (0.1, 0.5, 1.0)


def _hagen64():
    from diffsplitting_amd.model import networks
    from tests.util import golden_state_dict
    sd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()})
    assert netG.e == 0.01                                            # the sampler's own noise scale: the draws matter
    return netG


def _restated_maps(netG, dataset, q, gt=None):
    """The quantile (and rank) canvases from the draws restated tile batch by tile batch: ``inference`` with the sample
    ids ``k + r * total``, ``engine.sample_quantiles`` on the stacked draws -- held against the numpy restatement on the
    way --, one crop-paste per map."""
    from diffsplitting_amd import engine
    plan = dataset.plan
    quants, ranks = [], []
    for i in range(0, plan.total, BATCH):
        chunk = list(range(i, i + BATCH))
        x = dataset.tiles(chunk)["input"]
        draws = []
        for r in range(SAMPLES):
            netG.inference(x, continuous=False, num_timesteps=STEPS, seed=SEED, sample_ids=[k + r * plan.total for k in chunk])
            draws.append(netG.last_full_batch.clone())
        st = torch.stack(draws)
        tgt = plan.gather_canvas(gt, chunk) if gt is not None else None
        qt, rk = engine.sample_quantiles(st, q, tgt)
        host = st.cpu().numpy()
        assert same_bits(qt.cpu().numpy(), REF.quantiles(host, q))
        quants.append(qt)
        if gt is not None:
            assert same_bits(rk.cpu().numpy(), REF.ranks(host, tgt.cpu().numpy()))
            ranks.append(rk)
    want_q = torch.stack([plan.stitch(torch.cat([b[k] for b in quants])) for k in range(len(q))])
    return want_q, (plan.stitch(torch.cat(ranks)) if gt is not None else None)


def test_predict_stack_quantiles_on_an_input_only_stack():
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG = _hagen64()
    s = np.random.default_rng(5).integers(0, 6000, SHAPE).astype(np.uint16)
    nd = dict(mean_input=np.float64(3000.0), std_input=np.float64(1700.0), mean_target=np.array([1500.0, 1500.0]),
              std_target=np.array([850.0, 850.0]), target0_max=None, target1_max=None, input_max=None)
    stack = InputStackTiledPred(s, PATCH, nd, grid_size=GRID)
    assert stack.plan.total == 24
    kw = dict(batch_tiles=BATCH, num_timesteps=STEPS, samples=SAMPLES, return_std=True, seed=SEED)
    plain, _ = predict_stack(netG, stack, **kw)
    got, _ = predict_stack(netG, stack, quantiles=Q3, **kw)
    assert set(plain) == {"mean", "std"} and set(got) == {"mean", "std", "quantiles"}
    assert same_bits(got["mean"], plain["mean"]) and same_bits(got["std"], plain["std"]) and bool((got["std"] > 0).any())
    want, _ = _restated_maps(netG, stack, Q3)
    assert got["quantiles"].shape == (3,) + SHAPE + (2,) and same_bits(got["quantiles"], want)
    assert bool((got["quantiles"][0] <= got["quantiles"][1]).all()) and bool((got["quantiles"][1] <= got["quantiles"][2]).all())
    assert bool((got["quantiles"][0] < got["quantiles"][2]).any())
    # a blend of per-tile quantiles where the docstring says so, and ranks refused there
    from diffsplitting_amd._lib import DsxError
    blend, _ = predict_stack(netG, stack, quantiles=(0.5,), stitch="blend", **kw)
    assert blend["quantiles"].shape == (1,) + SHAPE + (2,) and bool(torch.isfinite(blend["quantiles"]).all())
    with pytest.raises(DsxError, match="ranks=True: the dataset holds no ground truth"):
        predict_stack(netG, stack, ranks=True, **kw)


def _two_channels(shape, patch, grid, seed=21):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    rng = np.random.default_rng(seed)
    c0, c1 = (rng.integers(0, 3000, shape).astype(np.float32) for _ in range(2))
    return SplitDatasetTiledPred("Hagen", DataLocation(arrays=(c0, c1)), patch, grid_size=grid, max_qval=0.98,
                                 channel_weights=[1, 1])


def test_predict_stack_quantiles_and_ranks_against_ground_truth():
    from diffsplitting_amd.core.calibration import interval_coverage, rank_histogram
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG, two = _hagen64(), _two_channels(SHAPE, PATCH, GRID)
    kw = dict(batch_tiles=BATCH, num_timesteps=STEPS, samples=SAMPLES, return_std=True, seed=SEED)
    plain, _ = predict_stack(netG, two, **kw)
    got, _ = predict_stack(netG, two, quantiles=Q3, ranks=True, **kw)
    assert set(got) == {"mean", "std", "psnr", "quantiles", "rank"}
    for k in ("mean", "std", "psnr"):
        assert same_bits(got[k], plain[k]), k
    gt = two.normalized_target_frames()
    want_q, want_r = _restated_maps(netG, two, Q3, gt)
    assert same_bits(got["quantiles"], want_q) and same_bits(got["rank"], want_r)
    ranks_only, _ = predict_stack(netG, two, ranks=True, **kw)
    assert "quantiles" not in ranks_only and same_bits(ranks_only["rank"], want_r)
    hist = rank_histogram(got["rank"], SAMPLES)
    pixels = SHAPE[0] * SHAPE[1] * SHAPE[2]
    assert hist.shape == (2, SAMPLES + 1) and (hist.sum(axis=1) == pixels).all()
    cov = interval_coverage(hist)
    assert cov.pixels == pixels and cov.m.tolist() == [1, 2] and cov.nominal.tolist() == [4 / 6, 2 / 6]
    # the rank says where the target lies among the order statistics
    r, q = got["rank"], got["quantiles"]
    assert bool((gt[r == SAMPLES] > q[2][r == SAMPLES]).all()) and bool((gt[r < SAMPLES] <= q[2][r < SAMPLES]).all())


# ----------------------------------------------------------------------------- 3. frame states
FOURS = [(list(range(i, i + 4)), 4) for i in (0, 4, 8)]


def test_predict_stack_frames_quantiles_and_ranks_are_exact_per_pixel():
    """three posterior samples of frame diffusion: the median and the rank against the restated frame states"""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiled_predict import predict_stack_frames
    netG, two = T.indi(), _two_channels((2, 40, 57), 32, 16)
    assert two.plan.total == 12
    kw = dict(batch_tiles=4, num_timesteps=3, seed=T.SEED, samples=3, return_std=True)
    plain, _ = predict_stack_frames(netG, two, **kw)
    got, _ = predict_stack_frames(netG, two, quantiles=(0.5,), ranks=True, **kw)
    assert set(got) == set(plain) | {"quantiles", "rank"}
    for k in plain:
        assert same_bits(got[k], plain[k]), k
    states = np.stack([T.restated_frames(netG, two, 3, FOURS, r=r) for r in range(3)])
    gt = two.normalized_target_frames().cpu().numpy()
    assert got["quantiles"].shape == (1, 2, 40, 57, 2)
    assert same_bits(got["quantiles"].cpu().numpy(), REF.quantiles(states, (0.5,)))
    assert same_bits(got["rank"].cpu().numpy(), REF.ranks(states, gt))
    need = 3 * 2 * 40 * 57 * 2 * 4
    with pytest.raises(DsxError, match=f"{need} bytes, quantile_bytes = {need - 1}"):
        predict_stack_frames(netG, two, quantiles=(0.5,), quantile_bytes=need - 1, **kw)


# ----------------------------------------------------------------------------- 4. split
def test_split_writes_quantile_maps_and_the_rank_histogram(tmp_path):
    from diffsplitting_amd import split
    cfg = {"name": "tiny_q", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 64, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 1],
                        "train": {"name": "Hagen"}, "val": {"name": "Hagen"}},
           "model": nets.hagen64_section()}
    p = lambda name: str(tmp_path / name)
    with open(p("tiny.json"), "w") as f:
        json.dump(cfg, f)
    torch.manual_seed(1234)                                          # the model's random initial weights
    split.main(["-c", p("tiny.json"), "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--synthetic", "1,64,96",
                "--steps", "2", "--batch-tiles", "4", "--sample-seed", "11", "--samples", "3", "--quantiles", "0,0.5,1",
                "--quantile-out", p("x.npy"), "--rank-histogram", p("h.json"), "--out", p("mean.npy")])
    x = np.load(p("x.npy"))
    assert x.dtype == np.float32 and x.shape == (3, 1, 64, 96, 2) and np.isfinite(x).all()
    assert (x[0] <= x[1]).all() and (x[1] <= x[2]).all() and (x[0] < x[2]).any()      # the median between min and max
    mean = np.load(p("mean.npy"))
    assert mean.shape == x.shape[1:] and (x[0] <= mean + 1e-3 * np.abs(mean)).all() and (mean <= x[2] + 1e-3 * np.abs(mean)).all()
    doc = json.load(open(p("h.json")))
    assert set(doc) == {"format", "version", "channels", "samples", "pixels", "hist", "intervals"}
    assert (doc["format"], doc["version"], doc["channels"], doc["samples"], doc["pixels"]) == \
        ("diffsplitting_amd.rank_histogram", 1, 2, 3, 64 * 96)
    hist = np.array(doc["hist"])
    assert hist.shape == (2, 4) and (hist.sum(axis=1) == 64 * 96).all() and (hist >= 0).all()
    assert [iv["m"] for iv in doc["intervals"]] == [1] and doc["intervals"][0]["nominal"] == 0.5
    assert doc["intervals"][0]["observed"] == [float(hist[c, 1:3].sum()) / (64 * 96) for c in range(2)]
