"""Input-only stacks on the device (`-m gpu`): dsx_tileplan_gather_input against the two-channel dataset and against a
numpy float64 restatement, bit for bit; the Welford moments against the numpy float64 recurrence, bit for bit; and
predict_stack / split.main end to end on the tiny InDI network of tests/multi_rank_predict_seeded.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from tests import nets
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
SEED = 11


# ----------------------------------------------------------------------------- gather
def _channels(shape, top, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, shape), rng.integers(0, top, shape)


def _two_channel(c0, c1, patch, grid):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    return SplitDatasetTiledPred("Hagen", DataLocation(arrays=(c0.astype(np.float32), c1.astype(np.float32))), patch,
                                 grid_size=grid, max_qval=0.98, channel_weights=[1, 1])


def _restate(host, plan, ids, nd, clip=None):
    """The expression of include/dsx.h on the host: widen to fp32 (exact), clip at the fp32 clip, then
    (float)(((double)x - mean) / std) with numpy's float64 statistics."""
    p = plan.patch_shape[1]
    out = np.empty((len(ids), 1, p, p), np.float32)
    for k, i in enumerate(ids):
        n, y, x = (int(v) for v in plan.patch_start[i])
        t = host[n, y:y + p, x:x + p].astype(np.float32)
        if clip is not None:
            t = np.minimum(t, np.float32(clip))
        out[k, 0] = ((t.astype(np.float64) - np.float64(nd["mean_input"])) / np.float64(nd["std_input"])).astype(np.float32)
    return torch.from_numpy(out)


def _id_lists(total):
    return [list(range(0, total)), list(range(1, total, 2)), list(range(2, total, 3)), [total - 1], [5]]


@pytest.mark.parametrize("shape", [(2, 40, 57), (2, 48, 64)])
@pytest.mark.parametrize("dtype,top", [(np.uint16, 32768), (np.uint8, 128)])
def test_gather_input_equals_the_two_channel_input(shape, dtype, top):
    """Frames (2, 40, 57), patch 16, grid 8: the shifted last tiles start at x0 = 41 and y0 = 24 (odd starts, a row pitch
    that is not 8-byte aligned for uint16); (2, 48, 64) is the fully aligned case.  s = c0 + c1 in the stack's own width
    against the two-channel set's 'input' (its own dict, weights [1, 1]): torch.equal on the bits."""
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    c0, c1 = _channels(shape, top, 3)
    two = _two_channel(c0, c1, 16, 8)
    nd = two.get_normalization_dict()
    s = (c0 + c1).astype(dtype)
    stack = InputStackTiledPred(s, 16, nd, grid_size=8)
    assert stack.resident_bytes() == s.nbytes and len(stack) == len(two) == stack.plan.total
    if shape == (2, 40, 57):
        assert tuple(stack.plan.patch_start[-1]) == (1, 24, 41)
    for ids in _id_lists(stack.plan.total):
        got, want = stack.tiles(ids)["input"], two.tiles(ids)["input"]
        assert got.shape == (len(ids), 1, 16, 16) and same_bits(got, want), ids[:3]
        assert same_bits(got.cpu(), _restate(s, stack.plan, ids, nd)), ids[:3]
    # an id list that is no arithmetic sequence, and the numpy item
    odd = [7, 0, 3]
    assert same_bits(stack.tiles(odd)["input"], two.tiles(odd)["input"])
    item = stack[stack.plan.total - 1]
    assert set(item) == {"input"} and item["input"].dtype == np.float32
    assert np.array_equal(item["input"], two[stack.plan.total - 1]["input"])


@pytest.mark.parametrize("shape,patch,grid", [((2, 40, 57), 16, 8), ((2, 48, 64), 16, 8), ((2, 40, 57), 18, 6)])
def test_gather_input_float_stack_and_clip_against_numpy(shape, patch, grid):
    """A float32 stack with non-integer values, and every pixel type under input_clip, against the float64 restatement;
    patch 18 (no multiple of 4) takes the ragged groups and the scalar stores."""
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    rng = np.random.default_rng(9)
    nd = dict(mean_input=np.float64(0.1 + 0.2) * 1000, std_input=np.float64(123.456789), mean_target=np.zeros(2),
              std_target=np.ones(2))
    f = (rng.random(shape) * 1000).astype(np.float32)
    for host, clip in ((f, None), (f, 700.25), (rng.integers(0, 65536, shape).astype(np.uint16), 20000.5),
                       (rng.integers(0, 65536, shape).astype(np.uint16), None),
                       (rng.integers(0, 256, shape).astype(np.uint8), 100)):
        stack = InputStackTiledPred(host, patch, nd, grid_size=grid, input_clip=clip)
        for ids in _id_lists(stack.plan.total):
            got = stack.tiles(ids)["input"].cpu()
            assert same_bits(got, _restate(host, stack.plan, ids, nd, clip)), (host.dtype, clip, ids[:3])
        if clip is not None:
            top = (np.float64(np.float32(clip)) - nd["mean_input"]) / nd["std_input"]
            assert float(stack.tiles(range(stack.plan.total))["input"].max()) == np.float32(top)


@pytest.mark.parametrize("patch,grid,guard", [(16, 8, 4), (16, 8, 3), (18, 6, 4), (18, 6, 5)])
def test_gather_input_writes_its_tiles_and_nothing_else(patch, grid, guard):
    """The output inside a larger NaN-filled buffer: every tile element is written, the guard elements on both sides
    keep their NaN bits.  guard 4 keeps the output 16-byte aligned (float4 stores), 3 and 5 do not (scalar stores)."""
    from diffsplitting_amd import _lib
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    host = np.random.default_rng(2).integers(0, 60000, (2, 40, 57)).astype(np.uint16)
    nd = dict(mean_input=30000.0, std_input=17000.0, mean_target=np.zeros(2), std_target=np.ones(2))
    stack = InputStackTiledPred(host, patch, nd, grid_size=grid)
    for first, stride, count in ((0, 1, stack.plan.total), (1, 2, 5), (stack.plan.total - 1, 1, 1)):
        n = count * patch * patch
        buf = torch.full((guard + n + guard,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib.dsx_tileplan_gather_input(stack.plan.handle, C.c_void_p(stack._dev.data_ptr()), _lib.PIX_U16,
                                                      first, stride, count, 30000.0, 17000.0, -1.0,
                                                      C.c_void_p(buf[guard:].data_ptr()),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = buf.cpu()
        assert torch.isnan(got[:guard]).all() and torch.isnan(got[guard + n:]).all()
        ids = [first + k * stride for k in range(count)]
        assert same_bits(got[guard:guard + n].view(count, 1, patch, patch), _restate(host, stack.plan, ids, nd))


def test_loaded_normalization_cuts_the_same_tiles(tmp_path):
    from diffsplitting_amd.data.normalization import load_normalization, save_normalization
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    c0, c1 = _channels((2, 40, 57), 3000, 4)
    arrays = (c0.astype(np.float32), c1.astype(np.float32))
    own = SplitDatasetTiledPred("Hagen", DataLocation(arrays=arrays), 16, grid_size=8, max_qval=0.97, channel_weights=[1, 0.3],
                                upper_clip=True)
    path = str(tmp_path / "n.json")
    save_normalization(path, own.get_normalization_dict(), data_type="Hagen", channel_weights=[1, 0.3], max_qval=0.97,
                       upper_clip=True, target_channel_idx=None)
    nd, meta = load_normalization(path)
    again = SplitDatasetTiledPred("Hagen", DataLocation(arrays=arrays), 16, grid_size=8, max_qval=0.5, normalization_dict=nd,
                                  channel_weights=meta["channel_weights"], upper_clip=meta["upper_clip"])
    a, b = own.tiles(range(len(own))), again.tiles(range(len(own)))
    assert same_bits(a["input"], b["input"]) and same_bits(a["target"], b["target"])


# ----------------------------------------------------------------------------- moments
def _welford(samples):
    """The recurrence of include/dsx.h in numpy float64, line by line in the same order."""
    mean = m2 = None
    for r, x in enumerate(samples):
        x = x.astype(np.float64)
        if r == 0:
            mean, m2 = x.copy(), np.zeros_like(x)
            continue
        d = x - mean
        mean = mean + d / (r + 1)
        m2 = m2 + d * (x - mean)
    n = len(samples)
    std = np.sqrt(m2 / (n - 1)).astype(np.float32) if n > 1 else np.zeros(mean.shape, np.float32)
    return mean.astype(np.float32), std


@pytest.mark.parametrize("count", [1, 255, 4097])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_moments_equal_the_float64_recurrence(count, n):
    from diffsplitting_amd import engine
    rng = np.random.default_rng(count * 10 + n)
    const = np.float32(0.1) * np.ones(count, np.float32)
    series = {"constant": [const] * n,
              "offset": [(1000 + 1e-2 * rng.standard_normal(count)).astype(np.float32) for _ in range(n)],
              "normal": [rng.standard_normal(count).astype(np.float32) for _ in range(n)]}
    for name, xs in series.items():
        mean = m2 = None
        for r, x in enumerate(xs):
            mean, m2 = engine.moments_update(torch.from_numpy(x).cuda(), mean, m2, r)
        got_mean, got_std = engine.moments_finish(mean, m2, n)
        want_mean, want_std = _welford(xs)
        assert same_bits(got_mean.cpu(), torch.from_numpy(want_mean)), name
        assert same_bits(got_std.cpu(), torch.from_numpy(want_std)), name
        assert not torch.isnan(got_std).any()
        if name == "constant":
            assert (got_mean.cpu() == 0.1 * torch.ones(1)).all() and (got_std == 0).all()   # 0.1 as fp32, exactly
        if n == 1:
            assert (got_std == 0).all() and same_bits(got_mean.cpu(), torch.from_numpy(xs[0]))
        only_mean, none = engine.moments_finish(mean, m2, n, want_std=False)
        assert none is None and same_bits(only_mean, got_mean)


def test_moments_python_face_refuses_what_the_kernel_cannot_take():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    x = torch.zeros(8, device="cuda")
    with pytest.raises(DsxError, match="r = 1 needs the running mean"):
        engine.moments_update(x, None, None, 1)
    mean, m2 = engine.moments_update(x)
    with pytest.raises(DsxError, match="float64 CUDA tensor of 8 elements"):
        engine.moments_update(x, mean[:4].contiguous(), m2, 1)
    with pytest.raises(DsxError, match="contiguous float32"):
        engine.moments_update(x.double(), mean, m2, 1)
    with pytest.raises(DsxError, match="n = 0"):
        engine.moments_finish(mean, m2, 0)


# ----------------------------------------------------------------------------- end to end
SHAPE, PATCH, GRID, BATCH, STEPS = (3, 96, 160), 64, 32, 4, 2


@pytest.fixture(scope="module")
def world():
    """The tiny InDI network of tests/multi_rank_predict_seeded.py, the two channels, their sum as a uint16 stack and the
    predictions every test below compares with (computed once)."""
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from diffsplitting_amd.model import networks
    from tests.util import golden_state_dict
    torch.set_grad_enabled(False)
    sd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()})
    assert netG.e == 0.01                                             # the sampler's own noise scale: the draws matter
    c0, c1 = _channels(SHAPE, 3000, 21)
    two = _two_channel(c0, c1, PATCH, GRID)
    s = (c0 + c1).astype(np.uint16)
    stack = InputStackTiledPred(s, PATCH, two.get_normalization_dict(), grid_size=GRID)
    assert stack.plan.total == 24
    kw = dict(batch_tiles=BATCH, num_timesteps=STEPS, seed=SEED)
    one, plan = predict_stack(netG, stack, **kw)
    three, _ = predict_stack(netG, stack, samples=3, return_std=True, **kw)
    return dict(netG=netG, c0=c0, c1=c1, two=two, s=s, stack=stack, one=one, three=three, plan=plan, kw=kw)


def test_predict_stack_equals_the_two_channel_prediction(world):
    from diffsplitting_amd.data.tiled_predict import predict_stack
    netG, stack, plan = world["netG"], world["stack"], world["plan"]
    assert set(world["one"]) == {"mean"} and world["one"]["mean"].shape == SHAPE + (2,)
    assert torch.isfinite(world["one"]["mean"]).all()
    ref, _ = predict_stack(netG, world["two"], **world["kw"])
    assert set(ref) == {"mean", "psnr"} and ref["psnr"].shape == (3, 2) and torch.isfinite(ref["psnr"]).all()
    assert same_bits(world["one"]["mean"], ref["mean"])
    # the batches of four from the last to the first, every tile id on its own stream: the same canvas
    outs = {}
    for i in reversed(range(0, plan.total, BATCH)):
        chunk = list(range(i, i + BATCH))
        netG.inference(stack.tiles(chunk)["input"], continuous=False, num_timesteps=STEPS, seed=SEED, sample_ids=chunk)
        outs[i] = netG.last_full_batch.clone()
    assert same_bits(world["one"]["mean"], plan.stitch(torch.cat([outs[i] for i in sorted(outs)])))
    # samples = 1 with the spread asked for: the same mean, a spread of exactly zero
    flat, _ = predict_stack(netG, stack, return_std=True, **world["kw"])
    assert same_bits(flat["mean"], world["one"]["mean"]) and (flat["std"] == 0).all()
    with pytest.raises(ValueError, match="samples = 0"):
        predict_stack(netG, stack, samples=0)


def test_predict_stack_three_samples_equal_the_restated_loop(world):
    netG, stack, plan = world["netG"], world["stack"], world["plan"]
    means, stds = [], []
    for i in range(0, plan.total, BATCH):
        chunk = list(range(i, i + BATCH))
        x = stack.tiles(chunk)["input"]
        xs = []
        for r in range(3):
            netG.inference(x, continuous=False, num_timesteps=STEPS, seed=SEED, sample_ids=[k + r * plan.total for k in chunk])
            xs.append(netG.last_full_batch.cpu().numpy())
        m, sd = _welford(xs)
        means.append(torch.from_numpy(m))
        stds.append(torch.from_numpy(sd))
    want_mean, want_std = plan.stitch(torch.cat(means).cuda()), plan.stitch(torch.cat(stds).cuda())
    got = world["three"]
    assert set(got) == {"mean", "std"}
    assert same_bits(got["mean"], want_mean) and same_bits(got["std"], want_std)
    assert (got["std"] > 0).any() and not same_bits(got["mean"], world["one"]["mean"])   # the repeats do differ


def test_command_line_round_trip(world, tmp_path, monkeypatch):
    from diffsplitting_amd import split
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.normalization import load_normalization
    from diffsplitting_amd.data.tiff import imread, imwrite
    from diffsplitting_amd.data.tiled_predict import predict_stack
    cfg = {"name": "tiny_input", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": PATCH, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 1],
                        "train": {"name": "Hagen"}, "val": {"name": "Hagen"}},
           "model": nets.hagen64_section()}
    cfg_path = str(tmp_path / "tiny.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    both = np.stack([world["c0"], world["c1"]], axis=-1).astype(np.float32)
    np.save(tmp_path / "both.npy", both)
    imwrite(str(tmp_path / "s.tif"), world["s"])
    p = lambda name: str(tmp_path / name)
    models = []
    create = split.create_model
    monkeypatch.setattr(split, "create_model", lambda opt: models.append(create(opt)) or models[-1])

    def main(*argv):
        torch.manual_seed(1234)                                       # the model's random initial weights
        return split.main(["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--steps", str(STEPS),
                           "--batch-tiles", str(BATCH), "--sample-seed", str(SEED)] + list(argv))

    pred_a = main("--frames", p("both.npy"), "--save-norm", p("norm.json"), "--out", p("a.npy"))
    nd, meta = load_normalization(p("norm.json"))
    assert meta["data_type"] == "Hagen" and meta["channel_weights"] == [1.0, 1.0] and meta["target_channel_idx"] is None
    own = world["two"].get_normalization_dict()
    assert nd["mean_input"] == own["mean_input"] and np.array_equal(nd["std_target"], np.asarray(own["std_target"]).reshape(-1))
    with pytest.raises(SystemExit, match="--std-out.*--samples 2"):
        main("--input", p("s.tif"), "--norm", p("norm.json"), "--out", p("b.tif"), "--std-out", p("c.tif"), "--samples", "1")
    pred_b = main("--input", p("s.tif"), "--norm", p("norm.json"), "--out", p("b.tif"))
    assert same_bits(pred_a, pred_b)
    a, b = np.load(p("a.npy")), imread(p("b.tif"))
    assert a.shape == SHAPE + (2,) and b.shape == (6,) + SHAPE[1:] and b.dtype == np.float32
    assert np.array_equal(b.reshape(3, 2, *SHAPE[1:]).transpose(0, 2, 3, 1).view(np.int32), a.view(np.int32))
    # three samples: mean and spread in raw counts, as predict_stack gives them with the same network
    main("--input", p("s.tif"), "--norm", p("norm.json"), "--out", p("b.tif"), "--std-out", p("c.tif"), "--samples", "3")
    stack = InputStackTiledPred(p("s.tif"), PATCH, nd, grid_size=GRID)
    want, _ = predict_stack(models[-1].netG, stack, samples=3, return_std=True, **world["kw"])
    mean_t = torch.as_tensor(nd["mean_target"], dtype=torch.float32, device="cuda")
    std_t = torch.as_tensor(nd["std_target"], dtype=torch.float32, device="cuda")
    pages = lambda name: torch.from_numpy(imread(p(name)).reshape(3, 2, *SHAPE[1:]).transpose(0, 2, 3, 1).copy())
    assert same_bits(pages("b.tif"), (want["mean"] * std_t + mean_t).cpu())
    assert same_bits(pages("c.tif"), (want["std"] * std_t).cpu())
    assert (pages("c.tif") > 0).any()
    # the two-channel prediction takes the flags too, and reports the PSNR of the mean
    pred_m = main("--frames", p("both.npy"), "--samples", "3", "--std-out", p("d.npy"), "--out", p("e.npy"))
    assert same_bits(pred_m, want["mean"]) and np.array_equal(np.load(p("d.npy")).view(np.int32), pages("c.tif").numpy().view(np.int32))
