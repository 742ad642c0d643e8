"""Blended stitching on the MI355X (`-m gpu`): dsx_tileplan_blend bit for bit against the numpy restatement of its
contract (tests/blend_ref.py) -- ragged plans, pw % 4 = 2, up to 12 contributors, a single tile, C = 1..3, both windows,
an unaligned canvas --, the rank-slot layouts against the one-rank bits, the PSNR sums, dsx_tileplan_gather_canvas
against torch slicing, and the drivers: ``predict_stack(stitch="blend")`` against the test's own loop plus ``blend_ref``,
``TileExchange(blend=True)`` over ranks, ``split --stitch blend`` end to end."""
import numpy as np
import pytest
import torch

from tests import blend_ref
from tests import tiled_util as T
from tests.bits import same_bits
from tests.metrics_ref import range_invariant_psnr
from tests.rank_worker import run_ranks
from tests.tiled_util import BATCH, BLEND_PLANS, SEED, SOLVERS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _same(canvas, want):
    return same_bits(canvas.cpu(), torch.from_numpy(want))


# ----------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("name", ["triangle", "hann"])
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_blend_is_its_restatement(shape, patch, grid, name):
    plan = T.plan_of(shape, patch, grid)
    plan.set_window(name)
    wy, wx = blend_ref.window_pair(plan, name)
    rng = np.random.default_rng(3)
    for Cn in (1, 2, 3):
        tiles = T.random_tiles(plan, Cn)
        got = plan.blend(torch.from_numpy(tiles).cuda())
        assert got.shape == plan.data_shape + (Cn,) and _same(got, blend_ref.blend_ref(plan, tiles, wy, wx)), Cn
        # tiles cut from one frame: they agree on every overlap, the blend stays within a few ulp of the frame
        frame = rng.standard_normal(plan.data_shape + (Cn,)).astype(np.float32)
        cut = blend_ref.cut_tiles(plan, frame)
        got = plan.blend(torch.from_numpy(cut).cuda())
        assert _same(got, blend_ref.blend_ref(plan, cut, wy, wx)), Cn
        assert (np.abs(got.cpu().numpy().astype(np.float64) - frame) <= 25 * 2.0 ** -24 * np.abs(frame)).all()


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_an_integer_frame_comes_back_exactly(shape, patch, grid):
    plan = T.plan_of(shape, patch, grid)
    plan.set_window("triangle")
    for Cn in (1, 2, 3, 4, 5):                                          # 5: the kernel's any-C form
        frame = torch.randint(-64, 65, plan.data_shape + (Cn,), generator=torch.Generator().manual_seed(Cn)).float().cuda()
        tiles = plan.gather_canvas(frame)
        assert same_bits(plan.blend(tiles), frame), Cn


@pytest.mark.parametrize("Cn", [1, 2, 4])
def test_blend_into_an_unaligned_view(Cn):
    """the canvas one float past a 16-byte boundary: one dword per channel whatever C is; its NaN neighbours stay NaN"""
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("hann")
    tiles = T.random_tiles(plan, Cn)
    n = int(np.prod(plan.data_shape)) * Cn
    buf = torch.full((n + 9,), float("nan"), device="cuda")
    view = buf[5:5 + n].view(plan.data_shape + (Cn,))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    out = plan.blend(torch.from_numpy(tiles).cuda(), canvas=view)
    assert out.data_ptr() == view.data_ptr()
    assert _same(view, blend_ref.blend_ref(plan, tiles, *blend_ref.window_pair(plan, "hann")))
    assert bool(torch.isnan(buf[:5]).all()) and bool(torch.isnan(buf[5 + n:]).all())


# ----------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("world", [2, 3])
def test_the_rank_slot_layouts_give_the_one_rank_bits(world):
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("hann")
    for Cn in (1, 2, 3):
        tiles = T.random_tiles(plan, Cn)
        one = plan.blend(torch.from_numpy(tiles).cuda())
        buf = blend_ref.slots(plan, tiles, world)
        assert buf.shape == (world, plan.blend_rank_stride(world, Cn))
        assert same_bits(plan.blend(torch.from_numpy(buf).cuda(), world=world, Cn=Cn), one), Cn


# ----------------------------------------------------------------------------- 3. PSNR
@pytest.mark.parametrize("Cn", [1, 2, 3, 4])
def test_blend_psnr(Cn):
    plan = T.plan_of((2, 40, 57), 16, 8)
    plan.set_window("triangle")
    rng = np.random.default_rng(9)
    gt = rng.standard_normal(plan.data_shape + (Cn,)).astype(np.float32)
    tiles = blend_ref.cut_tiles(plan, gt) + 0.3 * T.random_tiles(plan, Cn)
    t = torch.from_numpy(tiles).cuda()
    canvas, psnr = plan.blend(t, gt=torch.from_numpy(gt).cuda())
    part = plan.last_blend_partials.clone()
    assert part.shape == (2, plan.blend_blocks(), Cn, 8)
    want = blend_ref.blend_ref(plan, tiles, *blend_ref.window_pair(plan, "triangle"))
    assert _same(canvas, want) and same_bits(canvas, plan.blend(t))
    err = np.abs(psnr.cpu().numpy() - range_invariant_psnr(gt, want)).max()
    print(f"\nC = {Cn}: largest |psnr - float64| = {err:.3e}")
    assert err < 1e-3                                                   # the bound of the stitch-PSNR test (test_gpu_boundary)
    plan.blend(t, gt=torch.from_numpy(gt).cuda())
    assert torch.equal(plan.last_blend_partials.view(torch.int64), part.view(torch.int64))


# ----------------------------------------------------------------------------- 4. the canvas gather
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS[:4], ids=str)
def test_gather_canvas_is_torch_slicing(shape, patch, grid):
    plan = T.plan_of(shape, patch, grid)
    p = patch
    for Cn in (1, 2, 3):
        canvas = torch.randn(plan.data_shape + (Cn,), generator=torch.Generator().manual_seed(Cn)).cuda()
        for ids in (None, list(range(3, plan.total, 4)), [plan.total - 1, 2, 2, 0, plan.total // 2]):
            got = plan.gather_canvas(canvas, ids)
            want = torch.stack([canvas[n, y:y + p, x:x + p].permute(2, 0, 1)
                                for n, y, x in plan.patch_start[range(plan.total) if ids is None else ids]])
            assert same_bits(got, want), (Cn, ids)
        assert plan.gather_canvas(canvas, []).shape == (0, Cn, p, p)


# ----------------------------------------------------------------------------- 5. the drivers
def _own_loop(smp, stack, run):
    """the prediction of every tile, batch by batch from the last to the first, with a tile's id as its stream id"""
    plan, tiles = stack.plan, {}
    for i in reversed(range(0, plan.total, BATCH)):
        chunk = list(range(i, i + BATCH))
        tiles[i] = run(stack.tiles(chunk)["input"], chunk)
    return torch.cat([tiles[i] for i in sorted(tiles)])


@pytest.mark.parametrize("name", ["dpmpp2m", "ddim", "indi"])
def test_predict_stack_blend(name):
    """frames (2, 40, 57), patch 32, grid 16: 12 tiles in batches of 4; `seed` gives every tile its own stream"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    stack = T.stack32()
    plan = stack.plan
    if name == "indi":
        smp, kw = T.indi(), dict(num_timesteps=3)

        def run(x, chunk):
            smp.inference(x, continuous=False, num_timesteps=3, seed=SEED, sample_ids=chunk)
            return smp.last_full_batch.clone()
    else:
        smp, kw = T.sr3(), dict(solver=SOLVERS[name])
        run = lambda x, chunk: T.run(smp, x, SOLVERS[name], seed=SEED, sample_ids=chunk)
    tiles = _own_loop(smp, stack, run)
    for window in ("triangle", "hann"):
        out, plan2 = predict_stack(smp, stack, batch_tiles=BATCH, seed=SEED, stitch="blend", window=window, **kw)
        assert plan2 is plan and set(out) == {"mean"}
        assert _same(out["mean"], blend_ref.blend_ref(plan, tiles.cpu().numpy(), *blend_ref.window_pair(plan, window))), window
    crop, _ = predict_stack(smp, stack, batch_tiles=BATCH, seed=SEED, stitch="crop", **kw)
    default, _ = predict_stack(smp, stack, batch_tiles=BATCH, seed=SEED, **kw)
    assert same_bits(crop["mean"], plan.stitch(tiles)) and same_bits(default["mean"], crop["mean"])
    assert not torch.equal(out["mean"], crop["mean"])


def test_predict_stack_blend_mean_and_spread():
    """two posterior samples per tile: the float64 Welford of the two restated samples, mean and spread each blended"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["ddim"]
    plan = stack.plan
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, samples=2, return_std=True, stitch="blend")
    xs = [_own_loop(smp, stack, lambda x, chunk, r=r: T.run(smp, x, solver, seed=SEED,
                                                           sample_ids=[k + r * plan.total for k in chunk])).cpu().numpy()
          for r in range(2)]
    mean, std = T.welford(xs)
    win = blend_ref.window_pair(plan, "triangle")
    assert _same(got["mean"], blend_ref.blend_ref(plan, mean, *win))
    assert _same(got["std"], blend_ref.blend_ref(plan, std, *win)) and bool((got["std"] > 0).any())


def test_predict_stack_blend_psnr():
    """a dataset with a ground truth: 'psnr' comes out of the blend's own pass"""
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    rng = np.random.default_rng(0)
    frames = (rng.random((2, 40, 57, 2), dtype=np.float32) * 1000.0).astype(np.float32)
    val = SplitDatasetTiledPred("Hagen", DataLocation(arrays=(frames[..., 0], frames[..., 1])), 32, grid_size=16, max_qval=0.98,
                                enable_transforms=False, random_patching=False, device=torch.device("cuda"))
    smp, solver = T.sr3(), SOLVERS["dpmpp2m"]
    out, plan = predict_stack(smp, val, batch_tiles=BATCH, solver=solver, seed=SEED, stitch="blend")
    assert plan.total == 12 and out["psnr"].shape == (2, 2)
    gt = val.normalized_target_frames()
    want = range_invariant_psnr(gt.cpu().numpy(), out["mean"].cpu().numpy())
    assert np.abs(out["psnr"].cpu().numpy() - want).max() < 1e-3
    tiles = torch.cat([T.run(smp, val.tiles(list(range(i, i + BATCH)))["input"], solver, seed=SEED,
                            sample_ids=list(range(i, i + BATCH))) for i in range(0, plan.total, BATCH)])
    assert _same(out["mean"], blend_ref.blend_ref(plan, tiles.cpu().numpy(), *blend_ref.window_pair(plan, "triangle")))


def test_predict_tiled_blend():
    from diffsplitting_amd.data.tiled_predict import predict_tiled
    netG = T.indi()
    frames = torch.from_numpy(T.smooth((2, 40, 57))).cuda()
    got, plan = predict_tiled(netG, frames, 32, batch_tiles=BATCH, seed=SEED, stitch="blend", window="hann")
    tiles = []
    for i in range(0, plan.total, BATCH):
        chunk = list(range(i, i + BATCH))
        netG.inference(plan.gather(frames, chunk).unsqueeze(1), continuous=False, seed=SEED, sample_ids=chunk)
        tiles.append(netG.last_full_batch.clone())
    tiles = torch.cat(tiles)
    assert _same(got, blend_ref.blend_ref(plan, tiles.cpu().numpy(), *blend_ref.window_pair(plan, "hann")))
    crop, _ = predict_tiled(netG, frames, 32, batch_tiles=BATCH, seed=SEED)
    assert same_bits(crop, plan.stitch(tiles))


@pytest.mark.parametrize("world", [2, 3])
def test_blended_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout) share the hardware that is there, gloo transport:
    on every rank the blended canvas equals the one-rank tiles under blend_ref, bitwise (tests/multi_rank_predict_blend.py)"""
    r = run_ranks("multi_rank_predict_blend.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_BLEND_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ----------------------------------------------------------------------------- 6. split, end to end
def test_split_stitch_blend_end_to_end(tmp_path):
    """the flagged run twice (byte for byte the same file), once cropped and once under the other window"""
    data = T.split_runs(tmp_path, {"a": ["--stitch", "blend"], "b": ["--stitch", "blend"], "crop": [],
                                 "hann": ["--stitch", "blend", "--window", "hann"]})
    assert data["a"] == data["b"] and data["a"] != data["crop"] and data["a"] != data["hann"]
