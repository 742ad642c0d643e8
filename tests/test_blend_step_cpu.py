"""Frame diffusion for the InDI family without a GPU: dsx_tileplan_blend_step against header, binding and library, the
numpy restatement of its contract (tests/blend_step_ref.py), every host refusal of the entry point with fake device
pointers, and the refusals of ``predict_stack_frames`` and ``split --frame-steps`` by message, with no rank started and
no device touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import blend_ref
from tests.blend_step_ref import blend_step_ref
from tests.host_checks import BLEND_PLANS, ERR_INVALID, FAKE, binding, cpu_samplers, last_error, tile_plan
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_bound_and_exported():
    lib = binding()
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    assert re.search(r"\bint dsx_tileplan_blend_step\(", header)
    assert len(lib.SIGNATURES["dsx_tileplan_blend_step"][1]) == 13 and hasattr(lib._cdll, "dsx_tileplan_blend_step")
    assert lib.lib.dsx_abi_version() == 2
    from diffsplitting_amd.data.tiling import TilePlan
    assert callable(TilePlan.blend_step)


# ----------------------------------------------------------------------------- the restatement
def test_one_tile_per_frame_is_the_pointwise_formula():
    plan = tile_plan((3, 32, 32), 32, 32)
    assert plan.total == 3
    rng = np.random.default_rng(1)
    tiles = rng.standard_normal((3, 2, 32, 32)).astype(np.float32)
    X, Z = (rng.standard_normal((3, 32, 32, 2)).astype(np.float32) for _ in range(2))
    wy, wx = blend_ref.window_pair(plan, "hann")
    f = np.float32
    c0, cx, sg = f(1 / 3), f(1 - f(1 / 3)), f(0.0066667)
    v = tiles.transpose(0, 2, 3, 1)
    want = ((c0 * v).astype(f) + (cx * X).astype(f)).astype(f)
    assert np.array_equal(blend_step_ref(plan, tiles, wy, wx, X, c0, cx, 0.0, None).view(np.int32), want.view(np.int32))
    want = (want + (Z * sg).astype(f)).astype(f)
    got = blend_step_ref(plan, tiles, wy, wx, X, c0, cx, sg, Z)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_tiles_cut_from_one_frame_give_the_frame_back(shape, patch, grid):
    """c_x0 = 1, c_xt = 0, sigma = 0: 1 * v + 0 * X = v exactly, so the bound is the blend's own (test_blend_cpu):
    |out - v| <= (2 n + 1) 2^-24 |v| with n <= 12 contributors"""
    plan = tile_plan(shape, patch, grid)
    rng = np.random.default_rng(6)
    frame = rng.standard_normal(plan.data_shape + (1,)).astype(np.float32)
    X = rng.standard_normal(plan.data_shape + (1,)).astype(np.float32)
    tiles = blend_ref.cut_tiles(plan, frame)
    for name in ("triangle", "hann"):
        got = blend_step_ref(plan, tiles, *blend_ref.window_pair(plan, name), X, 1.0, 0.0, 0.0, None)
        assert (np.abs(got.astype(np.float64) - frame) <= 25 * 2.0 ** -24 * np.abs(frame)).all(), name


def test_sigma_zero_ignores_the_noise():
    plan = tile_plan((1, 40, 56), 32, 16)
    rng = np.random.default_rng(2)
    tiles = rng.standard_normal((plan.total, 2, 32, 32)).astype(np.float32)
    X = rng.standard_normal(plan.data_shape + (2,)).astype(np.float32)
    win = blend_ref.window_pair(plan, "triangle")
    nan = np.full_like(X, np.nan)
    got = blend_step_ref(plan, tiles, *win, X, 0.25, 0.75, 0.0, nan)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.int32), blend_step_ref(plan, tiles, *win, X, 0.25, 0.75, 0.0, None).view(np.int32))
    assert np.isnan(blend_step_ref(plan, tiles, *win, X, 0.25, 0.75, 0.5, nan)).all()


# ----------------------------------------------------------------------------- host refusals, no device
def _step(h, tiles=FAKE, Cn=1, world=1, stride=0, state=FAKE, c=(0.5, 0.5, 0.1), seed=3, id_base=0, draw=1):
    return binding().lib.dsx_tileplan_blend_step(h, tiles, Cn, world, stride, state, c[0], c[1], c[2], C.c_uint64(seed),
                                              C.c_uint64(id_base), C.c_uint32(draw), None)


def test_blend_step_refusals():
    from diffsplitting_amd.data import tiling
    name = "tileplan_blend_step"
    trim = tiling.TilePlan((1, 40, 56), (1, 16, 16), (1, 32, 32), mode=tiling.TRIM)
    ones = np.ones(32, dtype=np.float32)
    assert binding().lib.dsx_tileplan_set_window(trim.handle, ones, ones) == 0
    assert _step(trim.handle) == ERR_INVALID and f"{name}: the plan's tiles do not cover the frames" in last_error()
    plan = tile_plan((2, 40, 57), 16, 8)
    assert _step(plan.handle) == ERR_INVALID and f"{name}: the plan has no window" in last_error()
    plan.set_window("hann")
    # what the blend refuses
    assert _step(plan.handle, Cn=0) == ERR_INVALID and f"{name}: C = 0" in last_error()
    assert _step(plan.handle, world=0) == ERR_INVALID and f"{name}: world = 0" in last_error()
    assert _step(None) == ERR_INVALID and f"{name}: null argument" in last_error()
    assert _step(plan.handle, tiles=None) == ERR_INVALID and f"{name}: null argument" in last_error()
    need = 19 * 2 * 16 * 16                                             # 56 tiles over 3 ranks: rank 0 holds 19
    for stride in (need - 1, 0, -5):
        assert _step(plan.handle, Cn=2, world=3, stride=stride) == ERR_INVALID
        assert f"{name}: rank_stride_elems = {stride} is smaller than rank 0's 19 whole tiles" in last_error()
    # a null state
    assert _step(plan.handle, state=None) == ERR_INVALID and f"{name}: null argument" in last_error()
    # the field ids of the plan's two frames and the draw ordinal
    for id_base in (2 ** 40 - 1, 2 ** 40, 2 ** 63, 2 ** 64 - 1):
        assert _step(plan.handle, id_base=id_base) == ERR_INVALID
        assert f"{name}: id_base = {id_base} with 2 frames" in last_error() and "below 2^40" in last_error()
    for draw in (2 ** 24, 2 ** 32 - 1):
        assert _step(plan.handle, draw=draw) == ERR_INVALID and f"{name}: draw ordinal {draw}" in last_error()
    # a coefficient that is not finite
    for k in range(3):
        for bad in (float("nan"), float("inf"), float("-inf")):
            c = [0.5, 0.5, 0.1]
            c[k] = bad
            assert _step(plan.handle, c=c) == ERR_INVALID and f"{name}: c_x0 = " in last_error() and "must be finite" in last_error()


def test_the_python_face_refuses_before_the_library(monkeypatch):
    from diffsplitting_amd import _lib as L
    from diffsplitting_amd._lib import DsxError
    monkeypatch.setattr(L, "require_gpu", lambda: None)
    plan = tile_plan((2, 40, 57), 16, 8)
    with pytest.raises(DsxError, match="tiles must be a .* float32 CUDA tensor"):
        plan.blend_step(torch.zeros(plan.total, 2, 16, 16), torch.zeros(2, 40, 57, 2), 0.5, 0.5, 0.0, 3, 1)


# ----------------------------------------------------------------------------- the drivers' refusals, no rank, no device
def test_predict_stack_frames_refuses_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd import _lib as L, parallel
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tile_predict
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames

    def touched(*a, **k):
        raise AssertionError("the refusal came too late")
    monkeypatch.setattr(L, "require_gpu", touched)
    monkeypatch.setattr(tile_predict, "TileExchange", touched)
    monkeypatch.setattr(parallel, "all_gather_flat", touched)
    g, i, j = cpu_samplers()

    class Stack:
        plan = tile_plan((2, 40, 57), 32, 16)

        def tiles(self, ids):
            touched()

    class Many(Stack):
        class plan:
            data_shape = (2 ** 38 + 1, 40, 57)
    what = "predict_stack_frames"
    with pytest.raises(DsxError, match=f"{what}: GaussianSampler is a Gaussian sampler.*predict_stack\\(fuse=True\\)"):
        predict_stack_frames(g, Stack(), seed=3)
    for smp in (i, j):
        with pytest.raises(DsxError, match=f"{what} needs seed="):
            predict_stack_frames(smp, Stack())
        for t in ([0.5, 0.25], (0.5,), torch.tensor([0.5, 0.5]), np.array([0.5, 0.5])):
            with pytest.raises(DsxError, match=f"{what}: a per-sample t_float_start: a frame has one time"):
                predict_stack_frames(smp, Stack(), seed=3, t_float_start=t)
        for n in (0, -1):
            with pytest.raises(DsxError, match=f"{what}: samples = {n}"):
                predict_stack_frames(smp, Stack(), seed=3, samples=n)
        with pytest.raises(DsxError, match=f"{what}: samples \\* frames exceeds the 2\\^39 field ids"):
            predict_stack_frames(smp, Many(), seed=3, samples=2)
        with pytest.raises(DsxError, match=f"{what}: window = 'box'"):
            predict_stack_frames(smp, Stack(), seed=3, window="box")
    for smp, child in ((i, i), (j, j.indi2)):
        child._noise_mode = "brownian"
        with pytest.raises(DsxError, match=f"{what}: noise mode 'brownian'"):
            predict_stack_frames(smp, Stack(), seed=3)
        child._noise_mode = "gaussian"
    # predict_stack keeps refusing InDI, and names the new function
    with pytest.raises(DsxError, match="predict_stack: fuse: InDISampler is not a Gaussian sampler.*predict_stack_frames"):
        predict_stack(i, Stack(), noise="field", seed=3, fuse=True)


def test_split_refuses_frame_steps_where_it_does_not_apply(tmp_path, monkeypatch):
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfgs = {w: write_config(tmp_path, w) for w in ("sr3", "ddpm", "indi", "joint_indi")}

    def refused(argv, match, config="indi"):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", cfgs[config]] + argv)

    seed = ["--sample-seed", "3"]
    for which in ("sr3", "ddpm"):
        refused(["--frame-steps"] + seed, f"--frame-steps.*indi / joint_indi.*{which}", config=which)
        refused(["--frame-steps", "--solver", "ddim", "--solver-steps", "4"] + seed, "--frame-steps with --solver", config=which)
        refused(["--frame-steps", "--fuse-steps", "--noise-field", "--solver", "ddim", "--solver-steps", "4"] + seed,
                "--frame-steps together with --fuse-steps", config=which)
    for which in ("indi", "joint_indi"):
        refused(["--frame-steps"], "--frame-steps needs --sample-seed", config=which)
        refused(["--frame-steps", "--stitch", "crop"] + seed, "--frame-steps with --stitch crop", config=which)
        refused(["--frame-steps", "--gpus", "2", "--stitch", "crop"] + seed, "--frame-steps with --stitch crop", config=which)
    refused(["--frame-steps", "--validate"], "--frame-steps.*--validate")
    refused(["--frame-steps", "--mix-t", "0.3", "--t-from", "given"] + seed, "--frame-steps.*--mix-t", config="joint_indi")
    refused(["--frame-steps", "--mmse", "2"] + seed, "--frame-steps.*--mmse|--mmse", config="joint_indi")
    # without the flag nothing of this is looked at: the run goes on to start its ranks
    with pytest.raises(AssertionError, match="a rank was started"):
        split.main(["-c", cfgs["indi"]] + seed)
