"""Blended stitching without a GPU: the new entry points against header and binding, the numpy restatement of the blend
contract (tests/blend_ref.py) on integer frames (bit for bit the frame) and on random frames (a few ulp), the host
contributor tables against brute force, every host refusal of dsx_tileplan_set_window / _blend / _gather_canvas with
fake device pointers, and the refusals of ``predict_stack`` and ``split`` by message, with no rank started."""
import os
import re

import numpy as np
import pytest
import torch

from tests import blend_ref
from tests.host_checks import BLEND_PLANS, ERR_INVALID, FAKE, binding, cpu_samplers, last_error, tile_plan
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsx_tileplan_contributors": 3, "dsx_tileplan_set_window": 3, "dsx_tileplan_blend_blocks": 1,
       "dsx_tileplan_blend": 9, "dsx_tileplan_gather_canvas": 8}
# (frames, patch, grid): ragged extents with a shifted last row / column, up to 12 contributors, a single tile


def test_the_entry_points_are_declared_bound_and_exported():
    lib = binding()
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name, n in NEW.items():
        assert re.search(rf"\bint {name}\(", header), name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n and hasattr(lib._cdll, name)
    assert lib.lib.dsx_abi_version() == 2 and re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", header)


def test_windows():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.tiling import window
    assert window("triangle", 6).tolist() == [1, 2, 3, 3, 2, 1] and window("triangle", 5).tolist() == [1, 2, 3, 2, 1]
    for n in (1, 2, 7, 32, 512):
        for name in ("triangle", "hann"):
            w = window(name, n)
            assert w.dtype == np.float32 and w.shape == (n,) and np.isfinite(w).all() and (w > 0).all()
            assert np.array_equal(w, w[::-1])
        i = np.arange(n, dtype=np.float64)
        assert np.array_equal(window("hann", n), (np.sin(np.pi * (i + 0.5) / n) ** 2).astype(np.float32))
    t = window("triangle", 512).astype(np.float64)                     # every product of two values is exact in fp32
    assert np.array_equal(np.outer(t, t), np.outer(t, t).astype(np.float32).astype(np.float64)) and t.max() == 256
    with pytest.raises(DsxError, match="'box' is not a window"):
        window("box", 8)
    with pytest.raises(DsxError, match="n = 0"):
        window("hann", 0)


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_an_integer_frame_comes_back_bit_for_bit(shape, patch, grid):
    """tiles cut from one frame agree wherever they overlap; with integer values (|v| <= 64) and the integer triangle
    window every product and partial sum is an integer below 2^24, so num = v * den exactly and num / den = v"""
    plan = tile_plan(shape, patch, grid)
    rng = np.random.default_rng(5)
    frame = rng.integers(-64, 65, size=plan.data_shape + (2,)).astype(np.float32)
    wy, wx = blend_ref.window_pair(plan, "triangle")
    got = blend_ref.blend_ref(plan, blend_ref.cut_tiles(plan, frame), wy, wx)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), frame.view(np.int32))


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_a_random_frame_comes_back_within_a_few_ulp(shape, patch, grid):
    """n contributors: n products and n - 1 sums in num, n - 1 sums in den and one division, each within 2^-24 relative;
    the terms have one sign (w > 0, one v), so nothing cancels: |out - v| <= (2 n + 1) 2^-24 |v|, n <= 12 here"""
    plan = tile_plan(shape, patch, grid)
    frame = np.random.default_rng(6).standard_normal(plan.data_shape + (1,)).astype(np.float32)
    tiles = blend_ref.cut_tiles(plan, frame)
    for name in ("triangle", "hann"):
        got = blend_ref.blend_ref(plan, tiles, *blend_ref.window_pair(plan, name))
        assert (np.abs(got.astype(np.float64) - frame) <= 25 * 2.0 ** -24 * np.abs(frame)).all(), name


def test_random_tiles_against_float64():
    """independent tiles: the fp32 restatement against the same sums in float64"""
    plan = tile_plan((2, 40, 57), 16, 8)
    tiles = np.random.default_rng(7).standard_normal((plan.total, 3, 16, 16)).astype(np.float32)
    for name in ("triangle", "hann"):
        wy, wx = blend_ref.window_pair(plan, name)
        got, want = blend_ref.blend_ref(plan, tiles, wy, wx), blend_ref.blend_ref(plan, tiles, wy, wx, dtype=np.float64)
        assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS + [((2, 40, 57), 16, 8)], ids=str)
def test_contributor_tables(shape, patch, grid):
    plan = tile_plan(shape, patch, grid)
    rows, cols = plan.contributors()
    want_rows, want_cols = blend_ref.contributors_brute(plan)
    assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols)
    assert rows[:, 1].min() >= 1 and cols[:, 1].min() >= 1


def test_a_plan_that_does_not_cover_its_frames_has_no_tables():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tiling
    plan = tiling.TilePlan((1, 40, 56), (1, 16, 16), (1, 32, 32), mode=tiling.TRIM)
    with pytest.raises(DsxError, match="tileplan_contributors: the plan's tiles do not cover the frames"):
        plan.contributors()
    ones = np.ones(32, dtype=np.float32)
    assert binding().lib.dsx_tileplan_set_window(plan.handle, ones, ones) == 0
    assert binding().lib.dsx_tileplan_blend(plan.handle, FAKE, 1, 1, 0, FAKE, None, None, None) == ERR_INVALID
    assert "tileplan_blend: the plan's tiles do not cover the frames" in last_error()


# ----------------------------------------------------------------------------- host refusals, no device
def _blend(h, tiles=FAKE, Cn=1, world=1, stride=0, canvas=FAKE, gt=None, part=None):
    return binding().lib.dsx_tileplan_blend(h, tiles, Cn, world, stride, canvas, gt, part, None)


def test_blend_refusals():
    from diffsplitting_amd._lib import DsxError
    lib = binding().lib
    plan = tile_plan((2, 40, 57), 16, 8)
    assert _blend(plan.handle) == ERR_INVALID and "tileplan_blend: the plan has no window" in last_error()
    for k, bad in ((3, 0.0), (0, -1.0), (15, float("nan")), (7, float("inf")), (2, float("-inf"))):
        for axis in ("wy", "wx"):
            wy, wx = np.ones(16, dtype=np.float32), np.ones(16, dtype=np.float32)
            (wy if axis == "wy" else wx)[k] = bad
            assert lib.dsx_tileplan_set_window(plan.handle, wy, wx) == ERR_INVALID
            assert f"tileplan_set_window: {axis}[{k}]" in last_error() and "finite and > 0" in last_error()
            with pytest.raises(DsxError, match=rf"tileplan_set_window: {axis}\[{k}\]"):
                plan.set_window((wy, wx))
    assert lib.dsx_tileplan_set_window(plan.handle, None, np.ones(16, dtype=np.float32)) == ERR_INVALID
    assert lib.dsx_tileplan_set_window(None, np.ones(16, dtype=np.float32), np.ones(16, dtype=np.float32)) == ERR_INVALID
    assert _blend(plan.handle) == ERR_INVALID and "has no window" in last_error()          # a refused window sets nothing
    with pytest.raises(DsxError, match="must have 16 and 16 values, got 16 and 15"):
        plan.set_window((np.ones(16), np.ones(15)))
    plan.set_window("triangle")
    plan.set_window("hann")                                             # a second call replaces the first
    assert _blend(plan.handle, Cn=0) == ERR_INVALID and "tileplan_blend: C = 0" in last_error()
    assert _blend(plan.handle, world=0) == ERR_INVALID and "tileplan_blend: world = 0" in last_error()
    for kw in (dict(tiles=None), dict(canvas=None)):
        assert _blend(plan.handle, **kw) == ERR_INVALID and "tileplan_blend: null argument" in last_error()
    assert _blend(None) == ERR_INVALID and "tileplan_blend: null argument" in last_error()
    assert _blend(plan.handle, gt=FAKE) == ERR_INVALID and "PSNR sums need a partials buffer" in last_error()
    assert _blend(plan.handle, Cn=5, gt=FAKE, part=FAKE) == ERR_INVALID and "C <= 4" in last_error()
    # 56 tiles over 3 ranks: rank 0 holds 19 whole (2, 16, 16) tiles
    need = 19 * 2 * 16 * 16
    assert plan.blend_rank_stride(3, 2) == need
    for stride in (need - 1, 0, -5):
        assert _blend(plan.handle, Cn=2, world=3, stride=stride) == ERR_INVALID
        assert f"tileplan_blend: rank_stride_elems = {stride} is smaller than rank 0's 19 whole tiles" in last_error()
    assert lib.dsx_tileplan_blend_blocks(plan.handle) == 40 and plan.blend_blocks() == 40     # one segment, 40 rows
    assert lib.dsx_tileplan_blend_blocks(tile_plan((1, 300, 600), 32, 16).handle) == 3 * 128


def test_gather_canvas_refusals():
    lib = binding().lib
    plan = tile_plan((2, 40, 57), 16, 8)
    call = lambda h, f, s, c, Cn=2: lib.dsx_tileplan_gather_canvas(h, FAKE, Cn, f, s, c, FAKE, None)
    name = "tileplan_gather_canvas"
    for first, stride, count in ((plan.total, 1, 1), (0, 0, 2), (1, 2 ** 62, 3), (-1, 1, 1), (plan.total - 3, 1, 4),
                                 (1, 2, 29), (0, -1, 2)):
        assert call(plan.handle, first, stride, count) == ERR_INVALID, (first, stride, count)
        assert f"{name}: tiles {first} + k * {stride} ({count} of them) leave the plan (56 tiles)" in last_error()
    for count in (65536, -1):
        assert call(plan.handle, 0, 1, count) == ERR_INVALID and f"{name}: count = {count}" in last_error() and "65535" in last_error()
    assert call(None, 0, 1, 1) == ERR_INVALID and f"{name}: null argument" in last_error()
    assert call(plan.handle, 0, 1, 1, Cn=0) == ERR_INVALID and f"{name}: C = 0" in last_error()
    assert lib.dsx_tileplan_gather_canvas(plan.handle, None, 2, 0, 1, 1, FAKE, None) == ERR_INVALID and "null argument" in last_error()
    assert lib.dsx_tileplan_gather_canvas(plan.handle, FAKE, 2, 0, 1, 1, None, None) == ERR_INVALID and "null argument" in last_error()
    assert call(plan.handle, 0, 1, 0) == 0


# ----------------------------------------------------------------------------- the drivers' refusals, no rank, no device
def test_split_refuses_the_stitch_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfgs = {w: write_config(tmp_path, w) for w in ("sr3", "joint_indi")}

    def refused(argv, match, config="sr3"):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", cfgs[config]] + argv)

    solver = ["--solver", "ddim", "--solver-steps", "4"]
    refused(["--window", "hann"], "--window: only with --stitch blend")
    refused(["--window", "hann", "--stitch", "crop"], "--window: only with --stitch blend")
    refused(["--stitch", "blend", "--validate"], "--stitch blend.*--validate")
    refused(["--stitch", "blend", "--mix-t", "0.3", "--t-from", "given"], "--stitch blend.*--mix-t", config="joint_indi")
    refused(["--fuse-steps"], "--fuse-steps needs --solver")
    refused(["--fuse-steps", "--validate"], "--fuse-steps.*--validate")
    refused(["--fuse-steps", "--mix-t", "0.3", "--t-from", "given"], "--fuse-steps.*--mix-t", config="joint_indi")
    refused(["--fuse-steps", "--stitch", "crop"] + solver, "--fuse-steps with --stitch crop")
    refused(["--fuse-steps"] + solver, "--fuse-steps needs --sample-seed S and --noise-field")
    refused(["--fuse-steps", "--sample-seed", "3"] + solver, "--fuse-steps needs --sample-seed S and --noise-field")
    refused(["--fuse-steps", "--sample-seed", "3", "--noise-field", "--gpus", "2"] + solver, "--fuse-steps runs on one rank")
    refused(["--fuse-steps", "--sample-seed", "3", "--noise-field", "-gpu", "0,1"] + solver, "--fuse-steps runs on one rank")
    for bad in (["--stitch", "feather"], ["--stitch", "blend", "--window", "box"]):
        with pytest.raises(SystemExit):                               # argparse's own
            split.main(["-c", cfgs["sr3"]] + bad)


def test_predict_stack_refuses_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd import _lib, parallel
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tile_predict
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_tiled

    def touched(*a, **k):
        raise AssertionError("the refusal came too late")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(tile_predict, "TileExchange", touched)
    g, i, _ = cpu_samplers()

    class Stack:
        plan = tile_plan((2, 40, 57), 32, 16)

        def tiles(self, ids):
            touched()
    solver = dict(solver="ddim", steps=4, eta=0.0, spacing=None)
    ok = dict(solver=solver, noise="field", seed=3, fuse=True)
    for kw, match in ((dict(ok, solver=None), "fuse needs solver=.*ancestral"),
                      (dict(ok, noise="samples"), "fuse needs noise='field' and seed="),
                      (dict(ok, seed=None), "fuse needs noise='field' and seed="),
                      (dict(ok, stitch="crop"), "fuse with stitch='crop'"),
                      (dict(stitch="feather"), "stitch = 'feather': 'crop' or 'blend'"),
                      (dict(stitch="blend", window="box"), "window = 'box': one of triangle, hann")):
        with pytest.raises(DsxError, match="predict_stack: " + match):
            predict_stack(g, Stack(), **kw)
    with pytest.raises(DsxError, match="predict_stack: fuse: InDISampler is not a Gaussian sampler"):
        predict_stack(i, Stack(), noise="field", seed=3, fuse=True)
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(DsxError, match="predict_stack: fuse runs on one rank"):
        predict_stack(g, Stack(), **ok)
    with pytest.raises(DsxError, match="predict_tiled: stitch = 'feather'"):
        predict_tiled(i, torch.zeros(1, 40, 57), 32, stitch="feather")
