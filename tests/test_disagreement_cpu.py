"""Tile disagreement without a GPU: the two entry points against header and binding, dsx_tileplan_crop_lines against brute
force, the numpy restatement of the contract (tests/disagreement_ref.py) against closed forms and against the typical
mistakes it must reject, every host refusal of dsx_tileplan_disagreement with fake device pointers, and the refusals of
the drivers and of ``split`` by message, with no rank started."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import blend_ref
from tests import disagreement_ref as ref
from tests.host_checks import BLEND_PLANS, ERR_INVALID, FAKE, binding, cpu_samplers, last_error, tile_plan
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsx_tileplan_crop_lines": 4, "dsx_tileplan_disagreement": 9}
OVERLAPPING = [p for p in BLEND_PLANS if p != ((1, 32, 32), 32, 32)]


def random_tiles(plan, Cn, seed=11):
    return np.random.default_rng(seed).standard_normal((plan.total, Cn) + plan.patch_shape[1:]).astype(np.float32)


def test_the_entry_points_are_declared_bound_and_exported():
    lib = binding()
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name, n in NEW.items():
        assert re.search(rf"\bint {name}\(", header), name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n and hasattr(lib._cdll, name)
    assert lib.lib.dsx_abi_version() == 2 and re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", header)
    from diffsplitting_amd.data import tiling
    assert callable(tiling.TilePlan.crop_lines) and callable(tiling.TilePlan.disagreement)


@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_crop_lines_against_brute_force(shape, patch, grid):
    plan = tile_plan(shape, patch, grid)
    for band in (1, 3, 8, 64):
        rows, cols = plan.crop_lines(band)
        want_rows, want_cols = ref.near_masks(plan, band)
        assert rows.dtype == np.uint8 and rows.shape == (shape[1],) and cols.shape == (shape[2],)
        assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols), band
    lines = ref.crop_lines(plan)
    if plan.total == 1:
        assert lines == ([], []) and not plan.crop_lines(8)[0].any() and not plan.crop_lines(8)[1].any()
    else:
        rows, cols = plan.crop_lines(1)                                 # band 1: the line and the pixel before it
        assert sorted(set(np.flatnonzero(rows))) == sorted({v for L in lines[0] for v in (L - 1, L)})
        assert sorted(set(np.flatnonzero(cols))) == sorted({v for L in lines[1] for v in (L - 1, L)})


def test_crop_lines_refusals():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tiling
    lib = binding().lib
    plan = tile_plan((1, 40, 56), 32, 16)
    rows, cols = np.zeros(40, dtype=np.uint8), np.zeros(56, dtype=np.uint8)
    for band in (0, -1, 65536):
        assert lib.dsx_tileplan_crop_lines(plan.handle, band, rows, cols) == ERR_INVALID
        assert f"tileplan_crop_lines: band = {band}, must be in 1..65535" in last_error()
        with pytest.raises(DsxError, match="tileplan_crop_lines: band"):
            plan.crop_lines(band)
    assert lib.dsx_tileplan_crop_lines(plan.handle, 65535, rows, cols) == 0
    for args in ((None, 8, rows, cols), (plan.handle, 8, None, cols), (plan.handle, 8, rows, None)):
        assert lib.dsx_tileplan_crop_lines(*args) == ERR_INVALID and "tileplan_crop_lines: null argument" in last_error()
    trim = tiling.TilePlan((1, 40, 56), (1, 16, 16), (1, 32, 32), mode=tiling.TRIM)
    with pytest.raises(DsxError, match="tileplan_crop_lines: the plan's tiles do not cover the frames"):
        trim.crop_lines()


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,patch,grid", BLEND_PLANS, ids=str)
def test_tiles_cut_from_one_frame_do_not_disagree(shape, patch, grid):
    plan = tile_plan(shape, patch, grid)
    frame = np.random.default_rng(5).standard_normal(plan.data_shape + (2,)).astype(np.float32)
    smap, sc = ref.disagreement_ref(plan, blend_ref.cut_tiles(plan, frame), band=8)
    assert smap.dtype == np.float32 and not smap.any()
    assert not sc["sum_var"].any() and not sc["bound"].any()
    if plan.total == 1:
        assert not sc["count"].any() and np.isnan(sc["rms_pair"]).all()
        assert np.isposinf(sc["min_var"]).all() and np.isneginf(sc["max_var"]).all()
    else:
        assert (sc["count"][..., 0] > 0).all() and (sc["count"][..., 1] > 0).all()
        assert (sc["count"][..., 1] <= sc["count"][..., 0]).all()
        assert not sc["min_var"].any() and not sc["max_var"].any() and not sc["rms_pair"].any()


def _contributors(plan, n, y, x):
    ph, pw = plan.patch_shape[1:]
    return [t for t, (m, y0, x0) in enumerate(plan.patch_start) if m == n and y0 <= y < y0 + ph and x0 <= x < x0 + pw]


@pytest.mark.parametrize("shape,patch,grid", OVERLAPPING, ids=str)
def test_the_restatement_against_closed_forms(shape, patch, grid):
    plan = tile_plan(shape, patch, grid)
    tiles = random_tiles(plan, 2)
    var, k = ref.variance(plan, tiles)
    N, H, W = plan.data_shape
    rng = np.random.default_rng(3)
    seen = set()
    pixels = [(0, int(rng.integers(H)), int(rng.integers(W))) for _ in range(200)] + [(0, 0, 0), (0, H - 1, W - 1)]
    for n, y, x in pixels:
        ts = _contributors(plan, n, y, x)
        assert len(ts) == k[n, y, x]
        seen.add(len(ts))
        for c in range(2):
            v = np.array([tiles[t][c, y - plan.patch_start[t][1], x - plan.patch_start[t][2]] for t in ts], dtype=np.float64)
            got = var[n, y, x, c]
            if len(v) == 1:
                assert got == 0.0
                continue
            if len(v) == 2:                   # exactly (v1 - v2)^2 / 2: d and d / 2 are exact, d * (d / 2) rounds once
                assert got == (v[0] - v[1]) * (v[0] - v[1]) / 2
            assert abs(got - np.var(v, ddof=1)) <= 1e-12 * got
            pairs = [(a - b) ** 2 for a, b in itertools.combinations(v.tolist(), 2)]
            assert abs(np.mean(pairs) - 2 * got) <= 1e-12 * 2 * got
    assert 1 in seen and 2 in seen and max(seen) >= 4
    assert k.max() == max(len(_contributors(plan, 0, y, x)) for y in range(H) for x in range(W))


@pytest.mark.parametrize("shape,patch,grid", [((1, 40, 56), 32, 16), ((1, 37, 50), 24, 8), ((1, 45, 70), 30, 10)], ids=str)
@pytest.mark.parametrize("kind", ref.MISTAKES)
def test_the_contract_rejects_the_typical_mistakes(shape, patch, grid, kind):
    plan = tile_plan(shape, patch, grid)
    tiles = random_tiles(plan, 2)
    for band in (1, 8):
        want_map, want = ref.disagreement_ref(plan, tiles, band)
        assert ref.within_contract(want_map, want, want_map, want)
        got_map, got = ref.mistaken(plan, tiles, band, kind, window=blend_ref.window_pair(plan, "triangle"))
        if kind in ("band_late", "band_short") and band >= 8 and want["count"][0, 0, 0] == want["count"][0, 0, 1]:
            continue                                                  # the band already holds every overlap pixel
        assert not ref.within_contract(got_map, got, want_map, want), (kind, band)


def test_the_bound_is_a_few_ulp_and_rejects_a_dropped_pixel():
    plan = tile_plan((1, 64, 96), 32, 16)
    tiles = random_tiles(plan, 1)
    var, k = ref.variance(plan, tiles)
    _, sc = ref.disagreement_ref(plan, tiles, 8)
    m, T = sc["count"][0, 0, 0], sc["sum_var"][0, 0, 0]
    assert sc["bound"][0, 0, 0] == (m + 1) * ref.U * T and sc["bound"][0, 0, 0] < 1e-12 * T
    terms = var[0, :, :, 0][k[0] >= 2]
    assert abs(float(np.sum(terms)) - T) <= sc["bound"][0, 0, 0]                    # numpy's pairwise order
    assert abs(float(np.cumsum(terms)[-1]) - T) <= sc["bound"][0, 0, 0]             # one after the other
    assert abs(float(np.sum(np.sort(terms)[1:])) - T) > sc["bound"][0, 0, 0]        # the smallest term left out


# ----------------------------------------------------------------------------- host refusals, no device
def _call(h, tiles=FAKE, Cn=1, world=1, stride=0, band=8, smap=None, part=FAKE):
    return binding().lib.dsx_tileplan_disagreement(h, tiles, Cn, world, stride, band, smap, part, None)


def test_disagreement_refusals():
    from diffsplitting_amd.data import tiling
    name = "tileplan_disagreement"
    plan = tile_plan((2, 40, 57), 16, 8)                                # never given a window: none is needed
    for kw in (dict(tiles=None), dict(part=None)):
        assert _call(plan.handle, **kw) == ERR_INVALID and f"{name}: null argument" in last_error()
    assert _call(None) == ERR_INVALID and f"{name}: null argument" in last_error()
    for Cn in (0, -1, 5):
        assert _call(plan.handle, Cn=Cn) == ERR_INVALID and f"{name}: C = {Cn}, must be in 1..4" in last_error()
    for band in (0, -3, 65536):
        assert _call(plan.handle, band=band) == ERR_INVALID and f"{name}: band = {band}, must be in 1..65535" in last_error()
    assert _call(plan.handle, world=0) == ERR_INVALID and f"{name}: world = 0" in last_error()
    need = 19 * 2 * 16 * 16                                             # 56 tiles over 3 ranks: rank 0 holds 19
    for stride in (need - 1, 0, -5):
        assert _call(plan.handle, Cn=2, world=3, stride=stride) == ERR_INVALID
        assert f"{name}: rank_stride_elems = {stride} is smaller than rank 0's 19 whole tiles" in last_error()
    trim = tiling.TilePlan((1, 40, 56), (1, 16, 16), (1, 32, 32), mode=tiling.TRIM)
    assert _call(trim.handle) == ERR_INVALID and f"{name}: the plan's tiles do not cover the frames" in last_error()
    deep = tiling.TilePlan((4, 40, 56), (2, 16, 16), (2, 32, 32))      # two frames per tile
    assert _call(deep.handle) == ERR_INVALID and f"{name}: the plan's tiles do not cover the frames" in last_error()
    big = tile_plan((1, 40000, 40000), 30000, 10000)                   # C * ph * pw beyond 32 bits
    assert _call(big.handle, Cn=3) == ERR_INVALID and f"{name}: C * patch" in last_error()


# ----------------------------------------------------------------------------- the drivers' refusals, no rank, no device
def test_the_drivers_refuse_by_name_before_any_launch(monkeypatch):
    from diffsplitting_amd import _lib, parallel
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import tile_predict
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames

    def touched(*a, **k):
        raise AssertionError("the refusal came too late")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(tile_predict, "TileExchange", touched)
    g, i, j = cpu_samplers()

    class Stack:
        plan = tile_plan((2, 40, 57), 32, 16)

        def tiles(self, ids):
            touched()
    for kw, match in ((dict(disagreement="map"), "disagreement = 'map': False, 'sums' or True"),
                      (dict(disagreement=1), "disagreement = 1: False, 'sums' or True"),
                      (dict(disagreement=True, seam_band=0), "seam_band = 0: an integer in 1..65535"),
                      (dict(disagreement="sums", seam_band=65536), "seam_band = 65536: an integer in 1..65535"),
                      (dict(disagreement=True, seam_band=2.5), "seam_band = 2.5: an integer in 1..65535")):
        with pytest.raises(DsxError, match="predict_stack: " + match):
            predict_stack(g, Stack(), **kw)
        with pytest.raises(DsxError, match="predict_stack_frames: " + match):
            predict_stack_frames(i, Stack(), seed=3, **kw)
    solver = dict(solver="ddim", steps=4, eta=0.0, spacing=None)
    with pytest.raises(DsxError, match="predict_stack: disagreement=True on fuse=True with samples = 2.*'sums'"):
        predict_stack(g, Stack(), solver=solver, noise="field", seed=3, fuse=True, samples=2, disagreement=True)
    with pytest.raises(DsxError, match="predict_stack_frames: disagreement=True on the frame-state path with samples = 3"):
        predict_stack_frames(j, Stack(), seed=3, samples=3, disagreement=True)
    monkeypatch.setattr(type(g), "prediction_channels", property(lambda self: 5))
    with pytest.raises(DsxError, match="predict_stack: disagreement: 5 prediction channels, the measure takes 1..4"):
        predict_stack(g, Stack(), disagreement="sums")


def test_split_refuses_the_seam_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfgs = {w: write_config(tmp_path, w) for w in ("sr3", "indi", "joint_indi")}
    cfgs["colour"] = write_config(tmp_path, "indi", train={"name": "cifar10", "batch_size": 3, "datapath": "none"},
                                  val={"name": "cifar10", "datapath": "none"})

    def refused(argv, match, config="sr3"):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", cfgs[config]] + argv)

    R = ["--seam-report", str(tmp_path / "seam.json")]
    M = ["--seam-map", str(tmp_path / "seam.npy")]
    refused(M, "--seam-map: only with --seam-report FILE.json")
    refused(["--seam-band", "4"], "--seam-band: only with --seam-report FILE.json")
    refused(["--seam-report", "seam.txt"], "--seam-report seam.txt: a .json file")
    refused(R + ["--seam-map", "seam.png"], "--seam-map seam.png: a .npy or .tif file")
    refused(R + ["--seam-band", "0"], "--seam-band 0: 1..65535 pixels")
    refused(R + ["--seam-band", "65536"], "--seam-band 65536: 1..65535 pixels")
    refused(R + ["--validate"], "--seam-report .*not with --validate")
    refused(R + ["--mix-t", "0.3", "--t-from", "given"], "--seam-report: not with --mix-t", config="joint_indi")
    refused(R + ["--datapath"], "--seam-report .*colour items of a cifar10 config are not tiled", config="colour")
    solver = ["--solver", "ddim", "--solver-steps", "4", "--sample-seed", "3", "--noise-field"]
    refused(R + M + ["--fuse-steps", "--samples", "2"] + solver, "--seam-map with --fuse-steps and --samples 2")
    refused(R + M + ["--frame-steps", "--samples", "3", "--sample-seed", "3"], "--seam-map with --frame-steps and --samples 3",
            config="indi")
