"""The per-layer fp64 checks of tests/test_gpu_layers.py at map shapes off the 8 x 8 tile grid.

The tile of an MFMA conv follows from its output map (tile_geometry in dsx_plan.cpp): TW = the largest power of two
<= 16 that divides Wo, TH = the largest <= BM / TW that divides Ho, TB = BM / (TW TH) images per tile.  Every model the
other GPU tests run has maps whose sides are multiples of 8 (or 4 x 4 / 12 x 20 at the bottom) and never H > W, so they
run tiles 16x4x1, 8x8x1, 4x8x2, 4x4x4 and their 128- and 256-pixel counterparts and nothing else.  The sizes here
(oracle/cases.py SHAPE_CASES: 64x48, 64x24, 128x24, 48x32, 24x64 at B = 3) give maps 12, 6, 4 and 2 pixels wide and
tiles 4x16x1, 2x32x1, 2x16x2, 8x4x2, 16x2x2 (x2 / x4 images on the 128-pixel tile): other staging plans, other A-fragment
addressing (abase, a16, p16) and other epilogue pixel maps in k_conv_mfma, k_conv_ws and the split-K path; patches
exactly at the staging cap (2x16x2 and 16x2x2: 144 pixels; k_conv_ws 8x16x1: 180); multi-image tiles whose last tile
misses images; stride-2 convs on all five; the first conv off k_conv_first at default knobs (Wo % 16 != 0).

Every plan is checked layer by layer (tests/layer_check.py, the bounds of tests/layer_ref.py as they stand); the fp32
build is also compared end to end with the oracle in float64, which sees what a per-layer check cannot: a skip or an
up / down path wired for the wrong size.  test_reach keeps a planner change from silently emptying these tests; what each
plan reaches is pinned without a GPU by tests/test_planner_cpu.py (test_shape_plans_reach_their_geometry_classes)."""
import time

import pytest
import torch

from oracle import cases
from oracle.unet import unet_forward
from oracle.weights import synth_state_dict
from tests.gpu_util import maxabs
from tests.layer_check import DT, check_plan, geom_tag, inputs
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3        # tests/test_gpu_parity.py, tests/test_gpu_widths.py: the fp32 build against the oracle
SEED = 37              # w20's synthetic weights, as in tests/test_gpu_widths.py

# any grid fills the chip and the persistent kernel is off: the 128-pixel tiles, two and four images per tile
_WIDE_TILES = {"DSX_MIN_GRID": "1", "DSX_WS": "0"}
_MANY_CHUNKS = {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4",
                "DSX_WS_C4_MIN": "4"}        # as in tests/test_gpu_layers.py: k_conv_ws on the 128-pixel tile
_SPLITK = {"DSX_MIN_GRID": "100000", "DSX_WS": "0"}

# id -> (case, dtype, B, env)
PLANS = {}
for _c in cases.SHAPE_CASES:
    for _d in DT:
        PLANS[f"{_c}_{_d}"] = (_c, _d, 3, {})
for _c, _v in cases.SHAPE_CASES.items():
    if _v["model"] in ("sr3_tiny", "w20"):
        for _d in DT:
            PLANS[f"{_c}_{_d}_wide_tiles"] = (_c, _d, 3, _WIDE_TILES)
# (ddpm_tiny's 32-channel level on the slim 128 x 32 tile: the only plain 3 x 3 launches at 4x32x1 and 16x4x2 -- in
# sr3_tiny and w20 that level is wider than 32 channels and takes the 64-pixel tile first)
for _s in ("128x24", "24x64"):
    for _d in DT:
        PLANS[f"ddpm_tiny_{_s}_{_d}_wide_tiles"] = (f"ddpm_tiny_{_s}", _d, 3, _WIDE_TILES)
for _m in ("ddpm_tiny", "sr3_tiny"):
    for _s in ("64x48", "64x24", "128x24"):
        for _d in DT:
            PLANS[f"{_m}_{_s}_{_d}_many_chunk_ws"] = (f"{_m}_{_s}", _d, 3, _MANY_CHUNKS)
for _h, _w in cases.SHAPE_SIZES:
    PLANS[f"sr3_tiny_{_h}x{_w}_f32_splitk"] = (f"sr3_tiny_{_h}x{_w}", "f32", 3, _SPLITK)   # stride 2 under split-K
# one image on two-image tiles (2x16x2 on the 16 x 6 maps): half of every such tile is empty
PLANS["ddpm_tiny_64x24_b1_bf16"] = ("ddpm_tiny_64x24", "bf16", 1, {})
PLANS["ddpm_tiny_64x24_b1_f32"] = ("ddpm_tiny_64x24", "f32", 1, {})

# The geometry classes (tests/layer_check.py geom_tag, less its +tail suffix) that the union over the operand types must
# contain.  What each operand type must contain is REACH_BY_DTYPE, which tests/test_planner_cpu.py holds equal to what
# the planner's dry run of these very plans gives.
_NARROW5 = ("2x16x2", "2x32x1", "4x16x1", "8x4x2", "16x2x2")


def _classes(fam, size, tiles, bm):
    return {f"{fam} {size} {t}@{bm}" for t in tiles}


REACH = (_classes("mfma", "1x1", _NARROW5, 64)
         | _classes("mfma", "1x1", ("2x16x4", "2x32x2", "4x16x2", "4x32x1", "8x4x4", "16x2x4", "16x4x2"), 128)
         | _classes("mfma", "3x3", _NARROW5, 64) | _classes("mfma", "3x3", ("4x16x2", "4x32x1", "16x4x2"), 128)
         | _classes("mfma", "3x3 up", ("4x16x1",), 64) | _classes("mfma", "3x3 up", ("4x32x1", "16x4x2"), 128)
         | _classes("mfma", "3x3 s2", _NARROW5, 64)
         | _classes("g2", "3x3", ("4x32x1", "16x8x1"), 128)
         | _classes("splitK", "1x1", _NARROW5, 64) | _classes("splitK", "3x3", _NARROW5, 64)
         | _classes("splitK", "3x3 up", ("4x16x1",), 64) | _classes("splitK", "3x3 s2", _NARROW5, 64)
         | _classes("ws", "1x1", ("2x32x1", "4x16x1"), 64) | _classes("ws", "1x1", ("4x32x1", "8x16x1"), 128)
         | _classes("ws", "3x3", ("4x16x1",), 64) | _classes("ws", "3x3", ("8x16x1",), 128)
         | _classes("ws", "3x3 up", ("4x16x1",), 64))
# multi-image tiles whose last tile misses images (B = 3 on two- and four-image tiles), with their suffix
REACH_TAILS = ({c + "+tail" for c in _classes("mfma", "3x3", ("8x4x2", "2x16x2", "16x2x2"), 64)}
               | {c + "+tail" for c in _classes("mfma", "1x1", ("2x16x4", "2x32x2", "4x16x2", "8x4x4", "16x2x4", "16x4x2"),
                                                128)})

_CHECKED = {}          # plan -> {dtype, geom, layers, worst}
_SD = {}               # model -> state dict
_ORACLE = {}           # case -> float64 oracle output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _case_inputs(name, B=3):
    case = cases.SHAPE_CASES[name]
    # ddpm flavour: one scalar t for the whole batch, as the golden ddpm_tiny case and w20 have it
    return inputs(case, B, case["H"], case["W"], ddpm_t=torch.tensor([0.37]))


def _state_dict(model):
    if model not in _SD:
        if model == "w20":
            from diffsplitting_amd import engine
            case = cases.SHAPE_MODELS[model]
            cfg = case["cfg"]
            eng = engine.UNetEngine(engine.make_cfg(case["flavour"], cfg["in_channel"], cfg["out_channel"],
                                                    cfg["inner_channel"], cfg["norm_groups"], cfg["channel_mults"],
                                                    cfg["attn_res"], cfg["res_blocks"], cfg["image_size"]), case["flavour"])
            _SD[model] = synth_state_dict(zip(eng.param_names, eng.param_shapes), seed=SEED)
        else:
            _SD[model] = golden_state_dict("unet_" + model)[0]
    return _SD[model]


def _oracle64(name):
    if name not in _ORACLE:
        case = cases.SHAPE_CASES[name]
        x, t = _case_inputs(name)
        sd64 = {k: v.double() for k, v in _state_dict(case["model"]).items()}
        _ORACLE[name] = unet_forward(sd64, case["cfg"], case["flavour"], x.double(), t.double())
    return _ORACLE[name]


@pytest.mark.parametrize("plan", list(PLANS))
def test_every_layer_against_fp64(plan, dev, monkeypatch):
    t0 = time.time()
    name, dt, B, env = PLANS[plan]
    case = cases.SHAPE_CASES[name]
    x, t = _case_inputs(name, B)
    res = check_plan(plan, case, _state_dict(case["model"]), dt, B, case["H"], case["W"], env, x, t, dev, monkeypatch)
    geom = {geom_tag(L) for L in res["table"]} - {None}
    _CHECKED[plan] = dict(dtype=dt, geom=geom, layers=res["layers"], worst=res["worst"])
    torch.cuda.empty_cache()
    print(f"{plan}: {time.time() - t0:.1f} s; geometry classes {sorted(geom)}")


@pytest.mark.parametrize("name", list(cases.SHAPE_CASES))
def test_fp32_forward_against_fp64_oracle(name, dev):
    """End to end: the per-layer checks read what each launch read, so a skip connection or an up / down path wired for
    the wrong size passes them all; the whole forward against the oracle in float64 does not.  (The oracle's own
    fp32-against-fp64 difference at these models and sizes is recorded in DESIGN.md item 38: orders below the tolerance.
    No 16-bit threshold: the wiring is planner code that does not depend on the operand type.)"""
    from tests.gpu_util import build_engine
    case = cases.SHAPE_CASES[name]
    x, t = _case_inputs(name)
    ref = _oracle64(name)
    eng = build_engine(case["cfg"], case["flavour"], _state_dict(case["model"]), dtype="f32")
    y = eng.forward(x.to(dev), t.to(dev)).cpu()
    assert eng.handoff_timeouts() == 0
    err = maxabs(y, ref)
    print(f"\n{name}: max|hip - oracle64| = {err:.3e}, max|y| = {float(ref.abs().max()):.2f}")
    assert tuple(y.shape) == tuple(ref.shape)
    assert err <= FP32_TOL, err


def reach_by_dtype():
    """dtype -> the classes its plans must reach (tests/golden/shape_reach.json): tests/test_planner_cpu.py asserts that
    this equals what the planner's dry run of PLANS gives, so the table cannot drift from the planner unnoticed"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_reach.json")) as f:
        return {d: set(v) for d, v in json.load(f).items()}


def test_reach():
    """every required geometry class was met by a checked launch: the union over the operand types holds REACH and
    REACH_TAILS, each operand type holds every class the CPU pin says its plans reach (runs after the plans; skipped
    when only some of them ran, e.g. with -k)"""
    if set(PLANS) - set(_CHECKED):
        pytest.skip("needs every plan of this module checked in this session; missing: "
                    f"{sorted(set(PLANS) - set(_CHECKED))}")
    by_dt = {}
    for v in _CHECKED.values():
        by_dt.setdefault(v["dtype"], set()).update(v["geom"])
    print("\n" + "\n".join(f"{d}: {sorted(t)}" for d, t in sorted(by_dt.items())))
    union = set().union(*by_dt.values())
    missing = REACH - {t.replace("+tail", "") for t in union}
    assert not missing, f"never reached: {sorted(missing)}"
    assert not REACH_TAILS - union, f"never reached: {sorted(REACH_TAILS - union)}"
    for d, want in reach_by_dtype().items():
        missing = set(want) - by_dt.get(d, set())
        assert not missing, f"{d}: never reached: {sorted(missing)}"
