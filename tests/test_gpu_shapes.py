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
from tests import nets
from tests.gpu_util import maxabs
from tests.layer_check import check_plan, geom_tag, inputs
from tests.nets import dev  # noqa: F401  (the fixture)
from tests.plan_cases import SHAPE_PLANS as PLANS, SHAPE_REACH as REACH, SHAPE_REACH_TAILS as REACH_TAILS
from tests.plan_cases import shape_reach_by_dtype as reach_by_dtype
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3        # tests/test_gpu_parity.py, tests/test_gpu_widths.py: the fp32 build against the oracle
SEED = 37              # w20's synthetic weights, as in tests/test_gpu_widths.py

_CHECKED = {}          # plan -> {dtype, geom, layers, worst}
_SD = {}               # model -> state dict
_ORACLE = {}           # case -> float64 oracle output


def _case_inputs(name, B=3):
    case = cases.SHAPE_CASES[name]
    # ddpm flavour: one scalar t for the whole batch, as the golden ddpm_tiny case and w20 have it
    return inputs(case, B, case["H"], case["W"], ddpm_t=torch.tensor([0.37]))


def _state_dict(model):
    if model not in _SD:
        if model == "w20":
            _SD[model] = nets.engine_state_dict(cases.SHAPE_MODELS[model], SEED)
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
