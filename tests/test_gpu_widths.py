"""The per-layer fp64 checks of tests/test_gpu_layers.py at channel widths other than 16, 32 and 64.

dsx_model_create accepts any inner_channel that is a positive multiple of 4 and any channel_mults; every golden model
has inner_channel in {16, 32, 64} and power-of-two multipliers, so every channel count the other GPU tests run is
16 2^k.  The models here (oracle/cases.py WIDTH_CASES: widths 20, 24, 40, 48, 96 with multipliers 3 and 5) reach what
those never do: the scalar epilogue of k_conv_mfma with bias, FiLM and residual, stage mode 2 on every 16-bit conv, K
tails, split-K counts that are no powers of two, N tails on the wide tiles, GroupNorm with 3, 5, 6, 9, 10, 12, 15 or
20 channels per group (k_chan_stats: the fused statistics need Cout % 16 == 0), k_temb at inner != 16 / 32 / 64 and
k_attn inside the net at head dimensions 48, 72, 80, 192 and 200.

Weights: oracle.weights.synth_state_dict over the engine's own parameter names and shapes.  Every plan is checked layer
by layer (tests/layer_check.py, the bounds of tests/layer_ref.py as they stand); the fp32 build is also compared end to
end with the oracle evaluated in float64, which sees what a per-layer check cannot: a skip wired to the wrong layer.
test_reach keeps a planner change from silently emptying these tests."""
import time

import pytest
import torch

from oracle import cases
from oracle.unet import unet_forward
from tests import nets
from tests.gpu_util import maxabs
from tests.layer_check import DT, check_plan, inputs, reach_tags
from tests.nets import dev  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3        # tests/test_gpu_parity.py: the project's figure for the fp32 build against the oracle
SEED = 37

# any grid fills the chip and the persistent kernel is off: tile128x128, 64x128 and 128x32 with N tails
_WIDE_TILES = {"DSX_MIN_GRID": "1", "DSX_WS": "0"}
_MANY_CHUNKS = {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4",
                "DSX_WS_C4_MIN": "4"}        # as in tests/test_gpu_layers.py

# id -> (case, dtype, env).  Every case in every operand type at default knobs.  (w20x3 is w20 with a 60-channel level:
# at widths 20, 40 and 80 no upsampling conv reads rows that are no whole 16-byte units, and test_reach asks for one.)
PLANS = {}
for _c in cases.WIDTH_CASES:
    for _d in ("bf16", "f16", "f32"):
        PLANS[f"{_c}_{_d}"] = (_c, _d, {})
for _c in ("w20", "w24", "w96"):
    # (f16 too: at default knobs no 16-bit plan of these models takes a tile 128 wide; test_reach asks for one per type)
    for _d in ("bf16", "f16", "f32"):
        PLANS[f"{_c}_{_d}_wide_tiles"] = (_c, _d, _WIDE_TILES)
for _c in ("w48", "w96"):
    PLANS[f"{_c}_bf16_many_chunk_ws"] = (_c, "bf16", _MANY_CHUNKS)

# What must have been checked, per operand type, after every plan ran (test_reach; tests/layer_check.py reach_tags
# derives them from the layer table).
REACH = ("scalar+resid", "scalar+film", "scalar nbase>0", "stage2+gn", "stage2+cat", "stage2 1x1", "stage2 s2",
         "stage2 up", "splitK odd", "ws ktail", "wide ntail", "cpg3", "cpg5+", "attn")
_F32_WHOLE_UNITS = "fp32: inner_channel % 4 == 0 makes every source a whole number of 16-byte units"
REACH_EXEMPT = {
    "f32": dict({t: _F32_WHOLE_UNITS for t in REACH if t.startswith("stage2")},
                **{"ws ktail": "fp32: k_conv_ws stages 16-channel chunks; every fp32 plan of these models that takes it "
                               "has Cin a multiple of its group (the dry run shows none)"}),
}

_CHECKED = {}          # plan -> {dtype, reach, layers, worst}
_SD = {}               # case -> state dict
_ORACLE = {}           # case -> float64 oracle output


def _case_inputs(name):
    case = cases.WIDTH_CASES[name]
    B = case["B"]
    # ddpm flavour: one scalar t for the batch (w20, w20x3) and one per image (w40), as the golden ddpm cases have them
    ddpm_t = torch.tensor([0.37]) if name.startswith("w20") else torch.tensor([3.0, 1700.0][:B])
    return inputs(case, B, case["H"], case["W"], ddpm_t=ddpm_t)


def _state_dict(name):
    if name not in _SD:
        _SD[name] = nets.engine_state_dict(cases.WIDTH_CASES[name], SEED)
    return _SD[name]


def _oracle64(name):
    if name not in _ORACLE:
        case = cases.WIDTH_CASES[name]
        x, t = _case_inputs(name)
        sd64 = {k: v.double() for k, v in _state_dict(name).items()}
        _ORACLE[name] = unet_forward(sd64, case["cfg"], case["flavour"], x.double(), t.double())
    return _ORACLE[name]


@pytest.mark.parametrize("plan", list(PLANS))
def test_every_layer_against_fp64(plan, dev, monkeypatch):
    t0 = time.time()
    name, dt, env = PLANS[plan]
    case = cases.WIDTH_CASES[name]
    x, t = _case_inputs(name)
    res = check_plan(plan, case, _state_dict(name), dt, case["B"], case["H"], case["W"], env, x, t, dev, monkeypatch)
    groups = case["cfg"]["norm_groups"]
    reach = set()
    for L in res["table"]:
        reach |= reach_tags(L, dt, groups)
    _CHECKED[plan] = dict(dtype=dt, reach=reach, layers=res["layers"], worst=res["worst"])
    torch.cuda.empty_cache()
    print(f"{plan}: {time.time() - t0:.1f} s; reaches {sorted(reach)}")


@pytest.mark.parametrize("name", list(cases.WIDTH_CASES))
def test_fp32_forward_against_fp64_oracle(name, dev):
    """End to end: the per-layer checks read what each launch read, so a skip connection wired to the wrong layer
    passes them all; the whole forward against the oracle in float64 does not.  (The oracle's own fp32-against-fp64
    difference at these models is <= 2.4e-6 with max|y| 2.6 .. 4.1: three orders below the tolerance.  No 16-bit
    threshold: the wiring is planner code that does not depend on the operand type.)"""
    from tests.gpu_util import build_engine
    case = cases.WIDTH_CASES[name]
    x, t = _case_inputs(name)
    ref = _oracle64(name)
    eng = build_engine(case["cfg"], case["flavour"], _state_dict(name), dtype="f32")
    y = eng.forward(x.to(dev), t.to(dev)).cpu()
    assert eng.handoff_timeouts() == 0
    err = maxabs(y, ref)
    print(f"\n{name}: max|hip - oracle64| = {err:.3e}, max|y| = {float(ref.abs().max()):.2f}")
    assert tuple(y.shape) == tuple(ref.shape)
    assert err <= FP32_TOL, err


def test_reach():
    """every reach condition was met by a checked launch in every operand type that can meet it (runs after the plans;
    skipped when only some of them ran, e.g. with -k)"""
    if set(PLANS) - set(_CHECKED):
        pytest.skip("needs every plan of this module checked in this session; missing: "
                    f"{sorted(set(PLANS) - set(_CHECKED))}")
    by_dt = {}
    for v in _CHECKED.values():
        by_dt.setdefault(v["dtype"], set()).update(v["reach"])
    print("\n" + "\n".join(f"{d}: {sorted(t)}" for d, t in sorted(by_dt.items())))
    for d in DT:
        missing = set(REACH) - set(REACH_EXEMPT.get(d, {})) - by_dt.get(d, set())
        assert not missing, f"{d}: never reached: {sorted(missing)}"
