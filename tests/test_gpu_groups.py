"""The per-layer fp64 checks of tests/test_gpu_layers.py at GroupNorm groups wider than 64 channels.

dsx_model_create accepts any norm_groups >= 1 that divides every channel count, concatenated counts included, and the
reference's GroupNorm(groups, dim) runs norm_groups = 1 or 2 without comment; every other model of the suite has at most
40 channels per group.  The models here (oracle/cases.py GROUP_CASES: norm_groups 1, 2 and 3, 8 .. 512 channels per
group) reach what those never do: the tail loop of gn_finalize_item ("groups wider than the workgroup") in each of its
three hosts -- k_gn_finalize (64 threads) above 64 channels per group, k_gn_finalize_wide (256 threads) above 256, the
finalize that a residual 1 x 1 k_conv_ws launch hosts above 64 --, the waves 1 .. 3 of k_gn_finalize_wide owning a
channel, accumulate() with more than 64 channels of a group in one source of a concat and the rest in the other, with
fp32 and with pivot-shifted partials, and the plans the 8 x 8 level takes when k_conv_img turns its GroupNorm away
(more than 64 channels per group, or a count that is no power of two).

Weights: oracle.weights.synth_state_dict over the engine's own parameter names and shapes.  Every plan is checked layer
by layer (tests/layer_check.py, the bounds of tests/layer_ref.py as they stand); which kernel finalized a GroupNorm is
not in the layer table, so every plan also writes its DSX_PLAN_DUMP and the reach conditions are read from the dumped
launches (layer_check.group_reach_tags; tests/test_groups_plan_cpu.py establishes the same reach without a GPU).  The
fp32 build is also compared end to end with the oracle evaluated in float64.

Flat plans: the weights are the synthetic ones with a uniform background written in.  With one, two or three groups a map
is flat for GroupNorm only if its channels agree, which synthetic biases never do (|mean| / std stays below 0.5 in
every group of these models).  In the two bottleneck blocks the first conv's weights are scaled to 1e-3 under a FiLM
vector that is the same in every channel (FLAT_LEVEL), for the output channels of the first group (the other groups keep
the maps behind the block from being one value per channel).  The second GroupNorm of those blocks then has
|mean| / std > 1e3 on partials shifted by bias + FiLM (the split-K reduce; g3: k_chan_stats) in a group of 256 (g1),
128 (g2) or 48 (g3) channels; test_flat_reach asks for that.  In f32 the input is 1e-4 randn as well
(layer_check.inputs, flat) and the first conv's bias is FLAT_LEVEL in every channel: the first GroupNorm is as flat, on
partials shifted by the bias (k_conv_first; g3: k_chan_stats).  In bf16 the input and that bias are the ordinary ones: a level of 8 under
1e-4 is 8.0 in every pixel once stored in bf16, a GroupNorm over 8 or more channels does not bring the pixels apart
again as one channel per group does, so every map behind it is one value per channel and the store's rounding errors
are copies of B * C values -- Verdict's mean and slope bounds take them for independent and stand sqrt(H W) too low
(measured, g1: |mean(y - r)| 8.0e-4 against 7.6e-4, slope 3.7e-4 against 1.8e-4 at the first stride-2 conv, every
element inside half an ulp).  That is the input's doing, not a kernel's."""
import re
import time

import pytest
import torch

from oracle import cases
from oracle.unet import unet_forward
from tests import nets
from tests.gpu_util import maxabs
from tests.layer_check import DT, check_plan, group_reach_tags, inputs
from tests.nets import dev  # noqa: F401  (the fixture)
from tests.plan_cases import GROUP_PLANS as PLANS, GROUP_REACH as REACH, GROUP_REACH_EXEMPT as REACH_EXEMPT
from tests.plan_dump import read_dump

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3        # tests/test_gpu_parity.py: the project's figure for the fp32 build against the oracle
SEED = 37
FLAT_LEVEL = 8.0       # the uniform background of the flat plans: |mean| / std <= 8 / sqrt(eps) = 2530

_CHECKED = {}          # plan -> {dtype, reach, layers, worst, flat_wide}
_SD = {}               # case -> state dict
_ORACLE = {}           # case -> float64 oracle output


def case_inputs(name, flat=False):
    case = cases.GROUP_CASES[name]
    # ddpm flavour: one t per image (g1) and one scalar t for the batch (g3), as the golden ddpm cases have them
    ddpm_t = torch.tensor([3.0, 1700.0, 41.0]) if name == "g1" else torch.tensor([0.37])
    return inputs(case, case["B"], case["H"], case["W"], flat=flat, ddpm_t=ddpm_t)


def state_dict(name):
    """synthetic weights for the engine's own parameter table (no fixture: the engine names its parameters)"""
    if name not in _SD:
        _SD[name] = nets.engine_state_dict(cases.GROUP_CASES[name], SEED)
    return _SD[name]


def flat_state_dict(name, first_conv):
    """the synthetic weights with a uniform background (see the module's docstring): bottleneck blocks, the channels of
    the first group: first conv weights x 1e-3, its bias 0, the block's FiLM vector = FLAT_LEVEL; `first_conv`: the
    first conv's bias = FLAT_LEVEL in every channel"""
    case = cases.GROUP_CASES[name]
    sd = dict(state_dict(name))
    if first_conv:
        sd["downs.0.bias"] = torch.full_like(sd["downs.0.bias"], FLAT_LEVEL)
    film = "noise_func.noise_func.0" if case["flavour"] == "sr3" else "mlp.1"
    blocks = sorted({m.group(1) for m in (re.match(r"(mid\.\d+\.res_block)\.", k) for k in sd) if m})
    assert len(blocks) == 2, blocks
    for rb in blocks:
        w, b = sd[f"{rb}.block1.block.3.weight"].clone(), sd[f"{rb}.block1.block.3.bias"].clone()
        fw, fb = sd[f"{rb}.{film}.weight"].clone(), sd[f"{rb}.{film}.bias"].clone()
        cpg = w.shape[0] // case["cfg"]["norm_groups"]
        w[:cpg] *= 1e-3
        b[:cpg] = 0.0
        fw[:cpg] = 0.0
        fb[:cpg] = FLAT_LEVEL
        sd.update({f"{rb}.block1.block.3.weight": w, f"{rb}.block1.block.3.bias": b, f"{rb}.{film}.weight": fw,
                   f"{rb}.{film}.bias": fb})
    return sd


def _oracle64(name):
    if name not in _ORACLE:
        case = cases.GROUP_CASES[name]
        x, t = case_inputs(name)
        sd64 = {k: v.double() for k, v in state_dict(name).items()}
        _ORACLE[name] = unet_forward(sd64, case["cfg"], case["flavour"], x.double(), t.double())
    return _ORACLE[name]


@pytest.mark.parametrize("plan", list(PLANS))
def test_every_layer_against_fp64(plan, dev, monkeypatch, tmp_path):
    t0 = time.time()
    name, dt, env, flat = PLANS[plan]
    case = cases.GROUP_CASES[name]
    groups = case["cfg"]["norm_groups"]
    flat_in = flat and dt == "f32"                            # (bf16: see the module's docstring)
    x, t = case_inputs(name, flat_in)
    sd = flat_state_dict(name, flat_in) if flat else state_dict(name)
    dump = tmp_path / "plan.txt"
    res = check_plan(plan, case, sd, dt, case["B"], case["H"], case["W"], dict(env, DSX_PLAN_DUMP=str(dump)), x, t, dev,
                     monkeypatch, flat=flat)
    ops = read_dump(str(dump))
    # the dump is this plan's: every conv and attention launch of the layer table is one of its lines
    descs = [op["desc"] for op in ops]
    assert all(L["desc"] in descs for L in res["table"] if L["kind"] in (0, 1)), plan
    reach = group_reach_tags(ops, groups)
    # the widest group with |mean| / std > 1e3 among the finalized GroupNorms (flat plans)
    flat_wide = max([(L["C0"] + L["C1"]) // groups for L in res["table"] if (L["gn_ratio"] or 0.0) > 1e3], default=0)
    _CHECKED[plan] = dict(dtype=dt, reach=reach, layers=res["layers"], worst=res["worst"], flat=flat, flat_wide=flat_wide)
    torch.cuda.empty_cache()
    print(f"{plan}: {time.time() - t0:.1f} s; reaches {sorted(reach)}"
          + (f"; widest group with |mean|/std > 1e3: {flat_wide} channels" if flat else ""))


@pytest.mark.parametrize("name", list(cases.GROUP_CASES))
def test_fp32_forward_against_fp64_oracle(name, dev):
    """End to end: the per-layer checks read what each launch read, so a skip connection wired to the wrong layer
    passes them all; the whole forward against the oracle in float64 does not.  The oracle's own fp32-against-fp64
    difference at these models, measured on the CPU: g1 5.8e-6 at max|y| 2.33, g2 2.1e-6 at 3.79, g3 1.7e-6 at 2.73 --
    more than two orders below the tolerance.  (No 16-bit threshold: the wiring is planner code that does not depend
    on the operand type.)"""
    from tests.gpu_util import build_engine
    case = cases.GROUP_CASES[name]
    x, t = case_inputs(name)
    ref = _oracle64(name)
    eng = build_engine(case["cfg"], case["flavour"], state_dict(name), dtype="f32")
    y = eng.forward(x.to(dev), t.to(dev)).cpu()
    assert eng.handoff_timeouts() == 0
    err = maxabs(y, ref)
    print(f"\n{name}: max|hip - oracle64| = {err:.3e}, max|y| = {float(ref.abs().max()):.2f}")
    assert tuple(y.shape) == tuple(ref.shape)
    assert err <= FP32_TOL, err


def _all_checked():
    if set(PLANS) - set(_CHECKED):
        pytest.skip("needs every plan of this module checked in this session; missing: "
                    f"{sorted(set(PLANS) - set(_CHECKED))}")


def test_reach():
    """every reach condition was met by a checked launch in every operand type (runs after the plans; skipped when only
    some of them ran, e.g. with -k)"""
    _all_checked()
    by_dt = {}
    for v in _CHECKED.values():
        by_dt.setdefault(v["dtype"], set()).update(v["reach"])
    print("\n" + "\n".join(f"{d}: {sorted(t)}" for d, t in sorted(by_dt.items())))
    for d in DT:
        missing = set(REACH) - set(REACH_EXEMPT.get(d, {})) - by_dt.get(d, set())
        assert not missing, f"{d}: never reached: {sorted(missing)}"


def test_flat_reach():
    """the flat plans put |mean| / std > 1e3 into a group wider than 64 channels, in f32 and in bf16 (g1: 256 channels,
    g2: 128; g3's widest single-source group has 48)"""
    _all_checked()
    for dt in ("f32", "bf16"):
        wide = {p: v["flat_wide"] for p, v in _CHECKED.items() if v["flat"] and v["dtype"] == dt}
        print(f"\n{dt}: widest group with |mean|/std > 1e3 per flat plan: {wide}")
        assert wide[f"g1_{dt}_flat"] == 256 and wide[f"g2_{dt}_flat"] == 128 and wide[f"g3_{dt}_flat"] == 48, wide
