"""Every conv, attention, GroupNorm-statistics, FiLM and input-staging launch of a UNet forward checked against a
float64 reference of that one layer, computed from the tensors the launch actually read (the executor's layer table:
the workspace is never reused, so after a forward every intermediate is still there).  Bounds and their derivation:
tests/layer_ref.py (the checker itself is tested on the CPU in tests/test_layer_ref_cpu.py); the walk over the layer
table: tests/layer_check.py, shared with tests/test_gpu_widths.py.

One forward per plan.  Plans: the benchmark's (sr3_128, B = 16) in every operand type, the other golden shapes, the
planner's forced paths (environment knobs, read when the executor is created) and the edges no parity test reaches
(ragged 48 x 80 at B = 3: attention over L = 240 keys, a multiple of neither 32 nor 128, with head dimension 64).
A failure names the launch (its dsx_exec_op_info description), the layer's parameter and the worst element."""
import time

import pytest
import torch

from oracle import cases
from tests.layer_check import DT, KNOWN_TAGS, check_plan, inputs
from tests.nets import dev  # noqa: F401  (the fixture)
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_MANY_CHUNKS = {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4",
                "DSX_WS_C4_MIN": "4"}
_NO_SPECIAL = {"DSX_FIRST": "0", "DSX_IMG": "0", "DSX_NARROW_G2": "0"}

# id -> (case, dtype, B, H, W, env)
PLANS = {
    "sr3_128_b16_bf16": ("sr3_128", "bf16", 16, 128, 128, {}),          # exactly bench.py's plan
    "sr3_128_b16_f16": ("sr3_128", "f16", 16, 128, 128, {}),
    "sr3_128_b16_f32": ("sr3_128", "f32", 16, 128, 128, {}),
    "sr3_128_b1_bf16": ("sr3_128", "bf16", 1, 128, 128, {}),
    "sr3_128_b1_f32": ("sr3_128", "f32", 1, 128, 128, {}),
    "hagen_64_bf16": ("hagen_64", "bf16", 2, 64, 64, {}),               # norm_groups == C: one channel per group
    "hagen_64_f32": ("hagen_64", "f32", 2, 64, 64, {}),
    "joint_32_f16": ("joint_32", "f16", 2, 32, 32, {}),
    "ddpm_tiny_bf16": ("ddpm_tiny", "bf16", 3, 32, 48, {}),             # 32 x 48: three tiles per row
    "ddpm_tiny_f32": ("ddpm_tiny", "f32", 3, 32, 48, {}),
    "ragged_48x80_b3_bf16": ("ddpm_tiny", "bf16", 3, 48, 80, {}),       # attention L = 240, head dimension 64
    "ragged_48x80_b3_f32": ("ddpm_tiny", "f32", 3, 48, 80, {}),
    "sr3_128_b1_bf16_many_chunk_ws": ("sr3_128", "bf16", 1, 128, 128, _MANY_CHUNKS),
    "sr3_128_b1_f32_many_chunk_ws": ("sr3_128", "f32", 1, 128, 128, _MANY_CHUNKS),
    "sr3_128_b2_bf16_no_ws": ("sr3_128", "bf16", 2, 128, 128, {"DSX_WS": "0"}),
    "sr3_128_b16_f32_no_ws": ("sr3_128", "f32", 16, 128, 128, {"DSX_WS": "0"}),   # fp32 k_conv_mfma on wide tiles
    "sr3_128_b1_bf16_splitk": ("sr3_128", "bf16", 1, 128, 128, {"DSX_MIN_GRID": "100000", "DSX_WS": "0"}),
    "sr3_128_b1_f32_splitk": ("sr3_128", "f32", 1, 128, 128, {"DSX_MIN_GRID": "100000", "DSX_WS": "0"}),
    "hagen_64_bf16_no_fused_stats": ("hagen_64", "bf16", 2, 64, 64, {"DSX_FUSE_STATS": "0"}),
    "sr3_128_b16_bf16_no_host_fin": ("sr3_128", "bf16", 16, 128, 128, {"DSX_HOST_FIN": "0"}),
    # the first conv with stage mode 2 on k_conv_mfma, 8 x 8 maps on multi-image tiles whose last tile misses an image
    "sr3_128_b3_bf16_plain": ("sr3_128", "bf16", 3, 128, 128, _NO_SPECIAL),
    "sr3_128_b3_f32_plain": ("sr3_128", "f32", 3, 128, 128, _NO_SPECIAL),
    "ddpm_tiny_f32_naive": ("ddpm_tiny", "f32", 3, 32, 48, {"DSX_CONV_IMPL": "naive"}),
    # the same forced paths in the 16-bit types (narrow models with the two-chunk kernel off: the slim 128 x 32 tile)
    "ddpm_tiny_bf16_naive": ("ddpm_tiny", "bf16", 3, 32, 48, {"DSX_CONV_IMPL": "naive"}),
    "ddpm_tiny_f16_naive": ("ddpm_tiny", "f16", 3, 32, 48, {"DSX_CONV_IMPL": "naive"}),
    "ddpm_tiny_bf16_plain": ("ddpm_tiny", "bf16", 3, 32, 48, _NO_SPECIAL),
    "ddpm_tiny_f16_plain": ("ddpm_tiny", "f16", 3, 32, 48, _NO_SPECIAL),
    "sr3_128_b3_f16_plain": ("sr3_128", "f16", 3, 128, 128, _NO_SPECIAL),
    # any grid fills the chip: Cout <= 32 convs take the first slim tile, 128 x 32 (16-bit: only reachable this way)
    "ddpm_tiny_bf16_min_grid1": ("ddpm_tiny", "bf16", 3, 32, 48, dict(_NO_SPECIAL, DSX_MIN_GRID="1", DSX_WS="0")),
    "ddpm_tiny_f16_min_grid1": ("ddpm_tiny", "f16", 3, 32, 48, dict(_NO_SPECIAL, DSX_MIN_GRID="1", DSX_WS="0")),
    "sr3_128_b1_f16_splitk": ("sr3_128", "f16", 1, 128, 128, {"DSX_MIN_GRID": "100000", "DSX_WS": "0"}),
    "sr3_128_b1_f16_many_chunk_ws": ("sr3_128", "f16", 1, 128, 128, _MANY_CHUNKS),
    # the planner's knob -> col_split = 0 -> k_attn<*, 4, 1> at head dimension 512 (the default runs <*, 4, 2>)
    "sr3_128_b1_bf16_attn_cs1": ("sr3_128", "bf16", 1, 128, 128, {"DSX_ATTN_CS": "1"}),
}

# Every known tag must have been checked in every operand type, except where the planner cannot emit it:
EXEMPT = {
    # no default tile preference list of PlanKnobs names it: only a DSX_TILES_* override reaches it
    "tile256x128": "not in any default tile list",
}
REQUIRED_TAGS = {dt: KNOWN_TAGS - set(EXEMPT) for dt in DT}

_CHECKED = {}          # plan -> {dtype, tags, layers, worst}


def _check_plan(plan, dev, monkeypatch, flat=False):
    case_name, dt, B, H, W, env = PLANS[plan] if not flat else FLAT_PLAN
    case = cases.UNET_CASES[case_name]
    sd, _ = golden_state_dict("unet_" + case_name)
    if flat:
        sd = dict(sd)
        sd["downs.0.bias"] = torch.full_like(sd["downs.0.bias"], 10.0)   # the background level of a flat tile
    ddpm_t = torch.tensor([0.37]) if case_name == "ddpm_tiny" else torch.tensor([3.0, 1700.0][:B])
    x, t = inputs(case, B, H, W, flat, ddpm_t)
    res = check_plan(plan, case, sd, dt, B, H, W, env, x, t, dev, monkeypatch, flat)
    _CHECKED[plan] = dict(dtype=dt, tags=res["tags"], layers=res["layers"], worst=res["worst"])


@pytest.mark.parametrize("plan", list(PLANS))
def test_every_layer_against_fp64(plan, dev, monkeypatch):
    t0 = time.time()
    _check_plan(plan, dev, monkeypatch)
    torch.cuda.empty_cache()
    print(f"{plan}: {time.time() - t0:.1f} s")


# A flat background in the fp32 build: every layer, with the GroupNorm groups after the first conv (one channel per
# group) at |mean| / sqrt(var + eps) ~ 3 10^3 on the fused-statistics path.  The level is put into the first conv's bias
# (10) and the image is zero plus 1e-4 noise, rather than a constant image: with a constant c != 0 the zero padding makes
# the border pixels differ from the interior by c times the outside taps' weights, and those borders alone hold
# |mean| / std near 10.  (eps = 1e-5 caps the ratio at 316 per unit of mean, hence a level of 10.)  The raw fp32 sums
# of x and x^2 cancel here (gn_scale 13 times its bound); the first conv sums x - bias instead (StatPivot).
FLAT_PLAN = ("hagen_64", "f32", 2, 64, 64, {})


def test_flat_input_groupnorm_statistics(dev, monkeypatch):
    _check_plan("flat", dev, monkeypatch, flat=True)


def test_variant_coverage():
    """every required variant tag was checked in every operand type the planner emits it in (runs after the plans;
    skipped when only some of them ran, e.g. with -k)"""
    if set(PLANS) - set(_CHECKED):
        pytest.skip(f"needs every plan of this module checked in this session; missing: {sorted(set(PLANS) - set(_CHECKED))}")
    by_dt = {}
    for v in _CHECKED.values():
        by_dt.setdefault(v["dtype"], set()).update(v["tags"])
    print("\n" + "\n".join(f"{d}: {sorted(t)}" for d, t in sorted(by_dt.items())))
    for d, req in REQUIRED_TAGS.items():
        missing = req - by_dt.get(d, set())
        assert not missing, f"{d}: variants never checked: {missing}"
