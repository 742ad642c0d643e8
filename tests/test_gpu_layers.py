"""Every conv, attention, GroupNorm-statistics, FiLM and input-staging launch of a UNet forward checked against a
float64 reference of that one layer, computed from the tensors the launch actually read (the executor's layer table:
the workspace is never reused, so after a forward every intermediate is still there).  Bounds and their derivation:
tests/layer_ref.py; the checker itself is tested on the CPU in tests/test_layer_ref_cpu.py.

One forward per plan.  Plans: the benchmark's (sr3_128, B = 16) in every operand type, the other golden shapes, the
planner's forced paths (environment knobs, read when the executor is created) and the edges no parity test reaches
(ragged 48 x 80 at B = 3: attention over L = 240 keys, a multiple of neither 32 nor 128, with head dimension 64).
A failure names the launch (its dsx_exec_op_info description), the layer's parameter and the worst element."""
import math
import time

import pytest
import torch

from oracle import cases
from tests import layer_ref
from tests.gpu_util import build_engine
from tests.util import golden_state_dict

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
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

# every variant tag a checked launch may carry; a new kernel variant must be added here (and so get checked)
# (the tiles are ConvTile of dsx_kernels.h)
KNOWN_TAGS = {"first", "img", "g2", "ws", "ws c2", "ws c4", "+gn", "splitK", "s2", "up", "naive", "attn", "stage1",
              "stage2",
              "tile256x128", "tile128x128", "tile64x128", "tile256x64", "tile128x64", "tile64x64", "tile128x32",
              "tile256x32"}
# (stage1 / stage2: staging modes of k_conv_mfma / k_conv_ws, derived from the layer's shapes, see stage_tag.)
# Every known tag must have been checked in every operand type, except where the planner cannot emit it:
EXEMPT = {
    # no default tile preference list of PlanKnobs names it: only a DSX_TILES_* override reaches it
    "tile256x128": "not in any default tile list",
}
REQUIRED_TAGS = {dt: KNOWN_TAGS - set(EXEMPT) for dt in DT}

_CHECKED = {}          # plan -> {dtype, tags, layers, worst}


def stage_tag(L, dt):
    """k_conv_mfma / k_conv_ws staging mode of a conv (plan_conv): 1 = a concat whose first source ends inside a staged
    group, 2 = a source that is not a whole number of 16-byte units"""
    if {"first", "img", "naive"} & launch_tags(L["desc"]):
        return set()
    um, kc = (3, 16) if dt == "f32" else (7, 32)
    gw = (2 if L["ks"] == 1 else 1) * kc
    C0, C1 = L["C0"], L["C1"]
    mode = 2 if (C0 & um or C1 & um) else (0 if (C1 == 0 or C0 % gw == 0) else 1)
    return {f"stage{mode}"} if mode else set()


def launch_tags(desc):
    tok = desc.split()
    if not tok:
        return set()
    tags = set()
    head = tok[0]
    if head == "attn":
        return {"attn"}
    if head.endswith("-naive"):
        tags.add("naive")
    if head.endswith("s2"):
        tags.add("s2")
    if head.endswith("up"):
        tags.add("up")
    for i, t in enumerate(tok[1:], 1):
        if t in ("first", "img", "g2", "+gn"):
            tags.add(t)
        elif t == "ws":
            tags.add("ws")
            if i + 1 < len(tok) and tok[i + 1] in ("c2", "c4"):
                tags.add("ws " + tok[i + 1])
        elif t.startswith("splitK"):
            tags.add("splitK")
        elif t.startswith("tile"):
            tags.add(t)
    return tags


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _inputs(case_name, B, H, W, flat):
    case = cases.UNET_CASES[case_name]
    g = torch.Generator().manual_seed(1000 + B * 7 + H + W)
    cin = case["cfg"]["in_channel"]
    x = (1e-4 if flat else 1.0) * torch.randn((B, cin, H, W), generator=g)
    if case["flavour"] == "sr3":
        t = 0.05 + 0.95 * torch.rand((B, 1), generator=g)
    else:
        t = torch.tensor([0.37]) if case_name == "ddpm_tiny" else torch.tensor([3.0, 1700.0][:B])
    return x, t


def _film_reference(sd, case, t, B):
    """fp64 time MLP (sr3 PositionalEncoding / ddpm TimeEmbedding) and the stacked per-block linears, with an
    absolute error bound propagated through every fp32 step the kernel takes (each <= u32 relative, accumulations at
    4 sqrt(K) u32, sin/cos arguments rounded to fp32: <= 2 u32 (1 + |arg|))"""
    U = layer_ref.U32
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    inner = case["cfg"]["inner_channel"]
    tt = t.reshape(-1).to(torch.float64)
    if tt.numel() == 1:
        tt = tt.expand(B)
    if case["flavour"] == "sr3":
        freq = torch.exp(-math.log(1e4) * torch.arange(inner // 2, dtype=torch.float64) / (inner // 2))
        p1, p3 = "noise_level_mlp.1", "noise_level_mlp.3"
    else:
        freq = sd["time_mlp.0.inv_freq"]
        p1, p3 = "time_mlp.1", "time_mlp.3"
    arg = tt[:, None] * freq[None, :]
    enc = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)
    e = 2 * U * (1 + torch.cat([arg, arg], dim=-1).abs())

    def lin(h, eh, w, b):
        K = w.shape[1]
        y = h @ w.T + b
        S = h.abs() @ w.abs().T + b.abs()
        return y, eh @ w.abs().T + 4 * math.sqrt(K + 1) * U * S

    def sw(h, eh):
        a = layer_ref.swish(h)
        return a, 1.1 * eh + 4 * U * a.abs()
    h, eh = sw(*lin(enc, e, sd[p1 + ".weight"], sd[p1 + ".bias"]))
    h, eh = lin(h, eh, sd[p3 + ".weight"], sd[p3 + ".bias"])
    if case["flavour"] != "sr3":
        h, eh = sw(h, eh)
    return h, eh, sd


def _check_plan(plan, dev, monkeypatch, flat=False):
    case_name, dt, B, H, W, env = PLANS[plan] if not flat else FLAT_PLAN
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = cases.UNET_CASES[case_name]
    sd, _ = golden_state_dict("unet_" + case_name)
    if flat:
        sd = dict(sd)
        sd["downs.0.bias"] = torch.full_like(sd["downs.0.bias"], 10.0)   # the background level of a flat tile
    groups = case["cfg"]["norm_groups"]
    op = DT[dt]
    eng = build_engine(case["cfg"], case["flavour"], sd, dtype=dt)
    x, t = _inputs(case_name, B, H, W, flat)
    eng.forward(x.to(dev), t.to(dev))
    table = eng.layer_table(B, H, W)
    assert eng.handoff_timeouts() == 0
    images = [0, B - 1] if B >= 4 else None
    fails, tags, worst, n = [], set(), (0.0, ""), 0
    max_gn_ratio = 0.0
    film_h, film_e, sd64 = _film_reference(sd, case, t, B)
    film_h, film_e = film_h.to(dev), film_e.to(dev)

    def note(v, what):
        nonlocal worst
        if v.ratio > worst[0]:
            worst = (v.ratio, what)
        if not v.ok:
            fails.append(v.message())

    for L in table:
        kind = L["kind"]
        if kind == 3:                                  # staged input: bit-equal to round_T(x) in NHWC
            ref = x[:, L["C0"]:L["C0"] + L["Cout"]].permute(0, 2, 3, 1).to(dev).to(L["out"].dtype)
            if not torch.equal(L["out"], ref):
                fails.append(f"input staging (channels {L['C0']}..): not bit-equal to round_T(x)")
            n += 1
            continue
        if kind == 2:                                  # FiLM vector: checked below, per block
            continue
        n += 1
        tags |= launch_tags(L["desc"])
        where = f"[{plan}] {L['desc']} ({L['w_name'] or 'attention'})"
        if kind == 1:
            note(layer_ref.check_attention(L, op, images, where), where)
            continue
        tags |= stage_tag(L, dt)
        w = sd[L["w_name"]].to(dev)
        bias = None if (L["bias_in_film"] or L["b_name"] is None) else sd[L["b_name"]].to(dev)
        gamma = sd[L["gn_gamma_name"]].to(dev) if L["gn_gamma_name"] else None
        beta = sd[L["gn_beta_name"]].to(dev) if L["gn_beta_name"] else None
        # k_conv_naive multiplies fp32 weights by the fp32 activation in every build: its operands are not rounded
        op_conv = torch.float32 if "naive" in launch_tags(L["desc"]) else op
        note(layer_ref.check_conv(L, w, bias, gamma, beta, groups, op_conv, images, where), where)
        if L["gn_scale"] is not None:
            v1, v2, r = layer_ref.check_gn_stats(L, gamma, beta, groups, op, where)
            max_gn_ratio = max(max_gn_ratio, r)
            note(v1, where + " gn_scale")
            note(v2, where + " gn_shift")
        if L["film"] is not None:
            rb = L["w_name"][:-len(".block1.block.3.weight")]
            lk = rb + (".noise_func.noise_func.0" if case["flavour"] == "sr3" else ".mlp.1")
            wf, bf = sd64[lk + ".weight"].to(dev), sd64[lk + ".bias"].to(dev)
            ref = film_h @ wf.T + bf
            S = film_h.abs() @ wf.abs().T + bf.abs()
            if L["bias_in_film"]:
                cb = sd64[L["b_name"]].to(dev)
                ref, S = ref + cb, S + cb.abs()
            bound = film_e @ wf.abs().T + 4 * math.sqrt(wf.shape[1] + 2) * layer_ref.U32 * S
            fv = layer_ref.Verdict(L["film"].to(torch.float64), ref, bound, torch.zeros_like(ref), where + " film")
            fv.aggregate = []
            note(fv, where + " film")
    assert eng.handoff_timeouts() == 0
    print(f"\n{plan}: {n} layers checked, worst error/bound {worst[0]:.3f} at {worst[1]}; "
          f"max |mean|/std of a GroupNorm group {max_gn_ratio:.3g}")
    if flat:
        assert max_gn_ratio > 1e3, f"the flat case should reach |mean|/std > 1e3, got {max_gn_ratio:.3g}"
    assert not fails, f"{len(fails)} check(s) failed:\n" + "\n".join(fails[:20])
    unknown = tags - KNOWN_TAGS
    assert not unknown, f"launch variants without per-layer coverage: {unknown}"
    _CHECKED[plan] = dict(dtype=dt, tags=tags, layers=n, worst=worst)


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
