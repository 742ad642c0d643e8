"""Host-only checks of the launch planner (dsx_plan_dry_run: no GPU, no compute).

Round 1 shipped a workspace overflow: the planner's sizing pass and its planning pass diverged for some tile
preferences (a tiling decision keyed on a pointer that is null while sizing) and a conv wrote past the workspace
(`Memory access fault`, DSX_MIN_GRID=448).  dsx_exec_create now fails unless both passes walk exactly the same
number of bytes; these tests pin that for every tile-preference environment setting used while tuning, for all
BASELINE configs and operand types.  The knobs are read from the environment at plan time; every setting runs in a
child process with its own environment."""
import json
import os
import subprocess
import sys

import pytest

from tests.plan_cases import CONFIGS, ENV_SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from diffsplitting_amd import _lib     # ctypes only (no torch import: the child starts in ~0.1 s)
configs = json.loads(sys.argv[1])
out = {}
for name, (flavour, kw, B, H, W, cc) in configs.items():
    cfg = _lib.UnetCfg()
    cfg.flavour = 0 if flavour == "sr3" else 1
    for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "res_blocks", "image_size"):
        setattr(cfg, k, kw[k])
    cfg.n_mults = len(kw["channel_mults"]); cfg.n_attn_res = len(kw["attn_res"]); cfg.with_time_emb = 1
    for i, m in enumerate(kw["channel_mults"]): cfg.channel_mults[i] = m
    for i, m in enumerate(kw["attn_res"]): cfg.attn_res[i] = m
    for dt, code in (("f32", 0), ("bf16", 1), ("f16", 2)):
        a, b, n = C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.lib.dsx_plan_dry_run(C.byref(cfg), code, B, H, W, cc, C.byref(a), C.byref(b), C.byref(n)))
        out[name + "/" + dt] = (a.value, b.value, n.value)
print(json.dumps(out))
"""


@pytest.mark.parametrize("env", ENV_SETS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_sizing_and_planning_passes_agree(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, json.dumps(CONFIGS)], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 3 * len(CONFIGS)
    for name, (sizing, planning, launches) in res.items():
        assert sizing == planning and sizing > 0, (name, env, sizing, planning)
        assert launches > 10


def test_plan_rejects_sources_of_2gib():
    """The conv kernels address a source with 32-bit byte offsets (0x80000000 = forced out of bounds): a tensor of
    2 GiB or more must be refused by the planner, not silently read as zeros (sr_sr3_64_512 fp32 at B >= 16)."""
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    flavour, kw, _, H, W, cc = CONFIGS["c4_sr3_512_b2"]
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    a, b, _ = engine.plan_dry_run(cfg, "f32", 8, H, W, cc)          # 8 x 512 x 512 x 128 x 4 B = 1 GiB: fine
    assert a == b
    with pytest.raises(DsxError, match="2 GiB"):
        engine.plan_dry_run(cfg, "f32", 16, H, W, cc)               # 16 x 512 x 512 x 128 x 4 B = 2 GiB
    a, b, _ = engine.plan_dry_run(cfg, "bf16", 16, H, W, cc)        # bf16 storage halves it
    assert a == b
    with pytest.raises(DsxError, match="2 GiB"):
        engine.plan_dry_run(cfg, "bf16", 32, H, W, cc)


def test_headline_config_launch_count():
    """C2 (sr_sr3_16_128, B=16): one UNet forward is 134 launches (94 conv + 32 finalize + 6 attention + 2 split-K
    reduce; 194 in round 1): 14 GroupNorm finalizes run inside the residual 1 x 1 conv in front of them.  A planner
    change that adds launches shows up here, without a GPU."""
    from diffsplitting_amd import engine
    flavour, kw, B, H, W, cc = CONFIGS["c2_sr3_128_b16"]
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    for dt in ("f32", "bf16", "f16"):
        a, b, n = engine.plan_dry_run(cfg, dt, B, H, W, cc)
        assert a == b
        assert n <= 134, (dt, n)


_RANDOM_CHILD = r"""
import ctypes as C, json, random, sys
sys.path.insert(0, %r)
from diffsplitting_amd import _lib
rng = random.Random(int(sys.argv[1]))
bad = []
n_ok = n_refused = 0
for case in range(int(sys.argv[2])):
    levels = rng.choice([2, 3, 4])
    mults = [1] + sorted(rng.choice([1, 2, 4, 8]) for _ in range(levels - 1))
    inner = rng.choice([16, 32, 64])
    groups = rng.choice([8, 16])
    flavour = rng.choice([0, 1])
    cond = rng.choice([0, 1, 3]) if flavour == 0 else 0
    cin = rng.choice([1, 2, 3]) + cond
    unit = 1 << (levels - 1)
    # bottom-level maps of 2, 4, 6, ... 40 pixels per side.  An MFMA tile is TW x TH pixels x TB images with TW, TH the
    # largest powers of two (<= 16, <= BM / TW) dividing the map's sides, 2 x 32 or 4 x 4 x 4 as well as 8 x 8; a map is
    # refused only when the halo patches of the images it takes to fill a tile pass the staging registers (10 x 10 maps:
    # sixteen 4 x 4 patches), see test_admission_map
    H, W = unit * 2 * rng.randint(1, 20), unit * 2 * rng.randint(1, 20)
    B = rng.choice([1, 2, 3, 5, 8, 16])
    attn = [rng.choice([H, H // 2 or 1, 16])] if rng.random() < 0.4 else []
    cfg = _lib.UnetCfg()
    cfg.flavour = flavour; cfg.in_channel = cin; cfg.out_channel = rng.choice([1, 2, 3]); cfg.inner_channel = inner
    cfg.norm_groups = groups; cfg.res_blocks = rng.choice([1, 2]); cfg.image_size = H; cfg.with_time_emb = 1
    cfg.n_mults = len(mults); cfg.n_attn_res = len(attn)
    for i, m in enumerate(mults): cfg.channel_mults[i] = m
    for i, m in enumerate(attn): cfg.attn_res[i] = m
    for code in (0, 1, 2):
        a, b, n = C.c_size_t(), C.c_size_t(), C.c_int()
        rc = _lib.lib.dsx_plan_dry_run(C.byref(cfg), code, B, H, W, cond, C.byref(a), C.byref(b), C.byref(n))
        if rc != 0:
            msg = _lib.lib.dsx_last_error().decode()
            # a map no MFMA tile covers is refused by that message (and by no other); nothing is mis-sized
            if "fastdiv" in msg or "planner" in msg or "no MFMA tile fits" not in msg: bad.append((case, code, B, H, W, msg))
            n_refused += 1
            continue
        n_ok += 1
        if a.value != b.value or a.value == 0: bad.append((case, code, B, H, W, a.value, b.value))
print(json.dumps({"ok": n_ok, "refused": n_refused, "bad": bad}))
"""


_RANDOM_CASES = "150"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_shapes_size_and_plan_alike(seed):
    """Random UNet topologies, batch sizes and (ragged) image sizes, all three operand types, default knobs and the
    persistent kernel forced onto every grid: the sizing pass and the planning pass of dsx_exec_create's planner walk
    the same bytes, and the plan-time check of the start-up division magics never trips.  The sides are any even
    multiple of the model's unit, so most draws are maps no MFMA tile covers: those must be refused by that message, and
    enough cases are drawn that as many plan as when every side was a multiple of 8 units."""
    for env in ({}, {"DSX_WS_MIN_GRID": "1"}):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _RANDOM_CHILD % ROOT, str(seed), _RANDOM_CASES], env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert not res["bad"], res["bad"][:5]
        assert res["ok"] + res["refused"] == 3 * int(_RANDOM_CASES)
        assert res["ok"] >= 90, res


_WIDTHS_CHILD = r"""
import ctypes as C, json, random, sys
sys.path.insert(0, %r)
from diffsplitting_amd import _lib
rng = random.Random(int(sys.argv[1]))
bad, refusals = [], []
n_ok = 0
for case in range(int(sys.argv[2])):
    levels = rng.choice([2, 3, 4])
    mults = [1] + sorted(rng.choice([1, 2, 3, 4, 5, 6, 8]) for _ in range(levels - 1))
    inner = 4 * rng.randint(2, 32)
    groups = rng.choice([g for g in range(1, inner + 1) if inner %% g == 0])
    flavour = rng.choice([0, 1])
    cond = rng.choice([0, 1, 3]) if flavour == 0 else 0
    cin = rng.choice([1, 2, 3]) + cond
    unit = 1 << (levels - 1)
    H, W = unit * 8 * rng.randint(1, 3), unit * 8 * rng.randint(1, 3)   # bottom maps of 8 / 16 / 24 per side
    B = rng.choice([1, 2, 3, 5, 8])
    attn = [rng.choice([H, H // 2 or 1, 16])] if rng.random() < 0.4 else []
    cfg = _lib.UnetCfg()
    cfg.flavour = flavour; cfg.in_channel = cin; cfg.out_channel = rng.choice([1, 2, 3]); cfg.inner_channel = inner
    cfg.norm_groups = groups; cfg.res_blocks = rng.choice([1, 2]); cfg.image_size = H; cfg.with_time_emb = 1
    cfg.n_mults = len(mults); cfg.n_attn_res = len(attn)
    for i, m in enumerate(mults): cfg.channel_mults[i] = m
    for i, m in enumerate(attn): cfg.attn_res[i] = m
    for code in (0, 1, 2):
        a, b, n = C.c_size_t(), C.c_size_t(), C.c_int()
        rc = _lib.lib.dsx_plan_dry_run(C.byref(cfg), code, B, H, W, cond, C.byref(a), C.byref(b), C.byref(n))
        if rc != 0:
            refusals.append((case, code, inner, mults, B, H, W, _lib.lib.dsx_last_error().decode()))
            continue
        n_ok += 1
        if a.value != b.value or a.value == 0: bad.append((case, code, inner, mults, B, H, W, a.value, b.value))
print(json.dumps({"ok": n_ok, "bad": bad, "refusals": refusals}))
"""


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_widths_size_and_plan_alike(seed):
    """test_random_shapes_size_and_plan_alike over channel widths: inner_channel any multiple of 4 from 8 to 128,
    norm_groups any divisor of it, channel_mults that are no powers of two (3, 5, 6).  Every channel count is then
    some 4 m: K tails, N tails, sources that are no whole 16-byte units.  Sizing and planning walk the same bytes
    wherever the planner accepts the shape; a refusal is one of the two the planner is meant to give (a head dimension
    k_attn has no instantiation for, a map no MFMA tile covers), by its message."""
    for env in ({}, {"DSX_WS_MIN_GRID": "1"}):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _WIDTHS_CHILD % ROOT, str(seed), "60"], env=e, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert not res["bad"], res["bad"][:5]
        for ref in res["refusals"]:
            msg = ref[-1]
            assert "fastdiv" not in msg and "planner" not in msg, ref
            assert ("attention with head dimension" in msg and "is not supported" in msg) or "no MFMA tile fits" in msg, ref
        assert res["ok"] + len(res["refusals"]) == 180
        assert res["ok"] >= 120, (res["ok"], [r[-1] for r in res["refusals"]][:10])


def test_refusals_by_message():
    """The two refusals of the planner that a config at an unusual width or size can meet, by their text."""
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    # 12 x 3 = 36 channels at the bottom: k_attn stages the head dimension in 16-byte units of bf16 (multiples of 8)
    cfg = engine.make_cfg("ddpm", 2, 2, 12, 4, (1, 3), (), 1, 32)
    for dt in ("f32", "bf16", "f16"):
        with pytest.raises(DsxError, match=r"attention with head dimension 36 is not supported"):
            engine.plan_dry_run(cfg, dt, 2, 32, 32, 0)
    # ddpm_tiny (mults 1, 2, 4) at 20 x 36: the second level's maps are 10 x 18, whose tile is 2 x 2 pixels x 16 images --
    # sixteen 4 x 4 halo patches, more than the staging registers hold (test_admission_map has the rule)
    _, kw, *_ = CONFIGS["ragged_48x80_b3"]
    cfg = engine.make_cfg("ddpm", kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    for dt in ("f32", "bf16", "f16"):
        with pytest.raises(DsxError, match=r"no MFMA tile fits conv 3x3 \(10x18 out"):
            engine.plan_dry_run(cfg, dt, 5, 20, 36, 0)


@pytest.mark.parametrize("name,dt", [("c2_sr3_128_b16", "f32"), ("c2_sr3_128_b16", "bf16"), ("c3_hagen_512_b8", "bf16"),
                                     ("ragged_48x80_b3", "bf16")])
def test_plan_ops_match_recorded_plan(name, dt, tmp_path, monkeypatch):
    """The launches of the plan at default knobs, as DSX_PLAN_DUMP writes them: their (kind, description) sequence --
    kernel family, tile and chunk variant of every layer, and the launch order -- equals tests/golden/plan_ops.json,
    recorded from the planner before it was rewritten as decide / reserve / emit.  A planner change that means to
    alter a plan regenerates the fixture from the dump."""
    import re
    from diffsplitting_amd import engine
    flavour, kw, B, H, W, cc = CONFIGS[name]
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    path = tmp_path / "plan.txt"
    monkeypatch.setenv("DSX_PLAN_DUMP", str(path))
    a, b, n = engine.plan_dry_run(cfg, dt, B, H, W, cc)
    assert a == b
    ops = []
    for i, line in enumerate(path.read_text().splitlines()):
        m = re.match(r'(\d+) kind=(\d+) desc="([^"]*)" flops=\S+ bytes=\S+ launcher=\w+ dtype=\d+ tile=-?\d+ ks=\d+ '
                     r'stride=\d+ col_split=\d+ args=([0-9a-f]+)$', line)
        assert m and int(m.group(1)) == i, line[:200]
        ops.append([int(m.group(2)), m.group(3)])
    with open(os.path.join(ROOT, "tests", "golden", "plan_ops.json")) as f:
        want = json.load(f)[f"{name}/{dt}"]
    assert len(ops) == n == len(want)          # every launch of the plan is one line of the dump
    assert ops == want


# ---- the geometry classes of tests/test_gpu_shapes.py, from the planner's dry run of that module's own plans

_SHAPES_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %r)
from diffsplitting_amd import _lib
out = {}
for plan, (flavour, kw, code, B, H, W) in json.loads(sys.argv[1]).items():
    cfg = _lib.UnetCfg()
    cfg.flavour = 0 if flavour == "sr3" else 1
    for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "res_blocks", "image_size"):
        setattr(cfg, k, kw[k])
    cfg.n_mults = len(kw["channel_mults"]); cfg.n_attn_res = len(kw["attn_res"]); cfg.with_time_emb = 1
    for i, m in enumerate(kw["channel_mults"]): cfg.channel_mults[i] = m
    for i, m in enumerate(kw["attn_res"]): cfg.attn_res[i] = m
    os.environ["DSX_PLAN_DUMP"] = os.path.join(sys.argv[2], plan + ".txt")    # (read at plan time)
    a, b, n = C.c_size_t(), C.c_size_t(), C.c_int()
    _lib.check(_lib.lib.dsx_plan_dry_run(C.byref(cfg), code, B, H, W, 0, C.byref(a), C.byref(b), C.byref(n)))
    out[plan] = (a.value, b.value, n.value)
print(json.dumps(out))
"""


def dumped_geom_tag(op):
    """the geometry class of one DSX_PLAN_DUMP launch (tests/plan_dump.py read_dump), from the tile the planner wrote
    into its arguments; None for a launch outside the MFMA families"""
    if op["launcher"] not in ("conv_mfma", "conv_ws"):
        return None
    a = op["conv"]
    fam = "ws" if op["launcher"] == "conv_ws" else ("splitK" if " splitK" in op["desc"] else ("g2" if a.cpg == 2 else "mfma"))
    size = f"{op['ks']}x{op['ks']}" + (" s2" if op["stride"] == 2 else "") + (" up" if a.up else "")
    TW, TH, TB = 1 << a.tw_log2, 1 << a.th_log2, 1 << a.tb_log2
    return f"{fam} {size} {TW}x{TH}x{TB}@{TW * TH * TB}" + ("+tail" if a.B % TB else "")


def shape_plan_tags(tmp_path):
    """plan -> [(tag from the dumped tile, tag geom_tag derives from the shape fields)] per MFMA-family launch of every
    plan of tests/test_gpu_shapes.py: one child process per knob setting, a dry run and a dump per plan"""
    from oracle import cases
    from tests.layer_check import geom_tag
    from tests.plan_dump import read_dump
    from tests.plan_cases import SHAPE_PLANS as PLANS
    code = {"f32": 0, "bf16": 1, "f16": 2}
    by_env = {}
    for plan, (name, dt, B, env) in PLANS.items():
        c = cases.SHAPE_CASES[name]
        by_env.setdefault(json.dumps(env, sort_keys=True), {})[plan] = (c["flavour"], c["cfg"], code[dt], B, c["H"], c["W"])
    out = {}
    for env, plans in by_env.items():
        e = dict(os.environ)
        e.update(json.loads(env))
        r = subprocess.run([sys.executable, "-c", _SHAPES_CHILD % ROOT, json.dumps(plans), str(tmp_path)], env=e,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for plan in plans:
            sizing, planning, launches = res[plan]
            assert sizing == planning and sizing > 0, (plan, sizing, planning)
            ops = read_dump(tmp_path / (plan + ".txt"))
            assert len(ops) == launches
            pairs = []
            for o in ops:
                if o["launcher"] in ("conv_mfma", "conv_ws"):
                    a = o["conv"]
                    L = dict(kind=0, desc=o["desc"], ks=o["ks"], stride=o["stride"], up=a.up, Ho=a.Ho, Wo=a.Wo, B=a.B)
                    pairs.append((dumped_geom_tag(o), geom_tag(L), o["desc"]))
            out[plan] = pairs
    return out


def test_shape_plans_reach_their_geometry_classes(tmp_path):
    """tests/test_gpu_shapes.py without a GPU: geom_tag (the tile derived from Ho, Wo and the description, which is all
    the layer table gives) names the tile the planner wrote into every launch's arguments; the classes each operand
    type's plans reach are the recorded ones (tests/golden/shape_reach.json, which test_reach of the GPU module asks
    for); their union holds the module's REACH and REACH_TAILS."""
    from tests.plan_cases import SHAPE_PLANS as PLANS, SHAPE_REACH as REACH, SHAPE_REACH_TAILS as REACH_TAILS
    from tests.plan_cases import shape_reach_by_dtype as reach_by_dtype
    tags = shape_plan_tags(tmp_path)
    by_dt = {}
    for plan, pairs in tags.items():
        assert pairs, plan
        for dumped, derived, desc in pairs:
            assert dumped == derived, (plan, desc, dumped, derived)
        by_dt.setdefault(PLANS[plan][1], set()).update(t for t, _, _ in pairs)
    want = reach_by_dtype()
    assert set(want) == set(by_dt) == {"bf16", "f16", "f32"}
    for d in want:
        assert by_dt[d] == want[d], (d, sorted(by_dt[d] - want[d]), sorted(want[d] - by_dt[d]))
    union = set().union(*by_dt.values())
    assert not REACH - {t.replace("+tail", "") for t in union}, sorted(REACH - {t.replace("+tail", "") for t in union})
    assert not REACH_TAILS - union, sorted(REACH_TAILS - union)


# ---- which sizes plan at all

ADMISSION_MODELS = {
    "ddpm_tiny": CONFIGS["ragged_48x80_b3"],       # three levels
    "hagen_64": CONFIGS["c3_hagen_512_b8"],        # four levels
}
# patch pixels the staging registers of k_conv_mfma hold (mfma_max_px in dsx_conv_variants.h), per tile pixel count
_PATCH_CAP_S1 = {64: 144, 128: 220, 256: 400}
_PATCH_CAP_S2 = {64: 400}


def _map_fits(Ho, Wo, stride):
    """some tile of a 3 x 3 conv with this output map fits: TW = the largest power of two <= 16 dividing Wo, TH = the
    largest <= BM / TW dividing Ho, TB = BM / (TW TH) images (so TW TH TB == BM by construction), and the halo patch
    ((TH - 1) s + 3) ((TW - 1) s + 3) TB within the cap of that BM and stride"""
    from tests.layer_check import pow2_divisor
    for BM, cap in (_PATCH_CAP_S1 if stride == 1 else _PATCH_CAP_S2).items():
        TW = pow2_divisor(Wo, 16)
        TH = pow2_divisor(Ho, max(1, BM // TW))
        TB = BM // (TW * TH)
        assert TW * TH * TB == BM
        if ((TH - 1) * stride + 3) * ((TW - 1) * stride + 3) * TB <= cap:
            return True
    return False


def admitted(levels, H, W):
    """the stated rule: every level's map takes a stride-1 3 x 3 conv, every level below the first is also the output
    of a stride-2 one.  (The 1 x 1 convs have no halo and fit wherever the 3 x 3 of their level does; k_conv_first and
    k_conv_img only take maps that an MFMA tile covers too: Wo % 16 == 0, 8 x 8.)"""
    return all(_map_fits(H >> l, W >> l, 1) and (l == 0 or _map_fits(H >> l, W >> l, 2)) for l in range(levels))


@pytest.mark.parametrize("model", list(ADMISSION_MODELS))
def test_admission_map(model):
    """Which sizes plan: every H and W in 4, 8, ..., 128 at B = 3 in every operand type either plans (sizing and
    planning walk the same bytes) or is refused with "no MFMA tile fits", and which of the two equals `admitted`, the
    rule written out above.  Far fewer sizes plan than are divisible by 2^(levels - 1): 96 of the 1024 at three levels
    -- 40 x 40, 24 x 24 and 32 x 24 do not.  This pins the admitted set as it is; it is not a promise to keep refusing."""
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    flavour, kw, _, _, _, cc = ADMISSION_MODELS[model]
    levels = len(kw["channel_mults"])
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    sides = range(4, 129, 4)
    planned, wrong = {}, []
    for dt in ("f32", "bf16", "f16"):
        planned[dt] = set()
        for H in sides:
            for W in sides:
                try:
                    a, b, n = engine.plan_dry_run(cfg, dt, 3, H, W, cc)
                    assert a == b and a > 0 and n > 10, (dt, H, W, a, b, n)
                    planned[dt].add((H, W))
                except DsxError as e:
                    assert "no MFMA tile fits" in str(e), (dt, H, W, str(e))
                if ((H, W) in planned[dt]) != admitted(levels, H, W):
                    wrong.append((dt, H, W, (H, W) in planned[dt]))
    assert not wrong, (len(wrong), wrong[:10])
    assert planned["f32"] == planned["bf16"] == planned["f16"]
    if levels == 3:
        assert len(planned["f32"]) == 96
        assert not {(40, 40), (24, 24), (32, 24)} & planned["f32"]
        assert {(64, 48), (64, 24), (128, 24), (48, 32), (24, 64), (32, 48), (48, 80)} <= planned["f32"]
