"""What tests/test_gpu_groups.py reaches, without a GPU: the planner's dry run of that module's own plans (GROUP_CASES
of oracle/cases.py in every operand type, under the module's knob sets), read from DSX_PLAN_DUMP.  Which kernel runs
gn_finalize_item for each GroupNorm -- k_gn_finalize, k_gn_finalize_wide or a residual 1 x 1 k_conv_ws launch -- at how
many channels per group, from which partials, and that k_conv_img takes no GroupNorm it cannot finalize."""
import pytest

from oracle import cases
from tests.layer_check import finalizes, group_reach_tags
from tests.plan_cases import GROUP_PLANS as PLANS, GROUP_REACH as REACH, GROUP_REACH_EXEMPT as REACH_EXEMPT
from tests.plan_dump import read_dump

KNOBS = ("DSX_WS_MIN_GRID", "DSX_MIN_GRID", "DSX_WS", "DSX_HOST_FIN")      # every knob a plan of the module sets
DRY = sorted({(name, dt, tuple(sorted(env.items()))) for name, dt, env, _ in PLANS.values()})   # (flat plans: same plan)


def _dump(name, dt, env, tmp_path, monkeypatch):
    from diffsplitting_amd import engine
    case = cases.GROUP_CASES[name]
    kw = case["cfg"]
    cfg = engine.make_cfg(case["flavour"], kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    path = tmp_path / "plan.txt"
    monkeypatch.setenv("DSX_PLAN_DUMP", str(path))
    sizing, planning, launches = engine.plan_dry_run(cfg, dt, case["B"], case["H"], case["W"], 0)
    ops = read_dump(str(path))
    assert sizing == planning and sizing > 0 and len(ops) == launches, (name, dt, env, sizing, planning, launches)
    return ops, kw["norm_groups"]


@pytest.mark.parametrize("name,dt,env", DRY, ids=lambda v: v if isinstance(v, str) else "+".join(k for k, _ in v) or "default")
def test_finalize_launchers(name, dt, env, tmp_path, monkeypatch):
    """every GroupNorm of the plan: the launch rule against the dumped launcher, the hosts of the hosted finalizes, and
    what k_conv_img may take"""
    ops, groups = _dump(name, dt, env, tmp_path, monkeypatch)
    fins = finalizes(ops, groups)        # (asserts that a GroupNorm conv without a finalize launch follows a `+gn` launch)
    # one finalize per conv with a GroupNorm in front, or the conv is an img launch that finalizes in its prologue
    n_gn = sum(1 for op in ops if op["conv"] is not None and op["conv"].has_gn)
    n_img = sum(1 for op in ops if op["launcher"] == "conv_img" and op["conv"].has_gn)
    assert len(fins) == n_gn - n_img and n_gn > 20, (len(fins), n_gn, n_img)
    for f in fins:
        if f["host"] == "hosted":
            continue
        # launch_gn_finalize: more than 512 (channel, partial row) pairs per group -> four waves per (image, group)
        wide = f["cpg"] * max(f["nchunk0"], f["nchunk1"]) > 512
        assert f["host"] == ("gn_finalize_wide" if wide else "gn_finalize"), f
        assert f["nchunk0"] >= 1 and (f["nchunk1"] >= 1) == (f["C1"] > 0), f
    # hosted: one per `+gn` launch, the GroupNorm of the next conv launch; none with DSX_HOST_FIN=0
    hosts = [i for i, op in enumerate(ops) if op["desc"].endswith(" +gn")]
    assert len(hosts) == sum(f["host"] == "hosted" for f in fins)
    for i in hosts:
        assert ops[i]["launcher"] == "conv_ws" and ops[i]["ks"] == 1 and not ops[i]["conv"].has_gn
        assert ops[i + 1]["conv"] is not None and ops[i + 1]["conv"].has_gn and ops[i + 1]["ks"] == 3, ops[i + 1]["desc"]
    if ("DSX_HOST_FIN", "0") in env or ("DSX_WS", "0") in env:
        assert not hosts
    # conv_img_applicable: a GroupNorm of more than 64 channels per group, of a count that is no power of two, or whose
    # groups straddle the sources is not finalized in the consumer
    for op in ops:
        c = op["conv"]
        if op["launcher"] == "conv_img" and c.has_gn:
            cpg = (c.C0 + c.C1) // groups
            assert cpg <= 64 and cpg & (cpg - 1) == 0 and c.C0 % cpg == 0, op["desc"]
        if c is not None and c.has_gn and (c.Hs, c.Ws, c.Ho, c.Wo) == (8, 8, 8, 8):
            cpg = (c.C0 + c.C1) // groups
            if cpg > 64 or cpg & (cpg - 1):
                assert op["launcher"] in ("conv_mfma", "conv_ws"), op["desc"]
                assert any(f["consumer"] is op for f in fins), op["desc"]


def test_reach(tmp_path, monkeypatch):
    """every operand type reaches every condition of tests/test_gpu_groups.py REACH (or is exempt, with a reason), and
    the plans the module adds for one path reach it"""
    by_dt, by_plan = {}, {}
    for plan, (name, dt, env, flat) in PLANS.items():
        ops, groups = _dump(name, dt, tuple(sorted(env.items())), tmp_path, monkeypatch)
        by_plan[plan] = group_reach_tags(ops, groups)
        by_dt.setdefault(dt, set()).update(by_plan[plan])
    for dt in ("bf16", "f16", "f32"):
        missing = set(REACH) - set(REACH_EXEMPT.get(dt, {})) - by_dt[dt]
        assert not missing, f"{dt}: never reached: {sorted(missing)}"
        assert set(REACH_EXEMPT.get(dt, {})) <= set(REACH)
        # g1 alone, at default knobs: every condition, in every operand type
        assert by_plan[f"g1_{dt}"] == set(REACH), (dt, set(REACH) - by_plan[f"g1_{dt}"])
        # g2: the straddling groups of 192 channels (256 + 128: 192 / 64 and 64 / 128 of a group per source); g3: 72 and
        # 96 channels per group on an 8 x 8 map
        assert {"straddle>64", "npow2>64", "wide own>64", "f32part>64", "shifted>64"} <= by_plan[f"g2_{dt}"]
        assert {"straddle>64", "npow2>64", "fin>64", "wide own>64", "8x8 no img"} <= by_plan[f"g3_{dt}"]
    for plan in ("g2_bf16_ws", "g2_f32_ws"):
        assert {"hosted>64", "fin>64"} <= by_plan[plan], plan
    assert "hosted>64" not in by_plan["g1_f16_no_host"] and "hosted>64" in by_plan["g1_f16"]


def test_straddling_groups_of_g2(tmp_path, monkeypatch):
    """the concat of 256 + 128 channels in two groups: group 0 takes 192 channels of source 0, group 1 its last 64 and
    all 128 of source 1 -- accumulate() with n0 = 64, n1 = 128 --, and 128 + 64 channels in groups of 96: n0 = 32,
    n1 = 64; in every operand type, by k_gn_finalize_wide.  (n0 > 64 with n1 > 0 is g1's: one group over 256 + 128,
    256 + 256 and 128 + 64 channels.)"""
    for dt in ("bf16", "f16", "f32"):
        ops, groups = _dump("g2", dt, (), tmp_path, monkeypatch)
        split = set()
        for f in finalizes(ops, groups):
            if f["C1"] and f["C0"] % f["cpg"]:
                g = f["C0"] // f["cpg"]                      # the group that straddles
                n0 = f["C0"] - g * f["cpg"]
                split.add((f["host"], f["cpg"], n0, f["cpg"] - n0))
        assert split == {("gn_finalize_wide", 192, 64, 128), ("gn_finalize_wide", 96, 32, 64)}, (dt, split)
        ops, groups = _dump("g1", dt, (), tmp_path, monkeypatch)
        whole = {(f["C0"], f["C1"]) for f in finalizes(ops, groups) if f["C1"]}
        assert {(256, 128), (256, 256), (128, 64)} <= whole, (dt, whole)
