"""The planner's choice of the direct rows of k_conv_ws (ConvArgs::ws_direct, knob DSX_WS_DIRECT), without a GPU: which
launches of the benchmark's plan take them, that the knob changes nothing else, and that the small plans of
tests/test_gpu_direct.py reach what that module is there to run."""
import pytest

from tests.direct_cases import CASES, DIRECT_ENV, DIRECT_ROWS, PLANS, direct_flag, make_cfg
from tests.plan_cases import CONFIGS
from tests.plan_dump import read_dump

# the plain 1 x 1 launches of C2 (sr_sr3_16_128, B = 16, bf16): 14 residual convs and 5 attention output projections
C2_DIRECT = (
    ["conv1x1 128->256 @32x32 tile64x128 ws +gn", "conv1x1 256->512 @16x16 tile64x128 ws c4 +gn"]
    + ["conv1x1 512->512 @16x16 tile64x128 ws c4"] * 2
    + ["conv1x1 1024->512 @16x16 tile64x128 ws c4 +gn", "conv1x1 512->512 @16x16 tile64x128 ws c4"] * 2
    + ["conv1x1 768->512 @16x16 tile64x128 ws c4 +gn", "conv1x1 512->512 @16x16 tile64x128 ws c4",
       "conv1x1 768->256 @32x32 tile64x128 ws c4 +gn", "conv1x1 512->256 @32x32 tile64x128 ws c4 +gn",
       "conv1x1 384->256 @32x32 tile64x128 ws c4 +gn", "conv1x1 384->128 @64x64 tile64x128 ws c4 +gn",
       "conv1x1 256->128 @64x64 tile64x128 ws c4 +gn", "conv1x1 192->128 @64x64 tile64x128 ws +gn",
       "conv1x1 192->64 @128x128 tile128x64 ws +gn"]
    + ["conv1x1 128->64 @128x128 tile128x64 ws +gn"] * 2)


def _dump(cfg, dt, B, H, W, cc, tmp_path, monkeypatch, env):
    from diffsplitting_amd import engine
    for k in ("DSX_WS_DIRECT",) + tuple(DIRECT_ENV):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = tmp_path / "plan.txt"
    monkeypatch.setenv("DSX_PLAN_DUMP", str(path))
    sizing, planning, launches = engine.plan_dry_run(cfg, dt, B, H, W, cc)
    return read_dump(str(path)), sizing, planning, launches


def _c2_cfg():
    from diffsplitting_amd import engine
    flavour, kw, B, H, W, cc = CONFIGS["c2_sr3_128_b16"]
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    return cfg, B, H, W, cc


def test_headline_plan_marks_the_plain_1x1_launches(tmp_path, monkeypatch):
    cfg, B, H, W, cc = _c2_cfg()
    on, *_ = _dump(cfg, "bf16", B, H, W, cc, tmp_path, monkeypatch, {})
    marked = [op["desc"] for op in on if direct_flag(op)]
    assert len(C2_DIRECT) == 19 and marked == C2_DIRECT
    for op in on:
        if direct_flag(op):        # a plain 1 x 1 conv on the persistent kernel
            assert op["launcher"] == "conv_ws" and op["ks"] == 1 and not op["conv"].has_gn and not op["conv"].swish
        elif op["launcher"] == "conv_ws" and op["ks"] == 1:   # every other 1 x 1 launch of it has a GroupNorm in front
            assert op["conv"].has_gn, op["desc"]
    off, *_ = _dump(cfg, "bf16", B, H, W, cc, tmp_path, monkeypatch, {"DSX_WS_DIRECT": "0"})
    assert not any(direct_flag(op) for op in off)
    assert [(op["kind"], op["desc"]) for op in off] == [(op["kind"], op["desc"]) for op in on]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_both_settings_reserve_the_same_bytes(name, tmp_path, monkeypatch):
    from diffsplitting_amd import engine
    flavour, kw, B, H, W, cc = CONFIGS[name]
    cfg = engine.make_cfg(flavour, kw["in_channel"], kw["out_channel"], kw["inner_channel"], kw["norm_groups"],
                          kw["channel_mults"], kw["attn_res"], kw["res_blocks"], kw["image_size"])
    for dt in ("f32", "bf16", "f16"):
        got = {}
        for knob in ("1", "0"):
            ops, sizing, planning, launches = _dump(cfg, dt, B, H, W, cc, tmp_path, monkeypatch, {"DSX_WS_DIRECT": knob})
            assert sizing == planning and sizing > 0, (name, dt, knob, sizing, planning)
            got[knob] = (sizing, launches, [(op["kind"], op["desc"]) for op in ops])
        assert got["1"] == got["0"], (name, dt)


def test_small_plans_reach_every_direct_row(tmp_path, monkeypatch):
    """what tests/test_gpu_direct.py runs: per operand type every compiled direct row, a one-source and a two-source
    input, a hosted GroupNorm finalize, and a K tail (Cin no multiple of the item's channels)"""
    reach = {}
    for name, dt in PLANS:
        case = CASES[name]
        on, *_ = _dump(make_cfg(case), dt, case["B"], case["H"], case["W"], 3, tmp_path, monkeypatch, DIRECT_ENV)
        off, *_ = _dump(make_cfg(case), dt, case["B"], case["H"], case["W"], 3, tmp_path, monkeypatch,
                        dict(DIRECT_ENV, DSX_WS_DIRECT="0"))
        assert [(op["kind"], op["desc"]) for op in off] == [(op["kind"], op["desc"]) for op in on]
        assert not any(direct_flag(op) for op in off)
        r = reach.setdefault(dt, set())
        n = 0
        for op in on:
            if not direct_flag(op):
                continue
            n += 1
            c = op["conv"]
            cpg = c.ws_cpg if c.ws_cpg else 2
            assert (op["tile"], cpg) in DIRECT_ROWS, op["desc"]
            r.add((op["tile"], cpg))
            r.add("two sources" if c.C1 else "one source")
            if op["desc"].endswith("+gn"):
                r.add("hosted finalize")
            if (c.C0 + c.C1) % (cpg * (16 if dt == "f32" else 32)):
                r.add("k tail")
        assert n > 0, (name, dt)
    want = set(DIRECT_ROWS) | {"one source", "two sources", "hosted finalize", "k tail"}
    for dt in ("bf16", "f16", "f32"):
        assert reach[dt] == want, (dt, want - reach[dt])
