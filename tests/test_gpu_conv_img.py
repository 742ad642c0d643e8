"""k_conv_img in every instantiation: each image-resident launch of the smallest model with a full 8 x 8 level
(tests/test_conv_img_plan_cpu.py pins which launches those are and what they cover) against a float64 reference of that
one layer, computed from the tensors the launch read (tests/layer_ref.py: the bounds are derived there, none is added
here), and a second forward of the same input, which must reproduce every one of these outputs bit for bit: the
kernel's loads, conversions and MFMAs overlap freely, the order of every sum is fixed."""
import pytest
import torch

import bench
from tests import layer_ref
from tests.gpu_util import build_engine
from tests.plan_cases import COND_CHANNELS, IMG_LAUNCHES, IMG_MODEL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
B = 3


@pytest.mark.parametrize("dt", list(DT))
def test_img_launches_against_fp64_and_repeatable(dt):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    from diffsplitting_amd import engine
    cfg = engine.make_cfg("sr3", **IMG_MODEL)
    probe = engine.UNetEngine(cfg, "sr3")
    sd = bench.random_init_state_dict(probe.param_names, probe.param_shapes, seed=11)
    del probe
    eng = build_engine(IMG_MODEL, "sr3", sd, dtype=dt)
    H = IMG_MODEL["image_size"]
    g = torch.Generator().manual_seed(77)
    x = torch.randn((B, IMG_MODEL["in_channel"], H, H), generator=g).to(dev)
    t = (0.05 + 0.9 * torch.rand((B, 1), generator=g)).to(dev)

    def img_layers():
        eng.forward(x, t, cond_channels=COND_CHANNELS)
        return [L for L in eng.layer_table(B, H, H, COND_CHANNELS) if L["kind"] == 0 and L["desc"].endswith(" img")]

    first = img_layers()
    seen = {}
    for L in first:
        seen[L["desc"]] = seen.get(L["desc"], 0) + 1
    assert seen == IMG_LAUNCHES
    fails, worst = [], (0.0, "")
    for L in first:
        where = f"[{dt}] {L['desc']} ({L['w_name']})"
        w = sd[L["w_name"]].to(dev)
        bias = None if (L["bias_in_film"] or L["b_name"] is None) else sd[L["b_name"]].to(dev)
        gamma = sd[L["gn_gamma_name"]].to(dev) if L["gn_gamma_name"] else None
        beta = sd[L["gn_beta_name"]].to(dev) if L["gn_beta_name"] else None
        v = layer_ref.check_conv(L, w, bias, gamma, beta, IMG_MODEL["norm_groups"], DT[dt], None, where)
        if v.ratio > worst[0]:
            worst = (v.ratio, where)
        if not v.ok:
            fails.append(v.message())
    print(f"\n{dt}: {len(first)} img launches checked, worst error/bound {worst[0]:.3f} at {worst[1]}")
    assert not fails, f"{len(fails)} check(s) failed:\n" + "\n".join(fails[:20])
    second = img_layers()
    assert [L["desc"] for L in second] == [L["desc"] for L in first]
    diff = [f"{i}: {a['desc']}" for i, (a, b) in enumerate(zip(first, second)) if not torch.equal(a["out"], b["out"])]
    assert not diff, f"[{dt}] img launches whose output changed between two forwards of one input: {diff}"
    assert eng.handoff_timeouts() == 0
