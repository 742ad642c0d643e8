"""Which image-resident launches (k_conv_img) the smallest model with a full 8 x 8 level plans, and what they cover
(planner dry run: no GPU, no compute).  tests/test_gpu_conv_img.py checks exactly these launches on the device; this
file pins its coverage claim: every instantiation of the kernel (both kernel sizes, NPH 2 / 4 / 8 in every operand
type), one- and two-source inputs, GroupNorm with and without Swish, residual and output statistics on and off."""
import collections
import re

import pytest

from tests.plan_cases import COND_CHANNELS, IMG_LAUNCHES, IMG_MODEL
from tests.plan_dump import read_dump

# channel phases (8 waves x one 64-byte chunk each) -> the NPH the launcher instantiates: 2 and 4 exactly, 8 for the rest
PHASES = {"bf16": {1, 2, 3, 4}, "f16": {1, 2, 3, 4}, "f32": {2, 4, 6, 8}}
NPH = {"bf16": {1: 8, 2: 2, 3: 8, 4: 4}, "f16": {1: 8, 2: 2, 3: 8, 4: 4}, "f32": {2: 2, 4: 4, 6: 8, 8: 8}}


def img_launches(dt, B, path, monkeypatch):
    """[(description, ks, ConvArgsHead)] of the plan's image-resident launches, in launch order"""
    from diffsplitting_amd import engine
    cfg = engine.make_cfg("sr3", **IMG_MODEL)
    monkeypatch.setenv("DSX_PLAN_DUMP", str(path))
    H = IMG_MODEL["image_size"]
    a, b, n = engine.plan_dry_run(cfg, dt, B, H, H, COND_CHANNELS)
    assert a == b
    ops = read_dump(path)
    assert len(ops) == n
    out = []
    for o in ops:
        if o["desc"].endswith(" img"):
            assert o["launcher"] == "conv_img" and o["kind"] == 0, o["desc"]
            out.append((o["desc"], o["ks"], o["conv"]))
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_img_launches_of_the_smallest_8x8_model(dt, B, tmp_path, monkeypatch):
    L = img_launches(dt, B, tmp_path / "plan.txt", monkeypatch)
    assert dict(collections.Counter(d for d, _, _ in L)) == IMG_LAUNCHES
    kc = 16 if dt == "f32" else 32                     # channels of a 64-byte chunk
    phases, sizes, sources, acts, resid, stats = set(), set(), set(), set(), set(), set()
    for desc, ks, a in L:
        m = re.match(r"conv(\d)x\d (\d+)->(\d+) @8x8 img$", desc)
        assert int(m.group(1)) == ks and int(m.group(2)) == a.C0 + a.C1 and int(m.group(3)) == a.Cout, desc
        assert (a.B, a.Hs, a.Ws, a.Ho, a.Wo, a.up) == (B, 8, 8, 8, 8, 0), desc
        assert (a.C0 + a.C1) % (8 * kc) == 0 and a.kchunks * kc == a.C0 + a.C1, desc
        assert not (a.swish and not a.has_gn), desc
        phases.add((a.C0 + a.C1) // (8 * kc))
        sizes.add(ks)
        sources.add((a.C0, a.C1))
        acts.add((bool(a.has_gn), bool(a.swish)))
        resid.add(a.resid is not None)
        stats.add(a.stat_part is not None)
    assert phases == PHASES[dt]
    assert {NPH[dt][p] for p in phases} == {2, 4, 8}   # every instantiation of the operand type ...
    assert sizes == {1, 3}                             # ... in both kernel sizes
    for ks in (1, 3):
        assert {NPH[dt][(a.C0 + a.C1) // (8 * kc)] for _, k, a in L if k == ks} == {2, 4, 8}, ks
    assert {(512, 0), (512, 512), (512, 256)} <= sources
    assert acts == {(True, True), (True, False), (False, False)}   # GroupNorm + Swish, GroupNorm alone (qkv), neither
    assert resid == {False, True}
    assert stats == {False, True}
