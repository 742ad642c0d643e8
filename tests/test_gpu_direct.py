"""The direct rows of k_conv_ws (ConvArgs::ws_direct) against the path they replace.

A plain 1 x 1 conv -- no GroupNorm, no Swish in front: the residual convs and the attention output projections -- can
take a direct row: the loader waves DMA its activation units straight into swizzled MFMA images instead of copying them
through the raw ring.  The weight stream, the MFMA order, the epilogue and the fused statistics are the same code, so a
direct launch must write exactly the bytes the ring path writes.  Per plan (tests/direct_cases.py: the smallest models
that reach every compiled row in every operand type, one- and two-source inputs, hosted GroupNorm finalizes and K tails
whose last channel units the buffer descriptor zero-fills; tests/test_direct_plan_cpu.py holds that reach on the CPU):

  * one forward with DSX_WS_DIRECT=1 and one with 0 from the same inputs: the outputs and every conv launch's output in
    the layer table are torch.equal, no hand-off timed out, and a second forward of the direct plan repeats bitwise;
  * the direct plan passes the fp64 per-layer checker (tests/layer_check.py) with its bounds as they are.

Not reached at these sizes: a workgroup with more items than images, i.e. a DMA into an image that was read before (at
most 6 items per workgroup here, 5 to 8 images).  The benchmark's plans in tests/test_gpu_layers.py (B = 16, every
operand type, 12 to 24 items per workgroup at the 64^2 and 128^2 levels) run the direct rows through that."""
import time

import pytest
import torch

from oracle.weights import synth_state_dict
from tests.direct_cases import CASES, DIRECT_ENV, PLANS, make_cfg
from tests.gpu_util import build_engine
from tests.layer_check import check_plan, inputs
from tests.nets import dev  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEED = 41
_SD = {}


def _state_dict(name):
    if name not in _SD:
        from diffsplitting_amd import engine
        eng = engine.UNetEngine(make_cfg(CASES[name]), CASES[name]["flavour"])
        _SD[name] = synth_state_dict(zip(eng.param_names, eng.param_shapes), seed=SEED)
    return _SD[name]


def _forward(case, sd, dt, x, t, dev, monkeypatch, direct, repeat):
    """[y of each forward], layer table after the last one -- of an engine planned with DSX_WS_DIRECT=`direct`"""
    monkeypatch.setenv("DSX_WS_DIRECT", direct)
    eng = build_engine(case["cfg"], case["flavour"], sd, dtype=dt)
    ys = [eng.forward(x.to(dev), t.to(dev)).clone() for _ in range(repeat)]
    table = eng.layer_table(case["B"], case["H"], case["W"])
    assert eng.handoff_timeouts() == 0
    return ys, table


@pytest.mark.parametrize("name,dt", PLANS, ids=[f"{n}_{d}" for n, d in PLANS])
def test_direct_rows_write_the_bytes_of_the_ring_path(name, dt, dev, monkeypatch):
    t0 = time.time()
    case, sd = CASES[name], _state_dict(name)
    x, t = inputs(case, case["B"], case["H"], case["W"])
    for k, v in DIRECT_ENV.items():
        monkeypatch.setenv(k, v)
    (y1, y1b), tab1 = _forward(case, sd, dt, x, t, dev, monkeypatch, "1", 2)
    (y0,), tab0 = _forward(case, sd, dt, x, t, dev, monkeypatch, "0", 1)
    assert torch.equal(y1, y1b), "the direct plan does not repeat bitwise"
    assert torch.equal(y1, y0), "DSX_WS_DIRECT changes the output"
    assert [L["desc"] for L in tab1] == [L["desc"] for L in tab0]
    convs = 0
    for L1, L0 in zip(tab1, tab0):
        if L1["kind"] != 0:
            continue
        convs += 1
        assert torch.equal(L1["out"], L0["out"]), f"{L1['desc']} ({L1['w_name']}): DSX_WS_DIRECT changes its output"
    assert convs > 10
    print(f"\n{name}_{dt}: {convs} conv outputs bit-equal in {time.time() - t0:.1f} s")


@pytest.mark.parametrize("name,dt", PLANS, ids=[f"{n}_{d}" for n, d in PLANS])
def test_direct_plan_every_layer_against_fp64(name, dt, dev, monkeypatch):
    case = CASES[name]
    x, t = inputs(case, case["B"], case["H"], case["W"])
    env = dict(DIRECT_ENV, DSX_WS_DIRECT="1")
    check_plan(f"{name}_{dt}_direct", case, _state_dict(name), dt, case["B"], case["H"], case["W"], env, x, t, dev,
               monkeypatch)
    torch.cuda.empty_cache()
