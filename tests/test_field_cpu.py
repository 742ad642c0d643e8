"""Frame-keyed noise and the Gaussian tiled path, without a GPU: dsx_tileplan_randn is declared, bound and exported; its
host checks (the shared plan-form checks and the three refusals of its own) with fake device pointers; the new flags
of ``split``; ``noise_field`` against the two other noise sources; and the planner on the 3 -> 2 UNet of the reference's
``config/splitting.json``."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.host_checks import ERR_INVALID, FAKE, cpu_samplers, last_error
from tests.nets import write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_bound_and_exported():
    from diffsplitting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dsx.h")).read()
    m = re.search(r"int dsx_tileplan_randn\(([^)]*)\);", hdr)
    assert m, "include/dsx.h declares dsx_tileplan_randn"
    names = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names == ["plan", "C", "first", "stride", "count", "seed", "id_base", "draw", "out_dev", "stream"]
    res, kinds = _lib.SIGNATURES["dsx_tileplan_randn"]
    assert res is C.c_int and len(kinds) == 10
    assert kinds[0] == _lib.Handle and kinds[8] == _lib.Dev("float") and kinds[9] == _lib.Stream
    assert kinds[7] is C.c_uint32 and kinds[5] is C.c_uint64 and kinds[6] is C.c_uint64
    assert hasattr(_lib._cdll, "dsx_tileplan_randn") and callable(_lib.lib.dsx_tileplan_randn)
    assert _lib.lib.dsx_abi_version() == 2                            # additive under the same ABI version
    assert re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", hdr)


@pytest.fixture(scope="module")
def plan():
    from diffsplitting_amd.data.tiling import TilePlan
    p = TilePlan((2, 40, 57), (1, 8, 8), (1, 16, 16))                 # the plan of test_tiles_checks_cpu.py
    assert p.total == 56
    return p


def _randn(h, first, stride, count, Cn=2, seed=1, id_base=0, draw=0, out=FAKE):
    from diffsplitting_amd import _lib
    return _lib.lib.dsx_tileplan_randn(h, Cn, first, stride, count, seed, id_base, draw, out, None)


def test_the_shared_plan_form_checks_hold(plan):
    """the message format of geom_of_plan and of the count limit, under the name tileplan_randn"""
    for first, stride, count in ((plan.total, 1, 1), (0, 0, 2), (1, 2 ** 62, 3), (-1, 1, 1), (plan.total - 3, 1, 4),
                                 (1, 2, 29), (0, -1, 2)):
        assert _randn(plan.handle, first, stride, count) == ERR_INVALID, (first, stride, count)
        assert f"tileplan_randn: tiles {first} + k * {stride} ({count} of them) leave the plan (56 tiles)" in last_error()
    for count in (65536, -1):
        assert _randn(plan.handle, 0, 1, count) == ERR_INVALID
        assert f"tileplan_randn: count = {count}" in last_error() and "65535" in last_error()
    assert _randn(None, 0, 1, 1) == ERR_INVALID and "tileplan_randn: null argument" in last_error()
    assert _randn(plan.handle, 0, 1, 0) == 0                          # nothing to do: no error, and no device
    assert _randn(plan.handle, 0, 1, 0, out=None) == 0
    assert _randn(plan.handle, 0, 1, 1, out=None) == ERR_INVALID and "tileplan_randn: null argument" in last_error()


def test_the_refusals_of_its_own_are_by_name(plan):
    from diffsplitting_amd import _lib
    for Cn in (0, -3):
        assert _randn(plan.handle, 0, 1, 1, Cn=Cn) == ERR_INVALID and f"tileplan_randn: C = {Cn}" in last_error()
    lim = _lib.STREAM_ID_LIMIT
    for id_base in (lim - 1, lim, 2 ** 64 - 1):                       # two frames: id_base + 1 must stay below 2^40
        assert _randn(plan.handle, 0, 1, 1, id_base=id_base) == ERR_INVALID
        assert f"tileplan_randn: id_base = {id_base} with 2 frames" in last_error() and "2^40" in last_error()
    assert _randn(plan.handle, 0, 1, 0, id_base=lim - 2) == 0         # the last pair of ids that fits
    for draw in (_lib.STREAM_DRAW_LIMIT, 2 ** 32 - 1):
        assert _randn(plan.handle, 0, 1, 1, draw=draw) == ERR_INVALID
        assert f"tileplan_randn: draw ordinal {draw}" in last_error() and "2^24" in last_error()
    assert _randn(plan.handle, 0, 1, 0, draw=_lib.STREAM_DRAW_LIMIT - 1) == 0


def test_randn_field_refuses_on_the_python_side_too(plan, monkeypatch):
    from diffsplitting_amd import _lib
    from diffsplitting_amd._lib import DsxError
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)            # the refusals come before any device work
    with pytest.raises(DsxError, match="tile id out of range"):
        plan.randn_field([0, 56], 2, seed=1)
    with pytest.raises(DsxError, match="randn_field: C = 0"):
        plan.randn_field([0], 0, seed=1)
    with pytest.raises(DsxError, match="randn_field: draw ordinal"):
        plan.randn_field([0], 2, seed=1, draw=1 << 24)
    with pytest.raises(DsxError, match="randn_field: id_base"):
        plan.randn_field([0], 2, seed=1, id_base=(1 << 40) - 1)


# ----------------------------------------------------------------------------- command line
def test_split_refuses_the_new_flags_where_they_do_not_apply(tmp_path, monkeypatch):
    """Every refusal is a SystemExit that names the flag, raised on the command line and the config alone: no rank is
    started and nothing touches the device."""
    from diffsplitting_amd import parallel, split

    def touched(*a, **k):
        raise AssertionError("the refusal came too late: a rank was started or the device was initialised")
    monkeypatch.setattr(parallel, "init", touched)
    monkeypatch.setattr(parallel, "self_launch", touched)
    monkeypatch.setattr(split, "create_model", touched)
    cfgs = {w: write_config(tmp_path, w) for w in ("sr3", "ddpm", "indi", "joint_indi")}

    def refused(argv, match, config="sr3"):
        with pytest.raises(SystemExit, match=match):
            split.main(["-c", cfgs[config]] + argv)

    for which in ("indi", "joint_indi"):
        refused(["--solver", "ddim", "--solver-steps", "4"], f"--solver.*sr3 / ddpm.*{which}", config=which)
    for which in ("sr3", "ddpm"):
        refused(["--solver", "dpmpp2m"], "--solver needs --solver-steps", config=which)
    refused(["--solver-steps", "4"], "--solver-steps: only with --solver")
    refused(["--eta", "0.5"], "--eta: only with --solver")
    refused(["--spacing", "uniform"], "--spacing: only with --solver")
    refused(["--solver", "ddim", "--solver-steps", "0"], "--solver-steps 0")
    refused(["--solver", "dpmpp2m", "--solver-steps", "4", "--eta", "0.5"], "--eta 0.5.*dpmpp2m")
    refused(["--solver", "ddim", "--solver-steps", "4", "--eta", "1.5"], r"eta must lie in \[0, 1\]")
    refused(["--solver", "ddim", "--solver-steps", "4", "--validate"], "--solver.*--validate")
    refused(["--noise-field"], "--noise-field needs --sample-seed")
    refused(["--noise-field", "--sample-seed", "3", "--validate"], "--noise-field.*--validate")
    refused(["--noise-field", "--sample-seed", "3", "--mix-t", "0.3", "--t-from", "given"], "--noise-field.*--mix-t",
            config="joint_indi")
    with pytest.raises(SystemExit):                                   # argparse's own: not one of the two solvers
        split.main(["-c", cfgs["sr3"], "--solver", "euler", "--solver-steps", "4"])


# ----------------------------------------------------------------------------- the draw hook
def test_noise_field_is_refused_together_with_the_other_sources(monkeypatch):
    """by name, before anything is drawn or any kernel runs (the field and the source would raise if asked)"""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.model import samplers

    def asked(*a, **k):
        raise AssertionError("a draw was taken before the refusal")
    monkeypatch.setattr(samplers._SamplerBase, "_need_cuda", staticmethod(lambda *a, **k: None))
    g, i, j = cpu_samplers()
    assert g.noise_field is None and i.noise_field is None and j.noise_field is None
    x = torch.zeros(2, 1, 32, 32)
    calls = [lambda kw: g.p_sample_loop(x, **kw), lambda kw: g.solver_sample_loop(x, steps=4, **kw),
             lambda kw: g.super_resolution(x, **kw), lambda kw: i.inference(x, **kw),
             lambda kw: i.inference(x, t_float_start=[0.5, 0.25], **kw), lambda kw: j.inference(x, **kw)]
    state = torch.get_rng_state()
    for s in (g, i, j):
        s.noise_field = asked
    for call in calls:
        with pytest.raises(DsxError, match="noise_field together with sample_ids"):
            call(dict(seed=3, sample_ids=[0, 1]))
    for s in (g, i, j):
        s.noise_source = asked
    for call in calls:
        with pytest.raises(DsxError, match="noise_field together with noise_source"):
            call({})
    assert torch.equal(torch.get_rng_state(), state)                  # torch's generator is left alone


# ----------------------------------------------------------------------------- the planner
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("size", [32, 64, 512])
def test_the_splitting_unet_plans(dtype, size):
    """config/splitting.json of the reference: sr3, UNet 3 -> 2 (one condition channel + two noisy target channels),
    inner 16, groups 16, mults (1, 2, 4, 8), one res block, no attention -- at a tile of a small test, of the end-to-end
    test and of the config's own 512^2 patches, a batch of 8 and a single tile"""
    from diffsplitting_amd import engine
    cfg = engine.make_cfg("sr3", 3, 2, 16, 16, (1, 2, 4, 8), (), 1, 512)
    for B in (1, 8):
        sizing, planning, launches = engine.plan_dry_run(cfg, dtype, B, size, size, cond_channels=1)
        assert sizing > 0 and planning > 0 and launches > 0
