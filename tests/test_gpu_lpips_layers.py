"""Every LPIPS launch on the MI355X against float64, element by element, on uneven tile grids.  `-m gpu`.

One forward per case; `LPIPS.layer_table()` hands back every stage of it and tests/lpips_layer_ref.py recomputes each
launch from the tensor that launch read: the input scaling and the pools must be equal, every conv element within the
fp32-conv bound of tests/layer_ref.py, every partial row of a tap's distance within a bound propagated through the
kernel's fp32 roundings, the finish within one fp32 rounding.  tests/test_lpips_layers_cpu.py shows that these checks
reject a dropped tap, a shifted or transposed tile, a wrong halo, a short pool window, a swapped channel pair and a
lost partial row.  Run with -s for the worst error / bound ratio of each launch.

The sizes come from conv1_out(n) = (n - 7) // 4 + 1 and pool_out(n) = (n - 3) // 2 + 1; REACH names what they are
chosen for and test_reach says what an edited size lost.

End to end, the total and the five taps are also compared with the float64 restatement (tests/lpips_ref.py) under a
bound built as lpips_ref.bound() is -- MARGIN x the fp32-against-fp64 error of the restatement, relative, plus the
floor -- with the yardstick taken over THESE cases (`yardstick()` below; lpips_ref.bound() is untouched).  Its value
on the CPU: 9.24e-7 on the build host, at tap 4 of the 31 x 31 case, where taps 3..5 are a single pixel each, and
1.03e-6 on the GPU host's 16 threads (lpips_ref's own cases give 9.02e-7 on the build host: the 1 x 1 map asks for
hardly more).  Measured on the device (worst error / bound over the cases): conv1 0.070, conv2 0.031, conv3..5 0.026,
distance rows 0.014, finish 0.85 (one fp32 rounding); end to end at most 0.05 of the bound.
"""
import functools
import time

import pytest
import torch

from tests import lpips_layer_ref as L
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# name -> (B, H, W, seed): conv1 map, conv2 map, conv3..5 map
CASES = {"min_31": (1, 31, 31, 21),            # 7 x 7, 3 x 3, 1 x 1: the minimum, conv3..5 all halo
         "row_31x287": (2, 31, 287, 22),       # 7 x 71, 3 x 35, 1 x 17: 1 x 5, 1 x 3 and 1 x 2 tiles
         "col_287x31": (2, 287, 31, 23),       # the same, transposed
         "c1_67x71": (1, 67, 71, 24),          # 16 x 17, 7 x 8, 3 x 3: conv1 at an exact tile and one pixel over
         "c2_135x143": (1, 135, 143, 25),      # 33 x 35, 16 x 17, 7 x 8: conv2 at an exact tile and one pixel over
         "c3_271x287": (1, 271, 287, 26),      # 67 x 71, 33 x 35, 16 x 17: conv3..5 at an exact tile and one pixel over
         "cap_1031": (1, 1031, 1031, 27)}      # 257 x 257 = 66049 > 65536 pixels: nblk capped at 1024, ppb = 65
# only the launches in front of conv2: nothing behind them adds coverage at this size, and conv2's float64 reference
# at 128 x 128 would dominate the time
BIG = {"cap_1031"}
# what the cases together must have met, per conv level where it can occur (a 1 x 1 map: only behind both pools; a
# capped nblk: only tap 1 at a size a test can afford)
REACH = ({f"{lvl} {tag}" for lvl in ("conv1", "conv2", "conv3")
          for tag in ("tiles_x>tiles_y", "tiles_x<tiles_y", "0mod16", "1mod16")} | {"conv3 1x1", "dist1 capped"})
_CHECKED = {}


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    from diffsplitting_amd.core.lpips import LPIPS
    return LPIPS(net='alex', state_dict=sd).cuda()


@functools.lru_cache(maxsize=None)
def restatement(case, dtype):
    """(total, taps) of the restatement for a case, computed once and shared"""
    in0, in1 = R.make_pair(*CASES[case])
    return R.lpips_ref(R.synth_state_dict(), in0, in1, dtype, per_layer=True)


@functools.lru_cache(maxsize=None)
def yardstick():
    """lpips_ref.fp32_yardstick() over the cases of this module: the largest relative error, totals and taps, of the
    restatement evaluated in float32 against its float64 form"""
    worst = 0.0
    for case in CASES:
        for a32, a64 in zip(restatement(case, torch.float32), restatement(case, torch.float64)):
            worst = max(worst, ((a32.double() - a64).abs() / a64.abs().clamp_min(1e-30)).max().item())
    return worst


def bound(expected):
    """as lpips_ref.bound(), on this module's yardstick"""
    return R.MARGIN * yardstick() * expected.abs().double() + R.ABS_FLOOR


def _end_to_end(name, got, want):
    got, want = got.detach().double().cpu().reshape(want.shape), want.double()
    err, lim = (got - want).abs(), bound(want)
    print(f"  {name}: max |device - fp64| = {err.max().item():.3e} (relative {(err / want.abs()).max().item():.3e}), "
          f"{(err / lim).max().item():.2f} of the bound")
    assert bool((err <= lim).all()), (name, got, want, err, lim)


@pytest.mark.parametrize("case", list(CASES))
def test_every_launch_against_fp64(model, sd, case):
    from diffsplitting_amd.core import lpips as M
    t0 = time.time()
    B, H, W, _ = CASES[case]
    in0, in1 = R.make_pair(*CASES[case])
    got, taps = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    launches = L.BIG_LAUNCHES if case in BIG else L.LAUNCHES
    table = model.layer_table(stages=("x0", "f1", "p1") if case in BIG else None)
    geo = M.geometry(H, W)
    assert table["pairs"] == B
    for s, v in table["stages"].items():
        assert tuple(v["out"].shape) == (2 * B,) + geo[s], (s, tuple(v["out"].shape), geo[s])
    assert geo["f1"][:2] == (L.conv1_out(H), L.conv1_out(W)) and geo["p1"][:2] == (L.pool_out(geo["f1"][0]),
                                                                                   L.pool_out(geo["f1"][1]))
    per_tap = torch.cat(taps, dim=1).reshape(B, 5)
    worst, fails = L.check_table(table, sd, in0, in1, per_tap, got.reshape(B), launches)
    t_layers = time.time() - t0
    print(f"\n{case}: worst error / bound per launch: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not fails, "\n".join(fails)
    assert set(worst) == set(launches)
    maps = {lvl: m for lvl, m in L.level_maps(table).items() if lvl in launches}
    dist = [(k + 1, t["hw"]) for k, t in enumerate(table["taps"]) if f"dist{k + 1}" in launches]
    _CHECKED[case] = L.reach_tags(maps, dist)
    # end to end, against the restatement
    want, want_taps = restatement(case, torch.float64)
    _end_to_end(f"{case} total", got, want)
    for k in range(5):
        _end_to_end(f"{case} tap {k + 1}", taps[k], want_taps[:, k])
    print(f"  {case}: {time.time() - t0:.1f} s ({t_layers:.1f} s per launch); yardstick {yardstick():.3e}; "
          f"reached {sorted(_CHECKED[case])}")


def test_constant_image_through_the_per_tap_check(model, sd):
    """where the 1e-10 matters: tap-1 features of the constant image are exactly zero, 0 / (0 + 1e-10) on that side"""
    in0, in1 = R.constant_image(1, 64, 64), R.make_pair(1, 64, 64, 9)[1]
    got, taps = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    table = model.layer_table()
    assert not table["stages"]["f1"]["out"][0].any() and table["stages"]["f1"]["out"][1].any()
    worst, fails = L.check_table(table, sd, in0, in1, torch.cat(taps, dim=1).reshape(1, 5), got.reshape(1))
    print("\nconstant image: worst error / bound per launch: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not fails, "\n".join(fails)
    assert torch.isfinite(table["taps"][0]["part"]).all() and (table["taps"][0]["part"] > 0).all()


def test_layer_table_contract(model, sd):
    """shapes equal geometry()'s; refused before any forward and after frames(); reading it changes no result"""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core import lpips as M
    fresh = M.LPIPS(state_dict=sd).cuda()
    with pytest.raises(DsxError, match="holds no whole forward"):
        fresh.layer_table()
    in0, in1 = R.make_pair(2, 97, 131, 4)
    a = fresh(in0.cuda(), in1.cuda(), retPerLayer=True)
    table = fresh.layer_table()
    geo = M.geometry(97, 131)
    assert list(table["stages"]) == list(M.STAGES) and table["pairs"] == 2
    for s in M.STAGES:
        t = table["stages"][s]
        assert tuple(t["out"].shape) == (4,) + geo[s] and t["out"].dtype == torch.float32 and t["launch"] == M.STAGE_LAUNCH[s]
    for k, t in enumerate(table["taps"]):
        hw = geo[t["stage"]][0] * geo[t["stage"]][1]
        assert (t["hw"], t["nblk"]) == (hw, L.dist_blocks(hw)[0]) and tuple(t["part"].shape) == (2, t["nblk"])
    b = fresh(in0.cuda(), in1.cuda(), retPerLayer=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[0], model(in0.cuda(), in1.cuda()))
    again = fresh.layer_table()
    assert all(torch.equal(table["stages"][s]["out"], again["stages"][s]["out"]) for s in M.STAGES)
    tgt, prd = (torch.from_numpy(x).cuda() for x in R.make_frames())
    fresh.frames(tgt, prd, 0, chunk=2)
    with pytest.raises(DsxError, match="holds no whole forward"):
        fresh.layer_table()
    fresh(in0[:1].cuda(), in1[:1].cuda())
    assert fresh.layer_table()["pairs"] == 1


def test_reach():
    """the cases together met every condition of REACH at a checked launch (runs after the cases; skipped when only
    some of them ran, e.g. with -k)"""
    if set(CASES) - set(_CHECKED):
        pytest.skip(f"needs every case of this module checked in this session; missing: {sorted(set(CASES) - set(_CHECKED))}")
    print("\n" + "\n".join(f"{c}: {sorted(t)}" for c, t in _CHECKED.items()))
    missing = REACH - set().union(*_CHECKED.values())
    assert not missing, f"never reached: {sorted(missing)}"
