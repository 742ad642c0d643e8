"""The host-side checks that every tile gather / stitch shares (dsx_tiles.cpp: geom_of_host, geom_of_plan, the count
limit), form by form, without a GPU.  Every call below must be refused on the host: the device pointers are fake
(non-NULL, never dereferenced), so a call that got past the checks would not return INVALID with these messages."""
import ctypes as C

import numpy as np
import pytest

from tests.nets import dbl, i64

ERR_INVALID = -1
N, H, W, P = 2, 40, 56, 32
FAKE = C.c_void_p(4096)


def _lib():
    from diffsplitting_amd import _lib
    return _lib.lib


def _err():
    return _lib().dsx_last_error().decode()


def _table(rows):
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def _ids(ids):
    if ids is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


# ----------------------------------------------------------------------------- the five per-call gathers
def _gather(starts, ids, count):
    return _lib().dsx_tiles_gather(FAKE, i64(N, H, W), i64(1, P, P), starts, ids, count, FAKE, None)


def _gather_norm(starts, ids, count):
    return _lib().dsx_tiles_gather_norm(FAKE, FAKE, i64(N, H, W), i64(1, P, P), starts, ids, count, 1.0, 1.0,
                                        dbl(0, 1, 0, 1, 0, 1), 0, FAKE, FAKE, None)


def _gather_norm_planes(starts, ids, count):
    return _lib().dsx_tiles_gather_norm_planes(FAKE, FAKE, i64(N, 3, H, W), i64(P, P), starts, ids, count, 1.0, 1.0, 0.0,
                                               1.0, dbl(*[0.0] * 6), dbl(*[1.0] * 6), FAKE, FAKE, None)


def _gather_mix(starts, ids, count):
    return _lib().dsx_tiles_gather_mix(FAKE, FAKE, i64(N, H, W), i64(1, P, P), starts, ids, count, dbl(0, 1, 0, 1), 0.5,
                                       None, FAKE, None, None, None)


def _gather_mix_items(starts, ids, count):
    assert ids is None                                                # the per-item form has no id list
    t = np.full(max(int(count), 1), 0.5)
    return _lib().dsx_tiles_gather_mix_items(FAKE, FAKE, i64(N, H, W), i64(1, P, P), starts, count, dbl(0, 1, 0, 1),
                                             t.ctypes.data_as(C.POINTER(C.c_double)), None, FAKE, None, None, None)


GATHERS = [("gather", "tile", _gather), ("gather_norm", "tile", _gather_norm),
           ("gather_norm_planes", "item", _gather_norm_planes), ("gather_mix", "tile", _gather_mix),
           ("gather_mix_items", "item", _gather_mix_items)]
GATHER_IDS = [g[0] for g in GATHERS]
OUTSIDE = [(N, 0, 0), (0, H - P + 1, 0), (0, 0, -1)]                  # what every form refused already
WRAPS = [(0, 0, 2 ** 32 + 5), (0, 2 ** 32 + 3, 0), (2 ** 32 + 1, 0, 0), (0, 0, -2 ** 32)]   # the low 32 bits would fit


@pytest.mark.parametrize("name,label,call", GATHERS, ids=GATHER_IDS)
@pytest.mark.parametrize("bad", OUTSIDE + WRAPS, ids=str)
def test_gather_refuses_a_location_outside_the_frames(name, label, call, bad):
    """checked on the int64 values, before they are narrowed; the refusal names the entry point and the offender"""
    keep, starts = _table([(1, H - P, W - P), bad])                   # the first one is the last valid corner
    assert call(starts, None, 2) == ERR_INVALID
    assert f"{name}: {label} 1 at ({bad[0]}, {bad[1]}, {bad[2]}) lies outside the frames" in _err()
    assert call(starts, None, 0) == 0                                 # nothing to do is not an error, and needs no device


@pytest.mark.parametrize("name,label,call", GATHERS[:4], ids=GATHER_IDS[:4])
def test_gather_refuses_a_negative_tile_id(name, label, call):
    keep, starts = _table([(0, 0, 0), (1, 8, 24)])
    keep_ids, ids = _ids([1, -1])
    assert call(starts, ids, 2) == ERR_INVALID and f"{name}: negative tile id" in _err()
    # an id list picks its rows: row 1 is outside, row 0 is fine
    keep, starts = _table([(0, 0, 0), (0, 9, 0)])
    keep_ids, ids = _ids([0, 0, 1])
    assert call(starts, ids, 3) == ERR_INVALID and "outside the frames" in _err() and "(0, 9, 0)" in _err()


@pytest.mark.parametrize("name,label,call", GATHERS, ids=GATHER_IDS)
def test_gather_refuses_more_items_than_a_launch_takes(name, label, call):
    keep, starts = _table(np.zeros((65536, 3)))
    for count in (65536, -1):
        assert call(starts, None, count) == ERR_INVALID
        assert f"{name}: count = {count}" in _err() and "65535" in _err()


# ----------------------------------------------------------------------------- the two per-call stitches
def _stitch(regions, count):
    return _lib().dsx_stitch(FAKE, count, 1, P, P, regions, FAKE, i64(N, H, W), None)


def _stitch_psnr(regions, count):
    return _lib().dsx_stitch_psnr(FAKE, count, 1, P, P, regions, FAKE, i64(N, H, W), FAKE, FAKE, None)


STITCHES = [("stitch", _stitch), ("stitch_psnr", _stitch_psnr)]


def _regions(rows):
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 8))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.mark.parametrize("name,call", STITCHES, ids=[s[0] for s in STITCHES])
def test_stitch_refusals(name, call):
    good = (1, H - P, W - P, P, P, 0, 0, 0)                           # (frame, y, x, h, w, ry, rx, 0)
    for n, y, x in OUTSIDE:
        keep, regions = _regions([good, (n, y, x, P, P, 0, 0, 0)])
        assert call(regions, 2) == ERR_INVALID and "region 1 out of bounds" in _err()
    keep, regions = _regions([good] * 65536)
    for count in (65536, -1):
        assert call(regions, count) == ERR_INVALID
        assert f"{name}: count = {count}" in _err() and "65535" in _err()
    assert call(regions, 0) == 0


# ----------------------------------------------------------------------------- the plan forms
@pytest.fixture(scope="module")
def plan():
    from diffsplitting_amd.data.tiling import TilePlan
    p = TilePlan((2, 40, 57), (1, 8, 8), (1, 16, 16))                 # the plan of test_input_stack_cpu.py
    assert p.total == 56
    return p


def _plan_forms():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    d4, d6 = dbl(0, 1, 0, 1), dbl(0, 1, 0, 1, 0, 1)
    return [
        ("tileplan_gather", lambda h, f, s, c: lib.dsx_tileplan_gather(h, FAKE, f, s, c, FAKE, None)),
        ("tileplan_gather_norm", lambda h, f, s, c: lib.dsx_tileplan_gather_norm(h, FAKE, FAKE, f, s, c, 1.0, 1.0, d6, 0, FAKE,
                                                                                 FAKE, None)),
        ("tileplan_gather_mix", lambda h, f, s, c: lib.dsx_tileplan_gather_mix(h, FAKE, FAKE, f, s, c, d4, 0.5, None, FAKE, None,
                                                                               None, None)),
        ("gather_input", lambda h, f, s, c: lib.dsx_tileplan_gather_input(h, FAKE, _lib.PIX_U16, f, s, c, 10.0, 2.0, -1.0, FAKE,
                                                                          None)),
        ("tileplan_stitch", lambda h, f, s, c: lib.dsx_tileplan_stitch(h, FAKE, 1, f, s, c, FAKE, None, None, None)),
    ]


@pytest.mark.parametrize("form", range(5), ids=["gather", "gather_norm", "gather_mix", "gather_input", "stitch"])
def test_plan_forms_refuse_a_sequence_that_leaves_the_plan(plan, form):
    name, call = _plan_forms()[form]
    for first, stride, count in ((plan.total, 1, 1), (0, 0, 2), (1, 2 ** 62, 3),          # the last id overflows int64
                                 (-1, 1, 1), (plan.total - 3, 1, 4), (1, 2, 29), (0, -1, 2)):
        assert call(plan.handle, first, stride, count) == ERR_INVALID, (first, stride, count)
        assert f"{name}: tiles {first} + k * {stride} ({count} of them) leave the plan (56 tiles)" in _err()
    for count in (65536, -1):
        assert call(plan.handle, 0, 1, count) == ERR_INVALID and f"{name}: count = {count}" in _err() and "65535" in _err()
    assert call(None, 0, 1, 1) == ERR_INVALID and "null argument" in _err()
    if name != "gather_input":                                        # which asks for at least one tile
        assert call(plan.handle, 0, 1, 0) == 0


def test_pack_refuses_a_sequence_that_leaves_the_plan(plan):
    """dsx_tileplan_pack names its tiles first, first + world, ...: the same check"""
    lib = _lib()
    for first, world, count in ((plan.total, 1, 1), (50, 3, 3), (-1, 2, 1)):
        assert lib.dsx_tileplan_pack(plan.handle, FAKE, 1, world, first, count, FAKE, None) == ERR_INVALID
        assert f"tileplan_pack: tiles {first} + k * {world} ({count} of them) leave the plan (56 tiles)" in _err()
    assert lib.dsx_tileplan_pack(plan.handle, FAKE, 1, 2, 0, 65536, FAKE, None) == ERR_INVALID and "65535" in _err()
    assert lib.dsx_tileplan_pack(plan.handle, FAKE, 1, 2, 0, 0, FAKE, None) == 0
