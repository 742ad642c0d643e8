"""The two ways to name the tiles of a launch on the MI355X (`-m gpu`): the plan forms (dsx_tileplan_*: the plan's device
tables, an arithmetic id sequence) and the per-call forms (dsx_tiles_* / dsx_stitch*: a host table and an id list,
uploaded for the call) run the same kernels on the same geometry, so for the same ids they write the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.mark.parametrize("patch,grid", [(32, 16), (30, 10)], ids=["p32_g16", "p30_g10"])
def test_plan_forms_equal_the_per_call_forms(patch, grid):
    """(2, 40, 56) frames: ragged extents, shifted and clipped last tiles; patch 32 has pw % 4 == 0, patch 30 has not and
    starts at x = 10 and 26.  Gather, gather_norm, gather_mix (all three outputs), stitch and stitch + PSNR partial rows
    of the ids 1, 4, 7, ... through both forms."""
    from diffsplitting_amd._lib import check, lib
    from diffsplitting_amd.data.tiling import TilePlan, _i64x3, as_sequence
    shape = (2, 40, 56)
    plan = TilePlan(shape, (1, grid, grid), (1, patch, patch))
    assert plan.total == {32: 12, 30: 16}[patch]
    ids = np.arange(1, plan.total, 3, dtype=np.int64)
    first, stride, count = as_sequence(ids)
    assert (first, stride) == (1, 3) and count == len(ids) >= 4
    assert (plan.patch_start[ids, 2] % 4 != 0).any() == (patch == 30)
    g = torch.Generator().manual_seed(patch)
    f0 = (torch.rand(shape, generator=g) * 4000).cuda()
    f1 = (torch.rand(shape, generator=g) * 3000).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ds, ps = _i64x3(shape), _i64x3((1, patch, patch))
    table = plan.patch_start.ctypes.data_as(C.POINTER(C.c_int64))
    idp = ids.ctypes.data_as(C.POINTER(C.c_int64))
    new = lambda *s, dtype=torch.float32: [torch.full(s, float("nan"), dtype=dtype, device="cuda") for _ in range(2)]

    a, b = new(count, patch, patch)
    check(lib.dsx_tileplan_gather(plan.handle, ptr(f0), first, stride, count, ptr(a), st))
    check(lib.dsx_tiles_gather(ptr(f0), ds, ps, table, idp, count, ptr(b), st))
    assert torch.equal(a, b)
    n, y, x = (int(v) for v in plan.patch_start[ids[-1]])
    assert torch.equal(a[-1], f0[n, y:y + patch, x:x + patch])

    norm6 = (C.c_double * 6)(1246.59, 1211.3, 759.685, 741.25, 486.905, 470.5)
    for from_norm_target in (0, 1):
        ain, bin_ = new(count, 1, patch, patch)
        atar, btar = new(count, 2, patch, patch)
        check(lib.dsx_tileplan_gather_norm(plan.handle, ptr(f0), ptr(f1), first, stride, count, 1.0, 0.3, norm6,
                                           from_norm_target, ptr(ain), ptr(atar), st))
        check(lib.dsx_tiles_gather_norm(ptr(f0), ptr(f1), ds, ps, table, idp, count, 1.0, 0.3, norm6, from_norm_target,
                                        ptr(bin_), ptr(btar), st))
        assert torch.equal(ain, bin_) and torch.equal(atar, btar) and atar.std() > 0.1

    norm4, lohi = (C.c_double * 4)(759.685, 741.25, 486.905, 470.5), (C.c_double * 4)(-2.0, 3.0, -1.5, 2.5)
    am = [new(count, 2, patch, patch) for _ in range(3)]           # target, mix, cls: (plan form, per-call form)
    check(lib.dsx_tileplan_gather_mix(plan.handle, ptr(f0), ptr(f1), first, stride, count, norm4, 0.29, lohi,
                                      ptr(am[0][0]), ptr(am[1][0]), ptr(am[2][0]), st))
    check(lib.dsx_tiles_gather_mix(ptr(f0), ptr(f1), ds, ps, table, idp, count, norm4, 0.29, lohi, ptr(am[0][1]),
                                   ptr(am[1][1]), ptr(am[2][1]), st))
    for plan_out, call_out in am:
        assert torch.equal(plan_out, call_out)
    assert torch.equal(am[0][0], atar) and not torch.equal(am[1][0], am[2][0])

    Cn = 2
    pred = torch.randn((count, Cn, patch, patch), generator=g).cuda()
    gt = torch.randn(shape + (Cn,), generator=g).cuda()
    regions = np.ascontiguousarray(plan.regions[ids])
    rp = regions.ctypes.data_as(C.POINTER(C.c_int32))
    ca, cb = torch.zeros(shape + (Cn,), device="cuda"), torch.zeros(shape + (Cn,), device="cuda")
    check(lib.dsx_tileplan_stitch(plan.handle, ptr(pred), Cn, first, stride, count, ptr(ca), None, None, st))
    check(lib.dsx_stitch(ptr(pred), count, Cn, patch, patch, rp, ptr(cb), ds, st))
    assert torch.equal(ca, cb) and (ca != 0).any() and (ca == 0).any()
    pa, pb = torch.zeros_like(ca), torch.zeros_like(ca)
    ra, rb = new(count, plan.psnr_blocks(), Cn, 8, dtype=torch.float64)
    check(lib.dsx_tileplan_stitch(plan.handle, ptr(pred), Cn, first, stride, count, ptr(pa), ptr(gt), ptr(ra), st))
    check(lib.dsx_stitch_psnr(ptr(pred), count, Cn, patch, patch, rp, ptr(pb), ds, ptr(gt), ptr(rb), st))
    assert torch.equal(pa, ca) and torch.equal(pb, ca) and torch.equal(ra, rb)
    assert (ra[..., 5] <= ra[..., 6]).any()                            # min g <= max g where a workgroup saw pixels
