"""dsx_comoments on the MI355X (`-m gpu`): the 12 numbers of every plane against tests/comoments_ref.py within its derived
bound, read in place from NaN-poisoned strided layouts; the curve and its argmax; the bits of a plane at any position,
in calls of any number of planes, on either load path and run to run."""
import numpy as np
import pytest
import torch

from tests import comoments_ref as CR
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
T_LIST = np.arange(0, 1.0, 0.05)


def _span():
    """pixels per workgroup up to which a plane is one workgroup, read from dsx_comoments_blocks"""
    from diffsplitting_amd._lib import lib
    lo, hi = 1, 1 << 24
    assert lib.dsx_comoments_blocks(lo) == 1 and lib.dsx_comoments_blocks(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.dsx_comoments_blocks(mid) == 1 else (lo, mid)
    assert lib.dsx_comoments_blocks(2 * lo) == 2 and lib.dsx_comoments_blocks(2 * lo + 1) == 3
    return lo


def _poisoned(x, pixel=1, offset=0, gap=3):
    """``x`` (P, n) fp32 on the device as a strided view into a buffer that is NaN wherever the view does not point:
    ``pixel`` elements from pixel to pixel, ``gap`` more than a plane's span from plane to plane (rounded up to a
    multiple of 4 when offset % 4 == 0 and pixel == 1, so that the layout allows 16-byte loads), ``offset`` elements
    into the (256-byte aligned) allocation."""
    P, n = x.shape
    plane = (n - 1) * pixel + 1 + gap
    if pixel == 1 and offset % 4 == 0:
        plane = (plane + 3) // 4 * 4
    buf = torch.full((offset + P * plane + 8,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf.as_strided((P, n), (plane, pixel), offset)
    view.copy_(torch.from_numpy(x))
    assert int(torch.isnan(buf).sum()) == buf.numel() - P * n
    return view


LAYOUTS = {"aligned planes": dict(gap=0), "gaps": dict(), "pixel stride 2": dict(pixel=2), "misaligned base": dict(offset=1),
           "pixel stride 2, odd base": dict(pixel=2, offset=3, gap=0)}


def _device(g, p1, p2, **layout):
    from diffsplitting_amd.core.psnr import comoments
    m = comoments(*[_poisoned(np.ascontiguousarray(x.reshape(x.shape[0], -1)), **layout) for x in (g, p1, p2)])
    assert m.dtype == torch.float64 and m.is_cuda and m.shape == (g.shape[0], 12)
    return m


def _check(g, p1, p2, what, planted=False):
    """every layout against the restatement: moments, curve, t*, argmax; -> the bits every layout agreed on"""
    from diffsplitting_amd.core.psnr import range_invariant_psnr_curve
    ref, bnd = CR.moments(g, p1, p2, with_bounds=True)
    c_ref, t_ref = CR.curve(ref, T_LIST, 1 - T_LIST)
    c_bnd, t_bnd = CR.curve_bound(ref, bnd, T_LIST, 1 - T_LIST), CR.t_star_bound(ref, bnd)
    first = None
    for name, layout in LAYOUTS.items():
        dev = _device(g, p1, p2, **layout)
        m = dev.cpu().numpy()
        err = np.abs(m - ref)
        assert np.array_equal(m[:, :3], ref[:, :3]), (what, name)                 # n, min, max: exact
        assert (err <= bnd).all(), (what, name, CR.NAMES[int((err - bnd).max(axis=0).argmax())], err.max(), bnd.max())
        c, t = (v.cpu().numpy() for v in range_invariant_psnr_curve(dev, T_LIST, 1 - T_LIST))
        assert (np.isnan(c) == np.isnan(c_ref)).all() and (np.isnan(t) == np.isnan(t_ref)).all(), (what, name)
        ok = np.isfinite(c_bnd)
        with np.errstate(invalid="ignore"):                                       # inf - inf where the bound is inf
            c_err = np.where(ok, np.abs(c - c_ref), 0.0)
        assert (c_err[ok] <= c_bnd[ok]).all(), (what, name)
        okt = np.isfinite(t_bnd) & ~np.isnan(t_ref)
        assert (np.abs(t - t_ref)[okt] <= t_bnd[okt]).all(), (what, name)
        if planted and g.shape[1] > 2:
            assert np.isfinite(c_bnd).all() and (c.argmax(axis=1) == c_ref.argmax(axis=1)).all(), (what, name)
        if first is None:
            first = m
            worst = np.nanmax(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0))
            print(f"{what}: max moment err / bound {worst:.3f}; max curve err "
                  f"{np.nanmax(c_err):.3e} dB, bound {np.nanmax(np.where(ok, c_bnd, 0)):.3e} dB")
        else:                                                                  # either load path, any layout: same bits
            assert np.array_equal(m.view(np.uint64), first.view(np.uint64)), (what, name)
    from diffsplitting_amd.core.psnr import comoments
    plain = comoments(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (g, p1, p2)]).cpu().numpy()
    assert np.array_equal(plain.view(np.uint64), first.view(np.uint64)), (what, "contiguous")
    return first


@pytest.mark.parametrize("n", [1, 2, 63, 64, 257, 1023, 1024])
def test_small_planes_against_the_restatement(n):
    g, p1, p2 = CR.planted((3, n), seed=n)
    _check(g, p1, p2, f"n = {n}", planted=True)


@pytest.mark.parametrize("which", ["span - 1", "span", "span + 1", "2 span - 1", "2 span", "2 span + 1"])
def test_one_and_two_workgroups_worth(which):
    s = _span()
    n = {"span - 1": s - 1, "span": s, "span + 1": s + 1, "2 span - 1": 2 * s - 1, "2 span": 2 * s, "2 span + 1": 2 * s + 1}[which]
    g, p1, p2 = CR.planted((3, n), seed=7)
    _check(g, p1, p2, f"n = {n} ({which})", planted=True)


@pytest.mark.parametrize("planes", [1, 5])
def test_other_plane_counts(planes):
    g, p1, p2 = CR.planted((planes, 33, 130), seed=0)                  # the shape of the closed-form check, n % 4 != 0 ...
    _check(g, p1, p2, f"{planes} planes of 33 x 130", planted=True)
    g, p1, p2 = CR.planted((planes, 64, 64), seed=0)                   # ... and one that takes 16-byte loads
    _check(g, p1, p2, f"{planes} planes of 64 x 64", planted=True)


@pytest.mark.parametrize("n", [1023, 1020])
def test_hostile_inputs(n):
    """Raw-count-like planes, an outlying first pixel, p1 == p2, a constant g, anti-correlated estimates."""
    from diffsplitting_amd.core.psnr import range_invariant_psnr_curve
    for name, (g, p1, p2) in CR.hostile(n).items():
        m = _check(g, p1, p2, f"{name}, n = {n}")
        c, t = range_invariant_psnr_curve(torch.from_numpy(m).cuda(), T_LIST, 1 - T_LIST)
        if name == "constant":
            assert (m[:, 1] == m[:, 2]).all() and bool(torch.isnan(c).all())
        if name == "equal":
            assert bool(torch.isnan(t).all()) and bool(torch.isfinite(c).all())
    # what the contract forbids does leave the bound here: the check above can fail
    g, p1, p2 = CR.hostile(n)["counts"]
    ref, bnd = CR.moments(g, p1, p2, with_bounds=True)
    assert (np.abs(CR.moments_raw_fp32(g, p1, p2) - ref)[:, 6:] > bnd[:, 6:]).any()


def test_a_planes_bits_do_not_depend_on_the_call():
    from diffsplitting_amd.core.psnr import comoments
    s = _span()
    for n in (257, 2 * s + 4):
        g, p1, p2 = (np.ascontiguousarray(x) for x in CR.planted((5, n), seed=3))
        for x in (g, p1, p2):
            x[4] = x[0]                                                # the same plane first and last
        dg, d1, d2 = (torch.from_numpy(x).cuda() for x in (g, p1, p2))
        five = comoments(dg, d1, d2)
        again = comoments(dg, d1, d2)
        assert same_bits(five, again)                   # two runs
        assert same_bits(five[0], five[4])              # first and last
        for k in range(5):                                            # alone (a view into the stack, and a copy of its own)
            assert same_bits(comoments(dg[k:k + 1], d1[k:k + 1], d2[k:k + 1])[0], five[k]), (n, k)
        alone = comoments(dg[2:3].clone(), d1[2:3].clone(), d2[2:3].clone())
        assert same_bits(alone[0], five[2])
        three = comoments(dg[1:4], d1[1:4], d2[1:4])
        assert same_bits(three, five[1:4])


def test_views_are_read_in_place():
    """One channel of a (b, 2, p, p) tensor, a (b, 1, p, p) tensor and one channel of a channel-last canvas."""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core.psnr import comoments
    g, p1, p2 = CR.planted((4, 24, 40), seed=2)
    ref, bnd = CR.moments(g, p1, p2, with_bounds=True)
    est = torch.from_numpy(np.stack([p1, p2], axis=1)).cuda()                       # (4, 2, 24, 40)
    canvas = torch.from_numpy(np.stack([g, p2], axis=-1)).cuda()                    # (4, 24, 40, 2) channel-last
    tile = torch.from_numpy(p1[:, None]).cuda()                                     # (4, 1, 24, 40)
    m = comoments(canvas[..., 0], tile, est[:, 1]).cpu().numpy()
    assert (np.abs(m - ref) <= bnd).all()
    assert np.array_equal(m, comoments(canvas[..., 0], est[:, 0:1], canvas[..., 1]).cpu().numpy())
    with pytest.raises(DsxError, match="no stack of planes"):
        comoments(canvas[:, ::2, :, 0], tile[:, :, ::2], tile[:, :, ::2])          # every other row: two pixel strides
    with pytest.raises(DsxError, match="equally many"):
        comoments(canvas[..., 0], tile[:3], est[:, 1])
    with pytest.raises(DsxError, match="float32"):
        comoments(canvas[..., 0].double(), tile, est[:, 1])
    assert comoments(canvas[:0, ..., 0], tile[:0], est[:0, 1]).shape == (0, 12)
