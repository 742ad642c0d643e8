"""Float64 references of single LPIPS launches (dsx_lpips.hip), with bounds derived from fp32 rounding alone.

Each check recomputes ONE launch from the tensor that launch actually read (`LPIPS.layer_table()`: the workspace keeps
every stage of the last forward), the rule tests/layer_ref.py follows for the UNet: errors do not accumulate across
launches, so a single wrong pixel stands against the rounding of one launch and not under a spatial mean.  Everything
here is torch on the CPU; nothing calls the project's kernels.  tests/test_lpips_layers_cpu.py checks the checker.

u = U32 = 2^-24 (layer_ref), gamma(k) = k u / (1 - k u): k roundings, each (1 + delta)^(+-1) with |delta| <= u, compose
to a relative error <= gamma(k) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).

input  k_lpips_input_nchw: out = (x - shift) / scale, two IEEE fp32 operations (__fsub_rn, __fdiv_rn) -> bit-equal to the
       same two operations in torch-CPU float32.
conv   k_lpips_conv1 / k_lpips_conv<5|3>: y = relu(conv(x, w) + b).  With r = conv64(x, w) + b and S = conv64(|x|, |w|) +
       |b| the bound is layer_ref's for an fp32 conv, |y - relu(r)| <= ulp32(r) + C_ACC sqrt(K) u S, K = ks^2 Cin + 1 (the
       products' fp32 accumulation and the bias add; C_ACC and U32 are layer_ref's).  ReLU is 1-Lipschitz:
       |relu(a) - relu(b)| <= |a - b|, so it does not enlarge the bound.  The aggregates of layer_ref.Verdict (rms, mean,
       slope) run over the same variances as for the UNet's fp32 convs.
pool   k_lpips_pool: a maximum rounds nothing -> equal to max_pool2d(3, 2) of the device's own input.
dist   k_lpips_dist<NC>, C = 64 NC channels, one pixel at a time; a, c the two images' feature vectors, w = lin:
         s0 = sum a_j^2      per lane a chain of NC fmaf, then 6 butterfly adds: every term is >= 0, so the relative
                             error is <= gamma(NC + 6)                                      ("two fused sums of squares")
         n0 = sqrtf(s0) + e  sqrt halves the relative error of its argument (k_s = ceil((NC + 6) / 2)) and rounds:
                             HIP documents sqrtf at 1 ulp = 2 u -> 2 roundings; the add of e = fp32(1e-10) rounds once
                             and both summands are >= 0: k_n = k_s + 3.  (s0 = 0 gives n0 = e exactly: the reference
                             uses the fp32 value of 1e-10.)
         q0_j = a_j / n0     __fdiv_rn, one rounding: |dq0_j| <= gamma(k_n + 1) |q0_j|             ("two divisions")
         d_j = q0_j - q1_j   __fsub_rn: |dd_j| <= e_d := gamma(k_n + 1) (|q0_j| + |q1_j|) (1 + u) + u |d_j|
         t_j = w_j (d_j d_j) two roundings: |dt_j| <= |w_j| ((2 |d_j| e_d + e_d^2) (1 + gamma(2)) + gamma(2) d_j^2)
                                                                                     ("the square and the weight product")
       plus 4 x 2^-149 (1 + |w_j|) per element for results below the normal range, where a rounding is absolute.  t_j is
       converted to double exactly and added in double: lanes, waves and pixels of a workgroup in a fixed order, at most
       ppb NC + 9 adds deep, each <= 2^-53 relative of a sum of |t_j| -- gamma64(ppb NC + 9) sum |t_j| per row.  A
       partial row holds the pixels [i ppb, min(HW, (i + 1) ppb)), ppb = ceil(HW / nblk), nblk = min(1024, ceil(HW /
       64)); rows past the last pixel are zero.  Every row is checked against the float64 sum of its pixels; the rows'
       sum against the pair's float64 value follows (the bounds add).  Nothing in the bound is fitted.
finish k_lpips_finish: tap value = fp32((row_0 + row_1 + ...) / hw) in double: <= u |v| + gamma64(nblk + 1) sum |row_i| /
       hw; the total is the fp32 of the double sum of the five: <= u |total| + the taps' double terms.
"""
import math

import torch
import torch.nn.functional as F

from tests.layer_ref import C_ACC, U32, Verdict, ulp
from tests.lpips_ref import SCALE, SHIFT, TRUNK

U64 = 2.0 ** -53
EPS32 = float(torch.tensor(1e-10, dtype=torch.float32))
# launch -> (input stage, output stage, index into TRUNK, stride, padding)
CONVS = {"conv1": ("x0", "f1", 0, 4, 2), "conv2": ("p1", "f2", 1, 1, 2), "conv3": ("p2", "f3", 2, 1, 1),
         "conv4": ("f3", "f4", 3, 1, 1), "conv5": ("f4", "f5", 4, 1, 1)}
POOLS = {"pool1": ("f1", "p1"), "pool2": ("f2", "p2")}
LAUNCHES = ("input", "conv1", "dist1", "pool1", "conv2", "dist2", "pool2", "conv3", "dist3", "conv4", "dist4", "conv5",
            "dist5", "finish")
BIG_LAUNCHES = ("input", "conv1", "dist1", "pool1", "finish")


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def conv1_out(n):
    return (n - 7) // 4 + 1


def pool_out(n):
    return (n - 3) // 2 + 1


def dist_blocks(hw):
    """(nblk, ppb) of launch_lpips_dist, restated"""
    nblk = min(1024, max(1, (hw + 63) // 64))
    return nblk, (hw + nblk - 1) // nblk


class Exact:
    """The Verdict of a launch that rounds nothing: every element equal, or the first that is not."""

    def __init__(self, y, r, where="", bits=False):
        assert y.shape == r.shape, (where, tuple(y.shape), tuple(r.shape))
        bad = (y.view(torch.int32) != r.view(torch.int32)) if bits else ~((y == r) | (y.isnan() & r.isnan()))
        self.count = int(bad.sum())
        self.ratio = float("inf") if self.count else 0.0
        self.where, self.aggregate = where, []
        self.index = self.value = self.ref = None
        if self.count:
            i = int(torch.nonzero(bad.reshape(-1))[0])
            self.index = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(y.shape)))
            self.value, self.ref = float(y.reshape(-1)[i]), float(r.reshape(-1)[i])

    @property
    def ok(self):
        return self.count == 0

    def message(self):
        if self.ok:
            return f"{self.where}: equal"
        return (f"{self.where}: {self.count} elements differ, the first at {self.index}: value {self.value!r}, "
                f"reference {self.ref!r}")


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ input
def input_fp32(in0, in1):
    """(x - shift) / scale, one fp32 operation at a time, (2B, H, W, 3)"""
    x = torch.cat([in0, in1]).detach().cpu().to(torch.float32)
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    d = x - shift
    return (d / scale).permute(0, 2, 3, 1).contiguous()


def check_input(x0, in0, in1, where="k_lpips_input_nchw"):
    """x0 (2B, H, W, 3) NHWC, image, row, column, channel in the index"""
    return Exact(x0.detach().cpu().contiguous(), input_fp32(in0, in1), where, bits=True)


# ------------------------------------------------------------------------------------------------ convs
def conv_reference(x, w, b, stride, pad):
    """x (N, H, W, Cin) fp32 NHWC as the launch read it -> (r, S) float64 NCHW, before the ReLU"""
    x64, w64, b64 = _nchw(x).to(torch.float64), w.to(torch.float64), b.to(torch.float64)
    r = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    return r, S


def check_conv(x, out, w, b, stride, pad, where=""):
    """out (N, Ho, Wo, Cout) fp32 NHWC.  The Verdict's index is (image, channel, row, column)."""
    r, S = conv_reference(x, w, b, stride, pad)
    y = _nchw(out).to(torch.float64)
    assert y.shape == r.shape, (where, tuple(y.shape), tuple(r.shape))
    K = w.shape[1] * w.shape[2] * w.shape[3] + 1
    e_out = ulp(r, torch.float32)
    e_acc = C_ACC * math.sqrt(K) * U32 * S
    var = (e_out * e_out + (e_acc / C_ACC) ** 2) / 3.0
    return Verdict(y, torch.relu(r), e_out + e_acc, var, where)


# ------------------------------------------------------------------------------------------------ pools
def check_pool(x, out, where="k_lpips_pool"):
    """index: (image, channel, row, column)"""
    r = F.max_pool2d(_nchw(x).contiguous(), 3, 2)
    return Exact(_nchw(out).contiguous(), r, where)


# ------------------------------------------------------------------------------------------------ distance of one tap
def dist_reference(feat, lin):
    """feat (2B, H, W, C) fp32 NHWC (the device's tap), lin (C,) -> per pixel (v, e, t): the float64 value
    sum_j w_j (q0_j - q1_j)^2, its bound, and sum_j |t_j|; each (B, H W)"""
    f = feat.detach().cpu().to(torch.float64)
    B, C = f.shape[0] // 2, f.shape[-1]
    NC = C // 64
    a, c = f[:B].reshape(B, -1, C), f[B:].reshape(B, -1, C)
    w = lin.detach().cpu().to(torch.float64).reshape(1, 1, C)
    q0 = a / (torch.sqrt((a * a).sum(-1, keepdim=True)) + EPS32)
    q1 = c / (torch.sqrt((c * c).sum(-1, keepdim=True)) + EPS32)
    d = q0 - q1
    k_n = math.ceil((NC + 6) / 2) + 3
    e_d = gamma(k_n + 1) * (q0.abs() + q1.abs()) * (1 + U32) + U32 * d.abs()
    t = w.abs() * d * d
    e_t = w.abs() * ((2 * d.abs() * e_d + e_d * e_d) * (1 + gamma(2)) + gamma(2) * d * d) + 4 * 2.0 ** -149 * (1 + w.abs())
    return (w * d * d).sum(-1), e_t.sum(-1), t.sum(-1)


def dist_rows(v, hw):
    """per-pixel (B, HW) -> per-row (B, nblk) sums of launch_lpips_dist's pixel ranges"""
    nblk, ppb = dist_blocks(hw)
    return F.pad(v, (0, nblk * ppb - hw)).reshape(v.shape[0], nblk, ppb).sum(-1)


def check_dist(feat, lin, part, where=""):
    """part (B, nblk) float64: every partial row against the float64 sum of its pixels.  Index: (pair, row).  Returns
    (Verdict of the rows, Verdict of each pair's sum of rows)."""
    hw, NC = feat.shape[1] * feat.shape[2], feat.shape[3] // 64
    nblk, ppb = dist_blocks(hw)
    y = part.detach().cpu().to(torch.float64)
    assert tuple(y.shape) == (feat.shape[0] // 2, nblk), (where, tuple(y.shape), nblk)
    v, e, t = dist_reference(feat, lin)
    rows, bound = dist_rows(v, hw), dist_rows(e, hw) + gamma(ppb * NC + 9, U64) * dist_rows(t, hw)
    bound = bound + torch.finfo(torch.float64).tiny          # rows past the last pixel: 0 against 0
    v_rows = Verdict(y, rows, bound, torch.zeros_like(rows), where + " partial rows")
    v_sum = Verdict(y.sum(1), rows.sum(1), bound.sum(1) + gamma(nblk, U64) * y.abs().sum(1), torch.zeros(y.shape[0]),
                    where + " sum of the rows")
    v_rows.aggregate = v_sum.aggregate = []                  # element bounds only
    return v_rows, v_sum


# ------------------------------------------------------------------------------------------------ finish
def check_finish(parts, hws, per_tap, total, taps=range(5), where="k_lpips_finish"):
    """parts: the five (B, nblk) float64 partial-row tensors, per_tap (B, 5) and total (B,) fp32 as the forward returned
    them.  The taps named in `taps` are checked, the total only with all five.  Index: (pair, tap)."""
    pt = per_tap.detach().cpu().to(torch.float64).reshape(-1, 5)
    taps = list(taps)
    want, dbl = [], []
    for k in taps:
        p = parts[k].detach().cpu().to(torch.float64)
        want.append(p.sum(1) / hws[k])
        dbl.append(gamma(p.shape[1] + 1, U64) * p.abs().sum(1) / hws[k])
    want, dbl = torch.stack(want, 1), torch.stack(dbl, 1)
    bound = U32 * want.abs() + dbl + 2.0 ** -149
    out = [Verdict(pt[:, taps], want, bound, torch.zeros_like(want), where + " per tap")]
    if len(taps) == 5:
        tot = want.sum(1)
        bt = U32 * tot.abs() + dbl.sum(1) + gamma(5, U64) * want.abs().sum(1) + 2.0 ** -149
        out.append(Verdict(total.detach().cpu().to(torch.float64).reshape(-1), tot, bt, torch.zeros_like(tot),
                           where + " total"))
    for v in out:
        v.aggregate = []
    return out


# ------------------------------------------------------------------------------------------------ a whole table
def check_launch(name, table, sd, in0=None, in1=None, per_tap=None, total=None, taps=range(5)):
    """The verdicts (a list) of launch `name` (one of LAUNCHES) of a layer table (`LPIPS.layer_table()`, or the CPU
    stand-in of the same layout)."""
    st = table["stages"]
    if name == "input":
        return [check_input(st["x0"]["out"], in0, in1, "input " + st["x0"]["launch"])]
    if name in CONVS:
        src, dst, l, stride, pad = CONVS[name]
        k, idx, _ = TRUNK[l]
        return [check_conv(st[src]["out"], st[dst]["out"], sd[f"net.slice{k}.{idx}.weight"], sd[f"net.slice{k}.{idx}.bias"],
                           stride, pad, f"{name} {st[dst]['launch']}")]
    if name in POOLS:
        src, dst = POOLS[name]
        return [check_pool(st[src]["out"], st[dst]["out"], f"{name} {st[dst]['launch']}")]
    if name.startswith("dist"):
        k = int(name[4:]) - 1
        tap = table["taps"][k]
        feat = st[tap["stage"]]["out"]
        hw = feat.shape[1] * feat.shape[2]
        assert (tap["hw"], tap["nblk"]) == (hw, dist_blocks(hw)[0]), (name, tap["hw"], tap["nblk"], hw)
        return list(check_dist(feat, sd[f"lin{k}.model.1.weight"].reshape(-1), tap["part"], f"{name} {tap['launch']}"))
    assert name == "finish", name
    return check_finish([t["part"] for t in table["taps"]], [t["hw"] for t in table["taps"]], per_tap, total, taps)


def check_table(table, sd, in0, in1, per_tap, total, launches=LAUNCHES):
    """Every launch of `launches`: ({launch: worst ratio}, [failure messages]).  With a partial list (BIG_LAUNCHES) the
    finish check covers the taps whose distance launch is in the list."""
    taps = [k for k in range(5) if f"dist{k + 1}" in launches]
    worst, fails = {}, []
    for name in launches:
        for v in check_launch(name, table, sd, in0, in1, per_tap, total, taps):
            worst[name] = max(worst.get(name, 0.0), v.ratio)
            if not v.ok:
                fails.append(v.message())
    return worst, fails


def level_maps(table):
    """conv level -> (H, W) of the map its kernel tiles: conv1's output, conv2's, conv3..5's (absent stages left out)"""
    st = table["stages"]
    return {lvl: tuple(st[s]["out"].shape[1:3]) for lvl, s in (("conv1", "f1"), ("conv2", "f2"), ("conv3", "f3"))
            if s in st}


def reach_tags(maps, taps):
    """The conditions a forward met, from plain shapes: `maps` {level: (H, W)} of the checked conv launches, `taps`
    [(tap number, hw)] of the checked distance launches."""
    tags = set()
    for lvl, (H, W) in maps.items():
        ty, tx = (H + 15) // 16, (W + 15) // 16
        if tx > ty:
            tags.add(f"{lvl} tiles_x>tiles_y")
        if tx < ty:
            tags.add(f"{lvl} tiles_x<tiles_y")
        for n in (H, W):
            if n % 16 == 0:
                tags.add(f"{lvl} 0mod16")
            if n % 16 == 1 and n > 1:
                tags.add(f"{lvl} 1mod16")
        if (H, W) == (1, 1):
            tags.add(f"{lvl} 1x1")
    for k, hw in taps:
        if (hw + 63) // 64 > 1024:
            tags.add(f"dist{k} capped")
    return tags
