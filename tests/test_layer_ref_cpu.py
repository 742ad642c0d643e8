"""The per-layer checker of tests/test_gpu_layers.py, checked on the CPU: it must accept a kernel-like result (fp32
accumulation, fp32 activation rounded to the operand type) and reject each of the small, localised mistakes a conv or
attention kernel makes.  The simulated kernel below rounds with its own bit-level code (pack_conv's f2bf), not with
layer_ref's, so a wrong rounding in the reference makes the acceptance tests fail."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import layer_ref

DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def f2bf_np(x):
    """fp32 -> bf16 round to nearest even, bit-level (pack_conv's f2bf), returned as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def trunc_bf_np(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def op_round(t32, dt, trunc=False):
    """fp32 torch tensor -> operand type (simulated kernel), as fp32"""
    if dt == "f32":
        return t32
    f = trunc_bf_np if trunc else f2bf_np
    return torch.from_numpy(f(t32.numpy()).reshape(t32.shape))


def make_layer(dt, cin, seed, B=2, H=8, W=8, cout=32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, cin), generator=g) * 1.5 + 0.3
    x = torch.from_numpy(f2bf_np(x.numpy()).reshape(x.shape)) if dt == "bf16" else x
    w = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
    bias = 0.1 * torch.randn((cout,), generator=g)
    film = 0.2 * torch.randn((B, cout), generator=g)
    sc = (0.5 + torch.rand((B, cin), generator=g)).float()
    sh = (0.3 * torch.randn((B, cin), generator=g)).float()
    layer = dict(ks=3, stride=1, up=False, swish=True, x0=x.to(DT[dt]), x1=None, gn_scale=sc, gn_shift=sh,
                 film=film, resid=None)
    return layer, w, bias


def simulate(layer, w, bias, dt, trunc_w=False, a_hook=None, y_hook=None, pad_mode="zeros"):
    """what the kernel computes: fp32 activation, operands rounded to T, fp32 accumulation, fp32 epilogue, one store"""
    x = layer["x0"].float().permute(0, 3, 1, 2)
    t = x * layer["gn_scale"][:, :, None, None] + layer["gn_shift"][:, :, None, None]
    a = op_round(t * torch.sigmoid(t), dt)
    if a_hook:
        a = a_hook(a)
    wr = op_round(w.float(), dt, trunc_w)
    if pad_mode == "zeros":
        y = F.conv2d(a, wr, padding=1)
    else:
        y = F.conv2d(F.pad(a, (1, 1, 1, 1), mode=pad_mode), wr)
    y = y + bias[None, :, None, None] + layer["film"][:, :, None, None]
    if y_hook:
        y = y_hook(y, a, wr)
    out = dict(layer)
    out["out"] = y.permute(0, 2, 3, 1).contiguous().to(DT[dt])
    return out


def verdict(layer, w, bias, dt):
    return layer_ref.check_conv(layer, w, bias, torch.ones(1), None, 1, DT[dt], where="synthetic")


CASES = [(dt, cin) for dt in ("bf16", "f32") for cin in (64, 1024)]


@pytest.mark.parametrize("dt,cin", CASES)
def test_accepts_kernel_like_result(dt, cin):
    layer, w, bias = make_layer(dt, cin, seed=cin)
    v = verdict(simulate(layer, w, bias, dt), w, bias, dt)
    assert v.ok, v.message()
    # the bound is tight: the real error uses a visible part of it
    assert v.ratio > (0.1 if dt == "bf16" else 0.002), v.ratio


@pytest.mark.parametrize("dt,cin", CASES)
def test_rejects_one_dropped_tap(dt, cin):
    layer, w, bias = make_layer(dt, cin, seed=1 + cin)

    def drop(y, a, wr):                    # output pixel (1, 4, 5) misses tap (0, 0), i.e. input pixel (3, 4)
        y = y.clone()
        y[1, :, 4, 5] -= wr[:, :, 0, 0] @ a[1, :, 3, 4]
        return y
    v = verdict(simulate(layer, w, bias, dt, y_hook=drop), w, bias, dt)
    assert not v.ok and v.index[0] == 1 and v.index[2:] == (4, 5), v.message()


@pytest.mark.parametrize("dt,cin", CASES)
def test_rejects_channels_swapped_inside_a_16_byte_unit(dt, cin):
    layer, w, bias = make_layer(dt, cin, seed=2 + cin)
    unit = 8 if dt == "bf16" else 4
    c = unit * 3 + 1                        # channels c, c + 1 of one unit

    def swap(a):
        a = a.clone()
        a[:, [c, c + 1]] = a[:, [c + 1, c]]
        return a
    v = verdict(simulate(layer, w, bias, dt, a_hook=swap), w, bias, dt)
    assert not v.ok, v.message()


@pytest.mark.parametrize("dt,cin", CASES)
def test_rejects_halo_tap_from_the_neighbouring_pixel(dt, cin):
    layer, w, bias = make_layer(dt, cin, seed=3 + cin)
    good = simulate(layer, w, bias, dt)
    bad = simulate(layer, w, bias, dt, pad_mode="replicate")    # the zero padding read as the edge pixel
    out = good["out"].clone()
    out[0, 0, 3] = bad["out"][0, 0, 3]                          # at one border pixel only
    good["out"] = out
    v = verdict(good, w, bias, dt)
    assert not v.ok and v.index[0] == 0 and v.index[2:] == (0, 3), v.message()


@pytest.mark.parametrize("dt,cin", CASES)
def test_rejects_film_from_the_wrong_channel(dt, cin):
    layer, w, bias = make_layer(dt, cin, seed=4 + cin)
    wrong = dict(layer)
    f = layer["film"].clone()
    f[:, 5] = layer["film"][:, 6]
    wrong["film"] = f
    sim = simulate(wrong, w, bias, dt)
    sim["film"] = layer["film"]                  # the checker knows the right vector
    v = verdict(sim, w, bias, dt)
    assert not v.ok and v.index[1] == 5, v.message()


@pytest.mark.parametrize("cin", [64, 1024])
def test_rejects_weights_truncated_to_bf16(cin):
    layer, w, bias = make_layer("bf16", cin, seed=5 + cin)
    v = verdict(simulate(layer, w, bias, "bf16", trunc_w=True), w, bias, "bf16")
    assert not v.ok and v.aggregate, v.message()


# ------------------------------------------------------------------------------------------------ attention
def make_attention(dt, seed, B=2, L=96, C=64):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, L, C), generator=g) for _ in range(3))
    q = q * 2.0                                   # a peaked softmax, as after GroupNorm with learnt scales
    if dt == "bf16":
        q, k, v = (torch.from_numpy(f2bf_np(t.numpy()).reshape(t.shape)) for t in (q, k, v))
    return q, k, v


def simulate_attention(q, k, v, dt, drop=None):
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if drop is not None:
        b, row, key = drop
        s[b, row, key] = -float("inf")
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = (op_round(p, dt) @ v) / l
    return o.to(DT[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_attention_accepts_and_rejects_a_dropped_key(dt):
    q, k, v = make_attention(dt, seed=11)
    layer = dict(q=q.to(DT[dt]), k=k.to(DT[dt]), v=v.to(DT[dt]), out=simulate_attention(q, k, v, dt))
    ok = layer_ref.check_attention(layer, DT[dt], where="attn")
    assert ok.ok, ok.message()
    s = q[1, 17] @ k[1].T
    key = int(torch.argmax(s))                    # the row's heaviest key is lost
    layer["out"] = simulate_attention(q, k, v, dt, drop=(1, 17, key))
    bad = layer_ref.check_attention(layer, DT[dt], where="attn")
    assert not bad.ok and bad.index[:2] == (1, 17), bad.message()


def test_gn_stats_checker_accepts_exact_and_rejects_a_missing_tile():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 16, 16, 32), generator=g) * 0.7 + 2.0
    gamma, beta = 1 + 0.1 * torch.randn(32, generator=g), 0.1 * torch.randn(32, generator=g)
    groups = 8

    def stats(xs):
        xx = xs.permute(0, 3, 1, 2).double().reshape(2, groups, -1)
        mu, var = xx.mean(-1), xx.var(-1, unbiased=False)
        r = 1 / torch.sqrt(var + 1e-5)
        sc = gamma.double() * r.repeat_interleave(4, 1)
        return sc.float(), (beta.double() - mu.repeat_interleave(4, 1) * sc).float()
    sc, sh = stats(x)
    layer = dict(x0=x, x1=None, gn_scale=sc, gn_shift=sh)
    v1, v2, _ = layer_ref.check_gn_stats(layer, gamma, beta, groups, torch.float32)
    assert v1.ok and v2.ok, (v1.message(), v2.message())
    sc2, sh2 = stats(x[:, :, 4:])                 # one 16 x 4 strip of pixels left out of the sums
    layer.update(gn_scale=sc2, gn_shift=sh2)
    v1, v2, _ = layer_ref.check_gn_stats(layer, gamma, beta, groups, torch.float32)
    assert not (v1.ok and v2.ok)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gn_stats_checker_at_192_channels_per_group_over_a_concat(dt):
    """tests/test_gpu_groups.py: 256 + 128 channels in two groups of 192 -- group 0 ends inside source 0, group 1 takes
    its last 64 channels and source 1.  A kernel-like result (fp32 partial rows of 64 pixels per channel, summed in
    double as gn_finalize_item does, scale and shift in fp32) passes; a scale / shift that is right in the first 64
    channels of each group and wrong behind them -- what a finalize that loses the channels past its first wave leaves --
    fails, whether those channels were never written, their scale is off by 1e-4 (f32) / 1e-2 (bf16: the bound carries
    u_T = 2^-8) of itself, or their shift by 1e-4 / 2e-2."""
    g = torch.Generator().manual_seed(192)
    B, H, W, C0, C1, groups = 2, 16, 16, 256, 128, 2
    C, cpg = C0 + C1, (C0 + C1) // groups
    x = torch.randn((B, H, W, C), generator=g) * 0.7 + 1.5 * torch.randn((1, 1, 1, C), generator=g)
    x = op_round(x, dt)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rows = x.reshape(B, H * W // 64, 64, C)                                  # one partial row per 64 pixels
    s = rows.sum(2, dtype=torch.float32).double().sum(1)                     # [B][C]
    q = (rows * rows).sum(2, dtype=torch.float32).double().sum(1)
    n = float(H * W * cpg)
    mean = s.reshape(B, groups, cpg).sum(-1) / n
    var = (q.reshape(B, groups, cpg).sum(-1) / n - mean * mean).clamp(min=0)
    rstd = (1.0 / torch.sqrt(var + 1e-5)).float().repeat_interleave(cpg, 1)
    sc = rstd * gamma
    sh = beta - mean.float().repeat_interleave(cpg, 1) * sc
    layer = dict(x0=x[..., :C0].to(DT[dt]), x1=x[..., C0:].to(DT[dt]), gn_scale=sc, gn_shift=sh)
    v1, v2, _ = layer_ref.check_gn_stats(layer, gamma, beta, groups, DT[dt])
    assert v1.ok and v2.ok, (v1.message(), v2.message())
    behind = (torch.arange(C) % cpg) >= 64                                   # channels 64 .. 191 of each group
    for bad_sc, bad_sh in ((torch.where(behind, torch.zeros(()), sc), torch.where(behind, torch.zeros(()), sh)),
                           (torch.where(behind, sc * (1 + (1e-4 if dt == "f32" else 1e-2)), sc), sh),
                           (sc, torch.where(behind, sh + (1e-4 if dt == "f32" else 2e-2), sh))):
        layer.update(gn_scale=bad_sc, gn_shift=bad_sh)
        v1, v2, _ = layer_ref.check_gn_stats(layer, gamma, beta, groups, DT[dt])
        assert not (v1.ok and v2.ok)
        for v in (v1, v2):
            if not v.ok:
                assert v.index[1] % cpg >= 64, v.message()                  # and it names a channel behind the 64th
    # the same corruption in the first 64 channels only is seen there: the check is per channel
    layer.update(gn_scale=torch.where(behind, sc, torch.zeros(())), gn_shift=sh)
    v1, _, _ = layer_ref.check_gn_stats(layer, gamma, beta, groups, DT[dt])
    assert not v1.ok and v1.index[1] % cpg < 64


def test_reach_tags_of_the_widths_module():
    """tests/test_gpu_widths.py derives its reach conditions from plain layer-table fields (layer_check.reach_tags):
    hand-made entries, one per condition, and their nearest neighbours that must not count"""
    from tests.layer_check import reach_tags

    def conv(desc, ks=3, C0=32, C1=0, Cout=32, stride=1, up=0, resid=False, film=False, gn=False):
        return dict(kind=0, desc=desc, ks=ks, stride=stride, up=up, C0=C0, C1=C1, Cout=Cout, resid=resid, film=film,
                    gn_scale=gn, gn_in_kernel=0)
    t64 = "conv3x3 1->1 @8x8 tile64x64"
    # the scalar epilogue: Cout off 16, on an MFMA-family launch only
    assert reach_tags(conv(t64, C0=24, Cout=24, resid=True, film=True), "f32", 8) == {"scalar+resid", "scalar+film",
                                                                                       "scalar nbase>0"}
    assert reach_tags(conv(t64, Cout=12, film=True), "f32", 8) == {"scalar+film"}
    assert reach_tags(conv(t64, Cout=48, resid=True, film=True), "f32", 8) == set()
    assert reach_tags(conv("conv3x3 6->24 @8x8 first", C0=6, Cout=24, film=True), "f32", 8) == set()
    # stage mode 2: a source off the 16-byte unit (8 channels in 16 bits, 4 in fp32)
    L = conv("conv1x1s2 1->1 @8x8 tile64x64", ks=1, C0=20, C1=40, Cout=32, stride=2, gn=True)
    assert reach_tags(L, "bf16", 5) == {"stage2+gn", "stage2+cat", "stage2 1x1", "stage2 s2", "cpg5+"}
    assert reach_tags(L, "f32", 5) == {"cpg5+"}
    assert reach_tags(conv("conv3x3up 60->60 @8x8 tile64x64", C0=60, up=1), "f16", 5) == {"stage2 up"}
    assert reach_tags(conv("conv3x3up 80->80 @8x8 tile64x64", C0=80, up=1), "f16", 5) == set()
    # split counts, K tails of the persistent kernel, N tails of the wide tiles
    assert reach_tags(conv(t64 + " splitK6"), "bf16", 8) == {"splitK odd"}
    assert reach_tags(conv(t64 + " splitK4"), "bf16", 8) == set()
    assert reach_tags(conv(t64 + " ws", C0=96), "bf16", 8) == set()          # 3 x 3: 32-channel groups
    assert reach_tags(conv(t64 + " ws c2", C0=96), "bf16", 8) == {"ws ktail"}
    assert reach_tags(conv("conv1x1 1->1 @8x8 tile64x64 ws +gn", ks=1, C0=96), "bf16", 8) == {"ws ktail"}
    assert reach_tags(conv("conv1x1 1->1 @8x8 tile64x64 ws +gn", ks=1, C0=96), "f32", 8) == set()
    assert reach_tags(conv("conv3x3 1->1 @8x8 tile64x128", Cout=96), "bf16", 8) == {"wide ntail"}
    assert reach_tags(conv("conv3x3 1->1 @8x8 tile128x128", Cout=256), "bf16", 8) == set()
    assert reach_tags(conv("conv3x3 1->1 @8x8 tile256x64", Cout=96), "bf16", 8) == set()
    # channels per GroupNorm group, attention head dimensions
    assert reach_tags(conv(t64, C0=48, gn=True), "f32", 16) == {"cpg3"}
    assert reach_tags(conv(t64, C0=64, gn=True), "f32", 8) == set()                # 8 per group: a power of two
    assert reach_tags(conv(t64, C0=48), "f32", 16) == set()                        # no GroupNorm in front
    assert reach_tags(dict(kind=1, C0=72, desc="attn fused L=64 d=72"), "bf16", 8) == {"attn"}
    assert reach_tags(dict(kind=1, C0=64, desc="attn fused L=64 d=64"), "bf16", 8) == set()
    assert reach_tags(dict(kind=3, C0=0, desc=""), "bf16", 8) == set()


def test_geom_tags_of_the_shapes_module():
    """tests/test_gpu_shapes.py names the tile geometry of every MFMA-family launch from plain layer-table fields
    (layer_check.geom_tag): hand-made entries against tiles worked out by hand from the planner's rule (TW: largest power
    of two <= 16 dividing Wo; TH: largest <= BM / TW dividing Ho; TB = BM / (TW TH))"""
    from tests.layer_check import geom_tag

    def conv(desc, Ho, Wo, B=3, ks=3, stride=1, up=0):
        return dict(kind=0, desc=desc, ks=ks, stride=stride, up=up, Ho=Ho, Wo=Wo, B=B)
    # the maps every other GPU module runs: 8 x 8 pixels and wider
    assert geom_tag(conv("conv3x3 64->64 @32x32 tile64x64", 32, 32)) == "mfma 3x3 16x4x1@64"
    assert geom_tag(conv("conv3x3 64->64 @8x8 tile64x64", 8, 8)) == "mfma 3x3 8x8x1@64"
    assert geom_tag(conv("conv3x3 64->64 @8x12 tile64x64", 8, 12)) == "mfma 3x3 4x8x2@64+tail"
    assert geom_tag(conv("conv3x3 64->64 @4x4 tile64x64", 4, 4, B=4)) == "mfma 3x3 4x4x4@64"
    # narrow maps: 12, 6, 4 and 2 pixels wide, and 6 high
    assert geom_tag(conv("conv3x3 16->16 @64x12 tile64x64 ws", 64, 12)) == "ws 3x3 4x16x1@64"
    assert geom_tag(conv("conv1x1 32->32 @64x12 tile64x64 ws +gn", 64, 12, ks=1)) == "ws 1x1 4x16x1@64"
    assert geom_tag(conv("conv3x3up 32->32 @64x12 tile64x64 ws c2", 64, 12, up=1)) == "ws 3x3 up 4x16x1@64"
    assert geom_tag(conv("conv1x1 64->64 @32x6 tile64x64 ws", 32, 6, ks=1)) == "ws 1x1 2x32x1@64"
    assert geom_tag(conv("conv3x3 64->64 @16x6 tile64x64", 16, 6)) == "mfma 3x3 2x16x2@64+tail"
    assert geom_tag(conv("conv3x3 64->64 @16x6 tile64x64", 16, 6, B=2)) == "mfma 3x3 2x16x2@64"
    assert geom_tag(conv("conv3x3 64->64 @16x6 tile64x64", 16, 6, B=1)) == "mfma 3x3 2x16x2@64+tail"
    assert geom_tag(conv("conv3x3 64->64 @6x16 tile64x64 splitK3", 6, 16)) == "splitK 3x3 16x2x2@64+tail"
    assert geom_tag(conv("conv3x3s2 32->32 @12x8 tile64x64", 12, 8, stride=2)) == "mfma 3x3 s2 8x4x2@64+tail"
    assert geom_tag(conv("conv3x3s2 32->32 @12x8 tile64x64 splitK2", 12, 8, stride=2)) == "splitK 3x3 s2 8x4x2@64+tail"
    # the same map on a 128-pixel tile takes twice the rows, or twice the images once the rows are used up
    assert geom_tag(conv("conv3x3 16->16 @64x12 tile128x32", 64, 12)) == "mfma 3x3 4x32x1@128"
    assert geom_tag(conv("conv3x3 16->16 @64x12 tile128x32 g2", 64, 12)) == "g2 3x3 4x32x1@128"
    assert geom_tag(conv("conv1x1 64->64 @16x6 tile128x128", 16, 6, ks=1)) == "mfma 1x1 2x16x4@128+tail"
    assert geom_tag(conv("conv1x1 64->64 @16x6 tile128x128", 16, 6, ks=1, B=4)) == "mfma 1x1 2x16x4@128"
    assert geom_tag(conv("conv3x3 64->64 @64x24 tile128x64 ws c2", 64, 24)) == "ws 3x3 8x16x1@128"
    assert geom_tag(conv("conv3x3 16->3 @64x48 tile256x32 g2", 64, 48)) == "g2 3x3 16x16x1@256"
    # launches outside the MFMA families, and layers that are no convs
    assert geom_tag(conv("conv3x3 6->32 @64x48 first", 64, 48)) is None
    assert geom_tag(conv("conv3x3 512->512 @8x8 img", 8, 8)) is None
    assert geom_tag(conv("conv3x3-naive 16->16 @64x12", 64, 12)) is None
    assert geom_tag(dict(kind=1, desc="attn fused L=64 d=64")) is None
    assert geom_tag(dict(kind=3, desc="")) is None
