"""Float64 references of single UNet layers, with error bounds derived from operand rounding alone.

Each check recomputes ONE launch from the tensors that launch actually read (the executor's layer table,
`UNetEngine.layer_table`), so errors do not accumulate across layers and the tolerance can be written down from
first principles.  Everything here is float64 torch on whatever device the tensors live on; nothing calls the
project's kernels.  CPU-importable: tests/test_layer_ref_cpu.py checks the checker itself.

Notation: T is the operand / storage type of the build, u_T its unit roundoff (2^-24 fp32, 2^-8 bf16, 2^-11 fp16),
ulp_T(x) the spacing of T at |x|, u32 = 2^-24.

Conv layer (`check_conv`): out = conv(a', w') + bias + film + resid with
    a  = GroupNorm -> Swish of cat(x0, x1) in fp64 (or the identity).  Where the layer carries gn_scale / gn_shift,
         the kernel's own fp32 scale / shift are used (the statistics are checked by `check_gn_stats`); where
         k_conv_img normalises inside the kernel, GroupNorm is recomputed in fp64 (eps 1e-5).
    a' = round_T(a) (round to nearest even, as pack_bf16x2 / Unit::pack); fp32 operands are not rounded
    w' = round_T(w) as f2bf / f2h pack the weights; fp32 weights exact
    (k_conv_naive, the cross-check kernel, keeps fp32 weights and an fp32 activation in every build: T = fp32 for its
    operands, the output is still stored in the build's type)
Per-element bound |y - r| <= e_out + e_acc + e_flip + e_gn:
    e_out  = ulp_Tout(|r|)                      the output store rounds once (half an ulp; a whole ulp of |r| also
                                                covers the accumulator sitting on the other side of a binade)
    e_acc  = C_ACC sqrt(K) u32 S,  S = conv(|a'|, |w'|) + |bias| + |film| + |resid|
                                                fp32 accumulation of K = ks^2 Cin products and the epilogue adds: each
                                                rounding is <= u32 S, independent signs -> sqrt(K) at C_ACC = 4 sigma
    e_flip = C_FLIP u_T sqrt(conv(a'^2, w'^2))  only where the activation is recomputed here: the kernel's fp32
                                                activation may round to the neighbouring T value (one ulp <= 2 u_T |a|)
                                                or, in fp32, differ by a few ulps (<= 4: the scale/shift FMA, expf,
                                                the reciprocal, the product); random signs at 4 sigma
    e_gn   = conv(1.1 eps_gn |gamma| (|xhat| + |mu|/sigma), |w'|)
                                                k_conv_img only: its fp32-partial statistics (see check_gn_stats)
                                                perturb rstd and mean; Swish' <= 1.1
Aggregates (catch small systematic errors that hide under e_out):
    rms(y - r) <= 2 sqrt(mean(var_i)),  var_i = (ulp_Tout(r_i)^2 + e_acc_i^2 / C_ACC^2 + e_flip_i^2 / C_FLIP^2) / 3
    |mean(y - r)| <= 6 sqrt(sum var_i) / n + MEAN_FLOOR sum|r| / n
    |slope| = |sum (y - r) r| / sum r^2 <= 6 sqrt(sum var_i r_i^2) / sum r^2 + SLOPE_FLOOR
                                                a scale error (weights truncated instead of rounded: slope ~ -0.75 u_T)
The floors (16 u32) leave room for directed rounding inside the hardware accumulators; they are 2^-12 of a bf16
ulp-level scale error.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
C_ACC = 4.0
C_FLIP = {torch.float32: 32.0, torch.bfloat16: 8.0, torch.float16: 8.0}   # fp32: 4 ulps of 2 u each, 4 sigma
MEAN_FLOOR = SLOPE_FLOOR = 16 * U32
GN_TILE_PIXELS = 256     # most pixels one fp32 GroupNorm partial row sums (the largest fused-statistics tile)


def unit(dtype):
    return {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def ulp(x, dtype):
    """spacing of `dtype` at |x| (x float64), subnormals included"""
    _, e = torch.frexp(x.abs())
    e = e.to(torch.float64)
    emin = {torch.float32: -125, torch.bfloat16: -125, torch.float16: -13}[dtype]
    return unit(dtype) * torch.exp2(torch.clamp(e, min=emin))


def round_to(x, dtype):
    """float64 -> fp32 -> dtype (round to nearest even at each step, as the kernels convert fp32) -> float64"""
    return x.to(torch.float32).to(dtype).to(torch.float64)


def _nchw(t):
    return t.permute(0, 3, 1, 2).to(torch.float64)


def conv64(a, w, ks, stride=1, up=False):
    """float64 conv2d (N, C, H, W) x (Co, C, ks, ks) with padding ks // 2, optional nearest x2 upsample in front, as
    unfold + matmul.  Returns (N, Co, Ho, Wo)."""
    if up:
        a = a.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
    N, _, H, W = a.shape
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    cols = F.unfold(a, ks, padding=ks // 2, stride=stride)
    return (w.reshape(w.shape[0], -1).to(a) @ cols).reshape(N, w.shape[0], Ho, Wo)


def group_norm64(x, groups, gamma, beta, eps=1e-5):
    """fp64 GroupNorm of x (N, C, H, W); also returns |xhat| and |mu| / sigma broadcast per element"""
    N, C, H, W = x.shape
    g = x.reshape(N, groups, -1)
    mu = g.mean(-1, keepdim=True)
    var = g.var(-1, unbiased=False, keepdim=True)
    xh = ((g - mu) / torch.sqrt(var + eps)).reshape(N, C, H, W)
    rel = (mu.abs() / torch.sqrt(var + eps)).expand_as(g).reshape(N, C, H, W)
    return xh * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1), xh, rel


def swish(t):
    return t * torch.sigmoid(t)


class Verdict:
    """worst element (index, value, reference, bound), the worst ratio |y - r| / bound and the aggregate failures"""

    def __init__(self, y, r, bound, var, where=""):
        d = (y - r).abs()
        ratio = d / bound
        i = int(torch.argmax(ratio))
        self.ratio = float(ratio.reshape(-1)[i])
        self.index = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), tuple(y.shape)))
        self.value, self.ref, self.bound = float(y.reshape(-1)[i]), float(r.reshape(-1)[i]), float(bound.reshape(-1)[i])
        self.where = where
        n = y.numel()
        e = (y - r).reshape(-1)
        rr = r.reshape(-1)
        v = var.reshape(-1)
        self.aggregate = []
        rms, rms_b = float(torch.sqrt((e * e).mean())), 2.0 * float(torch.sqrt(v.mean()))
        if rms > rms_b:
            self.aggregate.append(f"rms(y - r) = {rms:.3e} > {rms_b:.3e}")
        mean, mean_b = float(e.mean()), 6.0 * float(torch.sqrt(v.sum())) / n + MEAN_FLOOR * float(rr.abs().sum()) / n
        if abs(mean) > mean_b:
            self.aggregate.append(f"|mean(y - r)| = {abs(mean):.3e} > {mean_b:.3e}")
        r2 = float((rr * rr).sum())
        if r2 > 0:
            slope = float((e * rr).sum()) / r2
            slope_b = 6.0 * float(torch.sqrt((v * rr * rr).sum())) / r2 + SLOPE_FLOOR
            if abs(slope) > slope_b:
                self.aggregate.append(f"scale error (y - r) ~ {slope:.3e} r, bound {slope_b:.3e}")

    @property
    def ok(self):
        return self.ratio <= 1.0 and not self.aggregate

    def message(self):
        return (f"{self.where}: worst element {self.index}: value {self.value:.6e}, reference {self.ref:.6e}, "
                f"|diff| {abs(self.value - self.ref):.3e} > bound {self.bound:.3e} (ratio {self.ratio:.2f})"
                + ("; " + "; ".join(self.aggregate) if self.aggregate else ""))


def conv_reference(layer, w, bias, gamma, beta, groups, op_dtype, images=None):
    """(r, bound, var) for a conv layer of the table (NCHW float64, images `images` of the batch).  `w`, `bias`,
    `gamma`, `beta`: the fp32 parameters as the state dict holds them (bias None where it is folded into the film
    vector or absent); `op_dtype`: the operand type T of the build."""
    idx = slice(None) if images is None else list(images)
    x = _nchw(layer["x0"][idx])
    if layer.get("x1") is not None:
        x = torch.cat([x, _nchw(layer["x1"][idx])], dim=1)
    N, Cin = x.shape[:2]
    ks, u = layer["ks"], unit(op_dtype)
    recomputed = gamma is not None or layer["swish"]
    d_gn = None
    if gamma is not None and layer.get("gn_scale") is not None:
        sc = layer["gn_scale"][idx].to(torch.float64).view(N, Cin, 1, 1)
        sh = layer["gn_shift"][idx].to(torch.float64).view(N, Cin, 1, 1)
        t = x * sc + sh
    elif gamma is not None:
        t, xh, rel = group_norm64(x, groups, gamma.to(x), beta.to(x))
        eps_gn = gn_stat_eps(op_dtype, rel)
        d_gn = 1.1 * eps_gn * gamma.to(x).abs().view(1, Cin, 1, 1) * (xh.abs() + rel)
    else:
        t = x
    a = swish(t) if layer["swish"] else t
    a1 = round_to(a, op_dtype) if op_dtype != torch.float32 else a
    w1 = round_to(w.to(torch.float64), op_dtype) if op_dtype != torch.float32 else w.to(torch.float64)
    w1 = w1.to(x.device)
    r = conv64(a1, w1, ks, layer["stride"], layer["up"])
    S = conv64(a1.abs(), w1.abs(), ks, layer["stride"], layer["up"])
    Ho, Wo = r.shape[-2:]
    if bias is not None:
        b = bias.to(x).view(1, -1, 1, 1)
        r, S = r + b, S + b.abs()
    if layer.get("film") is not None:
        f = layer["film"][idx].to(torch.float64).view(N, -1, 1, 1)
        r, S = r + f, S + f.abs()
    if layer.get("resid") is not None:
        q = _nchw(layer["resid"][idx])
        r, S = r + q, S + q.abs()
    K = ks * ks * Cin + 3
    e_acc = C_ACC * math.sqrt(K) * U32 * S
    out_dt = layer["out"].dtype
    e_out = ulp(r, out_dt)
    bound = e_out + e_acc
    var = (e_out * e_out + (e_acc / C_ACC) ** 2) / 3.0
    if recomputed:
        cf = C_FLIP[op_dtype]
        e_flip = cf * u * torch.sqrt(conv64(a1 * a1, w1 * w1, ks, layer["stride"], layer["up"]))
        bound = bound + e_flip
        var = var + (e_flip / cf) ** 2 / 3.0
    if d_gn is not None:
        bound = bound + conv64(d_gn, w1.abs(), ks, layer["stride"], layer["up"])
    return r, bound, var


def check_conv(layer, w, bias, gamma, beta, groups, op_dtype, images=None, where=""):
    r, bound, var = conv_reference(layer, w, bias, gamma, beta, groups, op_dtype, images)
    idx = slice(None) if images is None else list(images)
    y = _nchw(layer["out"][idx])
    return Verdict(y, r, bound, var, where)


def gn_stat_eps(op_dtype, rel):
    """Relative error bound of rstd (and of mu, in units of sigma) that a cancellation-free statistics path delivers.
    The fused paths sum the UNROUNDED fp32 outputs: the stored tensor differs by <= u_T |x| per element, which moves
    the variance by <= 2 u_T sigma rms(x) + u_T^2 rms(x)^2, i.e. rstd by u_T (1 + |mu|/sigma) + u_T^2 (1 + (mu/sigma)^2)
    / 2.  fp32 partial sums over <= GN_TILE_PIXELS pixels (rounding <= u32 per add, 4 sigma): 4 sqrt(n) u32 (1 + |mu|/
    sigma) -- linear in |mu|/sigma, as shifted sums or Chan's formula give; the raw E[x^2] - E[x]^2 form would be
    quadratic.  Finalize in fp32: 4 u32."""
    u = unit(op_dtype) if op_dtype != torch.float32 else 0.0
    return (u * (1 + rel) + 0.5 * u * u * (1 + rel * rel) + 4 * math.sqrt(GN_TILE_PIXELS) * U32 * (1 + rel) + 4 * U32)


def check_gn_stats(layer, gamma, beta, groups, op_dtype, where="", eps=1e-5):
    """gn_scale / gn_shift [B][C] against gamma rstd and beta - mu gamma rstd in fp64 over the STORED sources.
    Bounds: |d scale| <= eps_gn |gamma| rstd + u32 |scale|;
            |d shift| <= eps_gn |gamma| rstd (|mu| + sigma) + u32 (|beta| + 2 |mu scale|)."""
    x = _nchw(layer["x0"])
    if layer.get("x1") is not None:
        x = torch.cat([x, _nchw(layer["x1"])], dim=1)
    N, C = x.shape[:2]
    g = x.reshape(N, groups, -1)
    mu = g.mean(-1)
    var = g.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    cpg = C // groups
    mu_c = mu.repeat_interleave(cpg, dim=1)
    rstd_c = rstd.repeat_interleave(cpg, dim=1)
    sig_c = torch.sqrt(var + eps).repeat_interleave(cpg, dim=1)
    ga, be = gamma.to(x).view(1, C), beta.to(x).view(1, C)
    scale = ga * rstd_c
    shift = be - mu_c * scale
    e = gn_stat_eps(op_dtype, mu_c.abs() / sig_c)
    b_scale = e * ga.abs() * rstd_c + U32 * scale.abs()
    b_shift = e * ga.abs() * rstd_c * (mu_c.abs() + sig_c) + U32 * (be.abs() + 2 * (mu_c * scale).abs())
    ks = layer["gn_scale"].to(torch.float64)
    kh = layer["gn_shift"].to(torch.float64)
    v1 = Verdict(ks, scale, b_scale, torch.zeros_like(scale), where + " gn_scale")
    v2 = Verdict(kh, shift, b_shift, torch.zeros_like(shift), where + " gn_shift")
    v1.aggregate = v2.aggregate = []          # element bounds only: the statistics have no rounding-noise model
    return v1, v2, float((mu.abs() / torch.sqrt(var + eps)).max())


def attention_reference(q, k, v, op_dtype):
    """softmax(q k^T / sqrt(C)) v in fp64 from the stored q / k / v (B, L, C).  Bound (per element):
        ulp_Tout(|r|) + 2 u_T sum_j p_j |v_j|      P is rounded to T before P V (<= u_T p_j each; the normaliser
                                                   differs by the same relative amount)
        + 4 sqrt(C) u32 sum_j p_j (|q||k_j| / sqrt(C)) (|v_j| + |r|)   fp32 score error, through exp
        + 4 sqrt(L) u32 sum_j p_j |v_j|            fp32 accumulation of P V"""
    q, k, v = (t.to(torch.float64) for t in (q, k, v))
    L, C = q.shape[-2:]
    s = q @ k.transpose(-1, -2) / math.sqrt(C)
    p = torch.softmax(s, dim=-1)
    r = p @ v
    pv = p @ v.abs()
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) / math.sqrt(C)
    e_s = 4 * math.sqrt(C) * U32 * ((p * sabs) @ v.abs() + (p * sabs).sum(-1, keepdim=True) * r.abs())
    u = unit(op_dtype)
    core = 2 * u * pv + e_s + 4 * math.sqrt(L) * U32 * pv
    return r, core, pv


def check_attention(layer, op_dtype, images=None, where="", agg_rows=None, known_store=False):
    """The element bound holds for every query row.  The aggregate bounds of Verdict shrink as 1 / sqrt(n) because
    they take the n errors for independent.  Where the query rows of an image are bit-identical copies of each other
    (q = 0: every row is the mean of v), the output rows and their rounding errors are copies too: there are only
    B * C independent errors, each repeated L times, and a slope or mean that is pure rounding noise at n = B * C
    stands sqrt(L) above the bound at n = B * L * C.  For such an input the caller names the distinct rows in
    `agg_rows` and the aggregates are taken over those rows only -- the same bounds at the true n; every row still
    passes the element check.

    The aggregates also take the store's rounding error for a random-sign variable that does not know r.  It does
    where one key m holds nearly all of a row's weight: r = v_m + eps with v_m a value of T and |eps| < ulp / 2, so
    the store returns v_m and its error is -eps = w (v_m - the weighted mean of the other keys), w their weight: a
    slope of +w, in every row of the image alike when the scores are rank 1 (all queries prefer the same key).  This
    is a property of the exact result, not of the kernel -- the term is e0 = round_T(r) - r and is known here.  With
    eta the kernel's internal error (what the aggregates are after), y = round_T(r + eta) and y - round_T(r) is 0 or
    +-ulp, with mean eta over the position of r + eta in its cell and variance <= ulp |eta| <= ulp^2 / 4 < var_i;
    where r sits on a value of T it is 0 and says nothing about eta (the check gets weaker there, never wrong).  For
    such an input (`known_store`) the aggregates are taken of y - round_T(r) instead of y - r, against the same
    bounds.  Measured: slope of y - r 4.3e-4 against a bound of 2.7e-4 (bf16, ramp pattern, L = 33, C = 200), of
    which e0 alone is 4.2e-4 and y - round_T(r) 1e-5, kernel and emulation alike."""
    idx = slice(None) if images is None else list(images)
    r, core, _ = attention_reference(layer["q"][idx], layer["k"][idx], layer["v"][idx], op_dtype)
    y = layer["out"][idx].to(torch.float64)
    e_out = ulp(r, layer["out"].dtype)
    var = (e_out * e_out + (core / 4) ** 2) / 3.0
    bound = e_out + core
    verdict = Verdict(y, r, bound, var, where)
    if agg_rows is not None or known_store:
        rows = slice(None) if agg_rows is None else list(agg_rows)
        ya = y - (round_to(r, layer["out"].dtype) - r) if known_store else y
        verdict.aggregate = Verdict(ya[:, rows], r[:, rows], bound[:, rows], var[:, rows], where).aggregate
    return verdict
