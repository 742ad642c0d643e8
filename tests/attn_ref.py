"""Hostile inputs for the fused attention kernel (k_attn, csrc/dsx_attn.hip) and a tile-wise emulation of its
arithmetic.  CPU-importable, plain torch: nothing here calls the project's kernels.

Why: with synthetic weights the scores q.k / sqrt(C) of a UNet forward sit near zero and the softmax is almost flat, so
the running-max rescale (alpha ~ 1), the first tile's exp(-inf), the -inf mask of the keys past L and the zero fill of
the padded head dimension barely show in the result.  The patterns below make each of them decide the result; the
reference and the bound are tests/layer_ref.py's (`attention_reference` / `check_attention`), unchanged.

`emulate` restates the kernel's arithmetic (key tiles of 128, fp32 scores, fp32 online softmax, P rounded to the
operand type T for P.V, the normaliser summed from the unrounded p, one reciprocal, one store) with switches for the
mistakes a fused kernel makes.  tests/test_attn_ref_cpu.py shows that the bound accepts the faithful emulation on every
pattern and rejects every switch; tests/test_gpu_attention.py hands the same patterns to the kernel.

Worst |y - r| / bound per type over every pattern x shape; the aggregate checks hold on every one of them, for `unif`
and the two ramps in the form check() below derives:
                                                                        fp32     bf16     fp16
    emulation, the shapes of test_attn_ref_cpu.SHAPES, B = 2 (CPU)      0.110    0.415    0.338
    k_attn on an MI355X, every launch of test_gpu_attention.py          0.176    0.513    0.434
(measured: the first row by test_attn_ref_cpu.py, the second by test_gpu_attention.py, which print them)
"""
import math

import torch

from tests import layer_ref

BK = 128                                       # keys per tile of k_attn
PATTERNS = ("rand", "asc", "desc", "peak", "neg", "unif", "voff")


def _generator(pattern, L, C, device):
    g = torch.Generator(device=device)
    g.manual_seed(1_000_003 * (PATTERNS.index(pattern) + 1) + 1031 * L + C)
    return g


def make_pattern(pattern, L, C, B=1, device="cpu"):
    """(q, k, v) fp32 (B, L, C), seeded from (pattern, L, C); the B images hold different draws.  The caller rounds
    them to the storage type.

    rand  randn with q * 2: a moderately peaked softmax (test_layer_ref_cpu.make_attention)
    asc   scores rise with the key index by ~30 over the L keys (rank 1 along u = +-1): every key tile raises the
          running max, so every tile rescales the accumulator and the running sum
    desc  the same ramp reversed: the max is in the first tile, later tiles only add tails
    peak  one key per query at score 40, at key (37 i + 5) mod L: it lands on every position, tile edges, the ragged
          tail and key L - 1 included
    neg   every score ~ -50: a pad key left at score 0, or a non-zero padded column, would dominate
    unif  q = 0: out is the mean of v over exactly L keys
    voff  v = 100 + randn: the normaliser must match P to well below an output ulp"""
    g = _generator(pattern, L, C, device)
    rn = lambda *shape: torch.randn(shape, generator=g, device=device, dtype=torch.float32)
    q, k, v = rn(B, L, C), rn(B, L, C), rn(B, L, C)
    sign = lambda t: torch.where(t >= 0, 1.0, -1.0).to(torch.float32)
    rc = math.sqrt(C)
    if pattern == "rand":
        q = q * 2.0
    elif pattern in ("asc", "desc"):
        u = sign(rn(B, 1, C))
        j = torch.arange(L, device=device, dtype=torch.float32) / max(L - 1, 1)
        ramp = 30.0 * (j if pattern == "asc" else 1.0 - j)
        q = q + 4.0 * u
        k = k + (ramp / (4.0 * rc)).view(1, L, 1) * u
    elif pattern == "peak":
        k = sign(k)
        t = (37 * torch.arange(L, device=device) + 5) % L
        q = (40.0 / rc) * k[:, t]
    elif pattern == "neg":
        u = sign(rn(B, 1, C))
        c = math.sqrt(50.0 / rc)
        q = c * u + 0.1 * q
        k = -c * u + 0.1 * k
    elif pattern == "unif":
        q = torch.zeros_like(q)
    elif pattern == "voff":
        q = q * 2.0
        v = 100.0 + v
    else:
        raise ValueError(pattern)
    return q, k, v


def trunc_bf16(t32):
    """fp32 -> bf16 by dropping the low 16 bits (the mistake), as fp32"""
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(q, k, v, dtype, unmasked_pads=False, no_oacc_rescale=False, no_l_rescale=False, padded_c_div=False,
            trunc_p=False):
    """k_attn's arithmetic on q, k, v (B, L, C) of type `dtype`, returned in `dtype`.  The switches are the mistakes:
    unmasked_pads    keys past L of the last tile keep their score 0 (they read as zero rows)
    no_oacc_rescale  the output accumulator is not scaled by alpha when the running max rises
    no_l_rescale     the running sum is not
    padded_c_div     the scores are divided by sqrt(C rounded up to 128)
    trunc_p          P is truncated to bf16 instead of rounded (bf16 only)"""
    f32 = dtype == torch.float32
    B, L, C = q.shape
    q32, k32, v32 = (t.to(torch.float32) for t in (q, k, v))
    div = torch.tensor(float((C + 127) // 128 * 128 if padded_c_div else C), dtype=torch.float32).sqrt()
    inv_div = 1.0 / div                                     # fp32, as the planner sets it
    pad = (-L) % BK
    if pad:                                                 # rows past L read as zero through the buffer descriptor
        z = torch.zeros((B, pad, C), dtype=torch.float32, device=q.device)
        k32, v32 = torch.cat([k32, z], dim=1), torch.cat([v32, z], dim=1)
    m = torch.full((B, L, 1), -math.inf, dtype=torch.float32, device=q.device)
    l = torch.zeros((B, L, 1), dtype=torch.float32, device=q.device)
    o = torch.zeros((B, L, C), dtype=torch.float32, device=q.device)
    for key0 in range(0, L, BK):
        kt, vt = k32[:, key0:key0 + BK], v32[:, key0:key0 + BK]
        s = q32 @ kt.transpose(-1, -2)
        s = s / div if f32 else s * inv_div
        if not unmasked_pads and key0 + BK > L:
            s[..., L - key0:] = -math.inf
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp(m - m_new)                        # first tile: exp(-inf) = 0
        p = torch.exp(s - m_new)
        l = (l if no_l_rescale else l * alpha) + p.sum(-1, keepdim=True)
        if not f32:
            p = trunc_bf16(p) if trunc_p else p.to(dtype).to(torch.float32)
        o = (o if no_oacc_rescale else o * alpha) + p @ vt
        m = m_new
    return (o * (1.0 / l)).to(dtype)


def check(q, k, v, out, dtype, where="", pattern=None):
    """layer_ref.check_attention on tensors of type `dtype`: the Verdict (elements and aggregates).  Two patterns
    break an assumption of the aggregate bounds, each as derived in check_attention: `unif` is the one whose query
    rows are copies of each other (q = 0), so its aggregates are taken over one row per image; the ramps `asc` and
    `desc` have rank-1 scores, every query of an image prefers the same key and the result sits within half an ulp of
    that key's v, so their aggregates leave out the reference's own store rounding."""
    agg_rows = [0] if pattern == "unif" else None
    return layer_ref.check_attention(dict(q=q, k=k, v=v, out=out), dtype, where=where, agg_rows=agg_rows,
                                     known_store=pattern in ("asc", "desc"))
