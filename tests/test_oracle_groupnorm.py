"""The oracle's GroupNorm at the channel counts and norm_groups of oracle/cases.py GROUP_CASES, in float64: it judges
the end-to-end test of tests/test_gpu_groups.py, so it is held here, on the CPU.

oracle/unet.py normalises with torch.nn.functional.group_norm (eps 1e-5), as the reference's nn.GroupNorm does; the
per-layer checks use tests/layer_ref.py group_norm64.  Both are compared with the definition written out -- two passes
over each (image, group) in float64: the mean, then the mean of the squared deviations -- on random maps and on the flat
map of the flat plans (a level of 8 under 1e-4 randn, |mean| / std = 2530).

Tolerance, in float64 ulps (2^-52) of max|y| + max|gamma| k, k = |mean| / std of the worst group: rounding a group's
mean once, by 2^-53 of itself, already moves every normalised value by 2^-53 k, so on the flat map (max|y| = 0.4,
k = 2530) no two float64 evaluations agree to ulps of the output alone -- F.group_norm and the two-pass form differ by
up to 1.4e4 ulp of max|y| there, which is 1.3 ulp of this scale; on the random maps k < 0.2 and the scale is max|y|.
  F.group_norm (the oracle):        4 ulp; measured <= 1.8 on the random maps, <= 1.4 on the flat ones
  layer_ref.group_norm64:          32 ulp; measured <= 12 (its variance is a sum over up to 32768 elements), <= 0.1"""
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from tests import layer_ref

torch.set_grad_enabled(False)
ULPS_ORACLE, ULPS_LAYER_REF = 4, 32


def _channel_counts(cfg):
    """(C, H) of every GroupNorm input of a UNet: each level's width and its concats with the skips (unet.py)"""
    inner, mults = cfg["inner_channel"], cfg["channel_mults"]
    widths = [inner * m for m in mults]
    out = set()
    for i, w in enumerate(widths):
        out.add(w)
        out.add(2 * w)                                   # a level's own skip
        if i > 0:
            out.add(widths[i - 1])
            out.add(w + widths[i - 1])                   # the skip of the level above
    return sorted(out)


CASES = sorted({(name, C) for name, case in cases.GROUP_CASES.items() for C in _channel_counts(case["cfg"])})


def _two_pass(x, groups, gamma, beta, eps=1e-5):
    N, C, H, W = x.shape
    g = x.reshape(N, groups, -1)
    mu = g.sum(-1, keepdim=True) / g.shape[-1]
    d = g - mu
    var = (d * d).sum(-1, keepdim=True) / g.shape[-1]
    return (d / torch.sqrt(var + eps)).reshape(N, C, H, W) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)


@pytest.mark.parametrize("flat", [False, True], ids=["random", "flat"])
@pytest.mark.parametrize("name,C", CASES)
def test_group_norm_float64(name, C, flat):
    groups = cases.GROUP_CASES[name]["cfg"]["norm_groups"]
    assert C % groups == 0
    g = torch.Generator().manual_seed(1000 * groups + C)
    x = torch.randn((2, C, 8, 8), generator=g, dtype=torch.float64)
    x = 8.0 + 1e-4 * x if flat else 0.7 * x + 0.5 * torch.randn((1, C, 1, 1), generator=g, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    want = _two_pass(x, groups, gamma, beta)
    got = F.group_norm(x, groups, gamma, beta, eps=1e-5)             # what oracle/unet.py calls
    assert got.dtype == torch.float64
    ref, _, rel = layer_ref.group_norm64(x, groups, gamma, beta)     # what the per-layer checks call
    k = float(rel.max())
    ulp = 2.0 ** -52 * (float(want.abs().max()) + float(gamma.abs().max()) * k)
    err, err_ref = float((got - want).abs().max()) / ulp, float((ref - want).abs().max()) / ulp
    print(f"\n{name} C={C} groups={groups}: F.group_norm {err:.2f} ulp, group_norm64 {err_ref:.2f} ulp of "
          f"{ulp * 2.0 ** 52:.3f} (max|y| = {float(want.abs().max()):.3f}, |mean|/std {k:.3g})")
    assert err <= ULPS_ORACLE and err_ref <= ULPS_LAYER_REF, (err, err_ref)
    assert (k > 1e3) == flat
