"""tests/attn_ref.py checked on the CPU: layer_ref's attention bound accepts the tile-wise emulation of k_attn on
every hostile pattern, in every type, and rejects each mistake of a fused kernel on the pattern and shape where it
must show; dsx_attention refuses bad arguments with a status before any device work (no GPU needed)."""
import pytest
import torch

from tests import attn_ref

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(1, 8), (33, 72), (129, 136), (240, 64), (300, 264), (257, 520), (1024, 128)]       # (L, C)


def _case(pattern, L, C, dt, B=2):
    return tuple(t.to(DT[dt]) for t in attn_ref.make_pattern(pattern, L, C, B))


def _verdict(pattern, L, C, dt, **mutation):
    q, k, v = _case(pattern, L, C, dt)
    out = attn_ref.emulate(q, k, v, DT[dt], **mutation)
    return attn_ref.check(q, k, v, out, DT[dt], where=f"{pattern} L={L} C={C} {dt} {mutation or ''}", pattern=pattern)


@pytest.mark.parametrize("dt", list(DT))
def test_bound_accepts_the_emulation_on_every_pattern(dt):
    worst, fails = (0.0, ""), []
    for L, C in SHAPES:
        for pattern in attn_ref.PATTERNS:
            v = _verdict(pattern, L, C, dt)
            if v.ratio > worst[0]:
                worst = (v.ratio, v.where)
            if not v.ok:
                fails.append(v.message())
    print(f"\nemulation {dt}: worst error/bound {worst[0]:.3f} at {worst[1]}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("L,C", [(33, 72), (129, 136)])
@pytest.mark.parametrize("pattern", ["neg", "unif"])
def test_rejects_unmasked_pad_keys(pattern, L, C, dt):
    v = _verdict(pattern, L, C, dt, unmasked_pads=True)
    assert v.ratio > 1.0, v.message()


# `peak` puts the heavy key of query i at (37 i + 5) mod L: at L = 129 query 87 has it at key 128, the only key of the
# second tile, so one query must show the missing rescale.  The ramp of `asc` carries score noise of ~4 (q = randn + 4u
# against k's randn part): a second tile of one key, 0.23 up the ramp, rarely holds a row's maximum, so `asc` starts at
# L = 160, where the second tile's 32 keys are the top of the ramp.
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("pattern,L,C", [("peak", 129, 136), ("asc", 160, 136), ("peak", 300, 264), ("asc", 300, 264),
                                         ("peak", 1024, 128), ("asc", 1024, 128)])
@pytest.mark.parametrize("which", ["no_oacc_rescale", "no_l_rescale"])
def test_rejects_a_missing_rescale(which, pattern, L, C, dt):
    v = _verdict(pattern, L, C, dt, **{which: True})
    assert v.ratio > 1.0, v.message()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("L,C", [(33, 72), (129, 136)])
def test_rejects_division_by_the_padded_head_dimension(L, C, dt):
    v = _verdict("rand", L, C, dt, padded_c_div=True)
    assert v.ratio > 1.0, v.message()


@pytest.mark.parametrize("L,C", [(129, 136), (300, 264)])
def test_rejects_p_truncated_to_bf16_through_the_aggregates(L, C):
    v = _verdict("rand", L, C, "bf16", trunc_p=True)
    assert not v.ok and v.aggregate, v.message()


def test_one_key_softmax_needs_the_known_store_term():
    """Key 7 holds all but ~1e-3 of every row's weight: the exact fp64 result, rounded once -- the best any kernel can
    store -- has a slope above the plain aggregate bound, all of it the store's own rounding towards v_7 (see
    check_attention).  With that term taken out the same result passes."""
    from tests import layer_ref
    g = torch.Generator().manual_seed(3)
    B, L, C, dt = 3, 33, 64, torch.bfloat16
    k = torch.where(torch.randn((B, L, C), generator=g) >= 0, 1.0, -1.0)
    v = torch.randn((B, L, C), generator=g)
    q = (10.0 / C ** 0.5) * k[:, 7:8] + 0.3 * torch.randn((B, L, C), generator=g)
    q, k, v = (t.to(dt) for t in (q, k, v))
    r, _, _ = layer_ref.attention_reference(q, k, v, dt)
    layer = dict(q=q, k=k, v=v, out=layer_ref.round_to(r, dt).to(dt))
    plain = layer_ref.check_attention(layer, dt)
    assert plain.ratio <= 1.0 and any("scale error" in a for a in plain.aggregate), plain.message()
    known = layer_ref.check_attention(layer, dt, known_store=True)
    assert known.ok, known.message()


# ----------------------------------------------------------------------------- dsx_attention: refusals
def test_attention_wrapper_refuses_cpu_tensors():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    with pytest.raises(DsxError, match="CUDA tensor"):
        engine.attention(torch.zeros((4, 24)), 0, 8, 16, 1, 4, 8, torch.zeros((4, 8)))


def test_attention_refuses_bad_arguments_with_a_status():
    """Argument checks come before any device work: they run without a GPU and nothing throws."""
    from diffsplitting_amd._lib import lib
    buf, bf16 = 4096, 1                                        # a 16-byte-aligned address that is never dereferenced
    good = dict(qkv=buf, ld=3 * 64, q_col=0, k_col=64, v_col=128, out=buf, ldo=64, storage=bf16, B=2, L=40, C=64,
                col_split=0)

    def refused(needle, **change):
        a = dict(good, **change)
        rc = lib.dsx_attention(a["qkv"], a["ld"], a["q_col"], a["k_col"], a["v_col"], a["out"], a["ldo"], a["storage"],
                               a["B"], a["L"], a["C"], a["col_split"], None)
        msg = lib.dsx_last_error().decode()
        assert rc == -1 and msg.startswith("attention:") and needle in msg, (change, rc, msg)

    refused("null", qkv=None)
    refused("null", out=None)
    refused("not supported", C=4)                              # attn_supported: 8..1024, a multiple of 8, L >= 1
    refused("not supported", C=1032, ld=3 * 1032, k_col=1032, v_col=2064, ldo=1032)
    refused("not supported", C=60, ld=192)
    refused("not supported", L=0)
    refused("B =", B=0)
    refused("storage", storage=3)
    refused("storage", storage=-1)
    refused("offsets", q_col=-8, ld=200)
    refused("offsets", k_col=68, ld=200)                       # 16-bit unit: 8 elements
    refused("offsets", v_col=130, storage=0, ld=200)           # fp32 unit: 4 elements
    refused("do not fit", ld=184)                              # v_col + C > ld
    refused("do not fit", k_col=136, v_col=64, ld=192)         # k_col + C > ld
    refused("do not fit", q_col=136, k_col=136, v_col=136, ld=192)
    refused("before q", q_col=64, k_col=0)
    refused("before q", q_col=64, k_col=128, v_col=0)
    refused("ld =", ld=196)                                    # not a multiple of the unit
    refused("ldo", ldo=66)
    refused("ldo", ldo=56)                                     # < C
    refused("aligned", qkv=buf + 8)
    refused("aligned", out=buf + 4)
    # L * ld * ES >= 2^31 with a padded row, where attn_supported's ld = 3C estimate still passes
    L = (1 << 31) // ((3 * 64 + 64) * 4)
    assert L * 3 * 64 * 4 < (1 << 31)                          # ... i.e. this case is the new check's alone
    refused("descriptor", L=L, ld=3 * 64 + 64, storage=0)
    refused("descriptor", L=L + 5, ld=3 * 64 + 64, storage=0)
