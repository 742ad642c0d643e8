"""k_attn launched directly (engine.attention -> dsx_attention) on the MI355X (`-m gpu`): every instantiation
k_attn<ST, NDB, CS> of csrc/dsx_attn.hip, ragged L and C, and the hostile softmax inputs of tests/attn_ref.py, each
launch against layer_ref's fp64 reference and bound (elements and aggregates) computed from q / k / v as stored.

Every launch reads a poisoned layout: ld = 3C + 32 with 8 NaN columns before q and between and after the three
ranges, 32 NaN guard rows after the last image, different data per image; `out` has ldo = C + 8 and 32 guard rows
prefilled with a sentinel bit pattern that must come back unchanged.  A read outside an image's rows or a range's
columns turns the result into NaN; a store outside out[:, :C] breaks the sentinel."""
import pytest
import torch

from tests import attn_ref
from tests.bits import same_bits
from tests.nets import dev  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ST = {"f32": 0, "bf16": 1, "f16": 2}
ST_OF = {DT[d]: s for d, s in ST.items()}
SENTINEL = {2: (torch.int16, 0x7FA5), 4: (torch.int32, 0x7FA5A5A5)}     # by element size; a NaN in every type
PAD, GUARD = 8, 32

# head dimension -> the (NDB, CS) it must reach; the 4-chunk sizes run with col_split 0 and 1
C_TABLE = {(1, 1): (8, 64, 72, 128), (2, 1): (136, 200, 256), (4, 1): (264, 384, 392, 512), (4, 2): (264, 384, 392, 512),
           (8, 1): (520, 640, 1024)}
L_ALL = (1, 31, 32, 33, 127, 128, 129, 240, 257, 300)
L_FEW = (1, 33, 129, 300)                  # every C is crossed with these, ...
C_EVERY_L = (72, 200, 392, 520)            # ... these C with every L
GRID = [(C, cs - 1, (ndb, cs)) for (ndb, cs), cols in C_TABLE.items() for C in cols]      # (C, col_split, (NDB, CS))

_LAUNCHED = set()                          # (ST, NDB, CS)
_WORST = {}                                # dtype -> (ratio, where)
_RAN = set()                               # test ids of the grid


def instantiation(C, B, L, col_split):
    """(NDB, CS) by the dispatch rule of launch_attn_st: 128-channel chunks rounded up to 1, 2, 4 or 8; four chunks
    split their output channels over two workgroups when asked to and B * ceil(L / 32) <= 160"""
    ndb = (C + 127) // 128
    ndb = {1: 1, 2: 2, 3: 4, 4: 4}.get(ndb, 8)
    cs = 2 if (ndb == 4 and col_split and B * ((L + 31) // 32) <= 160) else 1
    return ndb, cs


def _launch(q, k, v, col_split, padded=True):
    """One launch on q, k, v (B, L, C) of the storage type: out (B, L, C).  padded: the poisoned layout (sentinels
    asserted); else the planner's (q first, ld = 3C, ldo = C)."""
    from diffsplitting_amd import engine
    B, L, C = q.shape
    rows, dt, dev = B * L, q.dtype, q.device
    pad, guard = (PAD, GUARD) if padded else (0, 0)
    ld, ldo = 3 * C + 4 * pad, C + pad
    cols = [pad, 2 * pad + C, 3 * pad + 2 * C]
    qkv = torch.full((rows + guard, ld), float("nan"), dtype=dt, device=dev)
    for c0, t in zip(cols, (q, k, v)):
        qkv[:rows, c0:c0 + C] = t.reshape(rows, C)
    it, word = SENTINEL[q.element_size()]
    out = torch.full((rows + guard, ldo), word, dtype=it, device=dev).view(dt)
    engine.attention(qkv, cols[0], cols[1], cols[2], B, L, C, out, col_split=bool(col_split))
    _LAUNCHED.add((ST_OF[dt],) + instantiation(C, B, L, col_split))
    ob = out.view(it)
    assert bool((ob[:rows, C:] == word).all()), f"out columns >= C written (B={B} L={L} C={C} {dt})"
    assert bool((ob[rows:] == word).all()), f"out guard rows written (B={B} L={L} C={C} {dt})"
    return out[:rows, :C].reshape(B, L, C)


def _run(pattern, B, L, C, dt, col_split, note):
    dev = torch.device("cuda:0")
    q, k, v = (t.to(DT[dt]) for t in attn_ref.make_pattern(pattern, L, C, B, device=dev))
    out = _launch(q, k, v, col_split)
    where = f"{pattern} B={B} L={L} C={C} {dt} col_split={col_split} <{ST[dt]},%d,%d>" % instantiation(C, B, L, col_split)
    assert bool(torch.isfinite(out).all()), f"{where}: non-finite output (a poisoned column or row was read)"
    note(attn_ref.check(q, k, v, out, DT[dt], where=where, pattern=pattern))


class _Notes:
    def __init__(self, dt):
        self.dt, self.worst, self.fails, self.n = dt, (0.0, ""), [], 0

    def __call__(self, v):
        self.n += 1
        if v.ratio > self.worst[0]:
            self.worst = (v.ratio, v.where)
        if not v.ok:
            self.fails.append(v.message())

    def finish(self, what):
        print(f"\n{what}: {self.n} launches checked, worst error/bound {self.worst[0]:.3f} at {self.worst[1]}")
        if self.worst[0] > _WORST.get(self.dt, (0.0, ""))[0]:
            _WORST[self.dt] = self.worst
        assert not self.fails, f"{len(self.fails)} check(s) failed:\n" + "\n".join(self.fails[:20])


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("C,col_split,inst", GRID, ids=[f"C{C}_cs{cs}" for C, cs, _ in GRID])
def test_every_pattern_against_fp64(C, col_split, inst, dt, dev):
    note = _Notes(dt)
    for L in (L_ALL if C in C_EVERY_L else L_FEW):
        assert instantiation(C, 3, L, col_split) == inst
        for pattern in attn_ref.PATTERNS:
            _run(pattern, 3, L, C, dt, col_split, note)
    note.finish(f"C={C} col_split={col_split} {dt}")
    _RAN.add((C, col_split, dt))


@pytest.mark.parametrize("dt", list(DT))
def test_eight_key_tiles(dt, dev):
    note = _Notes(dt)
    for pattern in ("asc", "desc", "peak"):
        _run(pattern, 1, 1024, 128, dt, 0, note)
    note.finish(f"L=1024 C=128 {dt}")


@pytest.mark.parametrize("dt", list(DT))
def test_split_threshold(dt, dev):
    """160 query tiles still split the output channels over two workgroups, 161 do not"""
    assert instantiation(264, 5, 1024, 1) == (4, 2) and 5 * (1024 // 32) == 160
    assert instantiation(264, 7, 736, 1) == (4, 1) and 7 * (736 // 32) == 161
    note = _Notes(dt)
    for B, L in ((5, 1024), (7, 736)):
        for pattern in ("rand", "peak"):
            _run(pattern, B, L, 264, dt, 1, note)
    note.finish(f"split threshold {dt}")


@pytest.mark.parametrize("dt", list(DT))
def test_workgroup_remap(dt, dev):
    """B * QT * CS a multiple of 8 (workgroups remapped so that one image's tiles share an XCD) and not"""
    note = _Notes(dt)
    for C, cs in ((72, 0), (392, 1)):
        for B in (8, 3):
            total = B * 2 * instantiation(C, B, 33, cs)[1]
            assert (total % 8 == 0) == (B == 8)
            for pattern in ("rand", "peak", "neg"):
                _run(pattern, B, 33, C, dt, cs, note)
    note.finish(f"workgroup remap {dt}")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("col_split", [0, 1])
@pytest.mark.parametrize("L,C", [(129, 200), (300, 392)])
def test_images_independent_and_launches_repeatable(L, C, col_split, dt, dev):
    q, k, v = (t.to(DT[dt]) for t in attn_ref.make_pattern("rand", L, C, 3, device=dev))
    out = _launch(q, k, v, col_split)
    again = _launch(q, k, v, col_split)
    assert same_bits(out, again), "two launches of the same input differ"
    for b in range(3):
        alone = _launch(q[b:b + 1], k[b:b + 1], v[b:b + 1], col_split)
        assert same_bits(out[b:b + 1], alone), f"image {b} of a B = 3 launch differs from the image alone"
    planner = _launch(q, k, v, col_split, padded=False)
    assert same_bits(out, planner), "the padded and the q-first layout differ"


def test_attention_wrapper_refuses_cpu_tensors(dev):
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    qkv, out = torch.zeros((4, 24)), torch.zeros((4, 8))
    with pytest.raises(DsxError):
        engine.attention(qkv, 0, 8, 16, 1, 4, 8, out)
    with pytest.raises(DsxError):
        engine.attention(qkv.to(dev), 0, 8, 16, 1, 4, 8, out)
    with pytest.raises(DsxError):
        engine.attention(qkv.to(dev), 0, 8, 16, 1, 4, 8, out.to(dev).half())


def test_every_instantiation_was_launched():
    """all fifteen k_attn<ST, NDB, CS> (runs after the grid; skipped when only part of it ran, e.g. with -k)"""
    grid = {(C, cs, dt) for C, cs, _ in GRID for dt in DT}
    if grid - _RAN:
        pytest.skip(f"needs the whole grid of this module in this session; missing {len(grid - _RAN)} ids")
    want = {(st, ndb, cs) for st in ST.values() for ndb, cs in C_TABLE}
    print("\nlaunched: " + " ".join("<%d,%d,%d>" % t for t in sorted(_LAUNCHED)))
    print("worst error/bound per type: " + "  ".join(f"{d} {r:.3f} ({w})" for d, (r, w) in sorted(_WORST.items())))
    assert len(want) == 15 and _LAUNCHED == want, f"missing {want - _LAUNCHED}, unexpected {_LAUNCHED - want}"
