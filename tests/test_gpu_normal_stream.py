"""The engine's normal stream on the MI355X (`-m gpu`) against its restatement, tests/normal_ref.py: dsx_randn and
dsx_randn_samples value by value against the definition in dsx_kernels.h -- Philox4x32-10 keyed by the whole 64-bit seed,
counter (block lo, block hi, subsequence lo, subsequence hi), Box-Muller on (r0, r1) and (r2, r3), cos before sin.  Every
other kernel that draws normals is compared bit for bit with dsx_randn elsewhere in the suite; this file is what anchors
dsx_randn itself.

The bound.  `close` asks |got - z| <= K * 2^-24 * radius per element, z and radius in float64 from the float32 uniforms
and angle the device forms.  Expected from the operations: logf 1 ulp, a correctly rounded sqrtf 1/2, sincosf <= 2 ulp of
a value <= 1, the product 1/2: at most 4 units.  K is twice the largest ratio measured on the MI355X over every case
here and over the 2^22 + 4099 elements of tests/test_gpu_grid_caps.py, rounded up to an integer, so that another libm
build does not flip a test; a K above 8 is refused: a kernel that needs more is a finding, not a tolerance.
Measured maximum: 3.617 (element 1 672 145 of the 2^22 + 4099; 2.781 over the 1027-element cases, 2.513 over the sample
rows), so K = ceil(2 * 3.617) = 8 (tests/normal_ref.py, K_DEVICE).

Not covered on the device: counter word 1 (block index >> 32) needs a stream of 2^34 elements; only the restatement's
known-answer vector with a non-zero second counter word (tests/test_normal_ref_cpu.py) covers it.
"""
import numpy as np
import pytest
import torch

from tests import normal_ref as nr
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
N = 1027                                  # 256 whole Philox blocks and a cut one; more than one workgroup
BIG = (7 | 5 << 40, (3 << 24) | 1 | 1 << 60)
CASES = [(0, 0), (11, 5), (2 ** 64 - 1, 2 ** 64 - 1), BIG]


def check_stream(name, got, seed, subseq):
    """every element of ``got`` against the first got.numel() elements of the restated stream (seed, subseq)"""
    z, radius = nr.stream(seed, subseq, got.numel())
    ok, worst, i = nr.close(got.cpu().numpy(), z, radius, nr.K_DEVICE)
    print(f"\n{name}: max |got - z| / (2^-24 radius) = {worst:.3f} at element {i} (K = {nr.K_DEVICE})")
    assert ok, (name, worst, i, float(got.reshape(-1)[i]), float(z[i]))
    return worst


def test_k_is_within_its_limit():
    assert 1 <= nr.K_DEVICE <= nr.K_LIMIT == 8


@pytest.mark.parametrize("seed,subseq", CASES)
def test_randn_is_the_restated_stream(seed, subseq):
    from diffsplitting_amd import engine
    got = engine.randn((N,), seed, subsequence=subseq)
    assert got.shape == (N,) and got.dtype == torch.float32
    check_stream(f"randn seed {seed:#x} subsequence {subseq:#x}", got, seed, subseq)


def test_high_words_of_seed_and_subsequence_reach_the_generator():
    """The cases above prove each stream against its own restatement; this names the failure: a dropped high word of
    the seed (the second key word) or of the subsequence (the fourth counter word)."""
    from diffsplitting_amd import engine
    base = engine.randn((N,), 7, subsequence=3)
    assert not same_bits(engine.randn((N,), 7 | 1 << 40, subsequence=3), base), "seed bit 40 is ignored"
    assert not same_bits(engine.randn((N,), 7, subsequence=3 | 1 << 60), base), "subsequence bit 60 is ignored"
    assert same_bits(engine.randn((N,), 7, subsequence=3), base)


@pytest.mark.parametrize("chw", [(3, 5, 7), (3, 8, 8)])                 # 105 elements: scalar stores; 192: 16-byte stores
def test_randn_samples_rows_are_the_restated_streams(chw):
    """Row b is the stream (seed, id_b << 24 | draw) from its first element, whatever the row's position: ids at both
    ends of their 40 bits and one above 2^32, the last draw ordinal."""
    from diffsplitting_amd import engine
    ids, draw, seed = [0, 2 ** 40 - 1, 1 << 33], 2 ** 24 - 1, BIG[0]
    got = engine.randn_samples((len(ids),) + chw, seed, ids, draw)
    assert got.shape == (3,) + chw
    for b, sid in enumerate(ids):
        sub = nr.sample_subseq(sid, draw)
        assert sub == (sid << 24) | draw
        check_stream(f"randn_samples chw {chw} id {sid:#x}", got[b], seed, sub)
    assert not same_bits(got[0], got[1]) and not same_bits(got[0], got[2])
