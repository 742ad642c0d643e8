"""The bits of every kernel that reduces through csrc/dsx_reduce.h, on the MI355X (`-m gpu`).

"Fixed order, bitwise reproducible" is otherwise only tested as "two runs agree".  tests/golden/reduce_bits.npz holds
the outputs of the cases below as the libraries of the commits named in its ``meta`` entry produced them -- for every
group of cases the commit in front of the one that restated its reductions (the shared reduction; the row reduction and
the PSNR accumulator); tools/gen_reduce_golden.py wrote it through these same functions with that commit's library
loaded.  The comparison is on the raw bits, no tolerance: a butterfly or a combine whose order changes shows here, and
the fix is the order, never the fixture.

Shapes: the smallest that give a full chunk, a ragged tail with partly idle waves and more than one workgroup per
reduction (stated per case).  Inputs come from seeded CPU generators; only outputs are stored."""
import numpy as np
import pytest
import torch

from tests.bits import bits, same_bits
from tests.reduce_cases import CASES

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def golden():
    from tests.util import load_golden
    return load_golden("reduce_bits")


@pytest.mark.parametrize("case", list(CASES))
def test_bits_equal_the_recorded_ones(golden, case):
    got = CASES[case]()
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(case + "/")}
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(got):
        g, w = np.asarray(got[k]), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (case, k, g.dtype, w.dtype, g.shape, w.shape)
        differ = int((bits(g) != bits(w)).sum())
        print(f"{case}/{k}: {g.dtype} {g.shape}, {differ} of {g.size} values differ from {str(golden['meta'])}")
        assert same_bits(g, w), (case, k)
