"""Writes tests/golden/reduce_bits.npz: the outputs of the cases of tests/test_gpu_reduce_bits.py, on one MI355X,
from a library built from the commit IN FRONT of the shared reduction (csrc/dsx_reduce.h) -- never from this tree's own
library: a fixture made by the code under test proves nothing.

    git worktree add /tmp/parent <commit> && bash /tmp/parent/diffsplitting_amd/csrc/build.sh
    DSX_LIB_PATH=/tmp/parent/diffsplitting_amd/libdsx.so python tools/gen_reduce_golden.py <commit> [out.npz]

The Python side (wrappers, case list) is this tree's; only the library differs.  Only outputs are stored, a few KB per
case; the inputs come from the seeded generators of the test module."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library: both then share torch's HIP runtime, as in the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(commit, path=os.path.join(ROOT, "tests", "golden", "reduce_bits.npz")):
    lib_path = os.environ.get("DSX_LIB_PATH")
    assert lib_path, "set DSX_LIB_PATH to the library built from the recorded commit"
    assert os.path.realpath(lib_path) != os.path.realpath(os.path.join(ROOT, "diffsplitting_amd", "libdsx.so")), \
        "the fixture is recorded from the parent's library, not from this tree's"
    from diffsplitting_amd import _lib
    from tests.test_gpu_reduce_bits import CASES
    assert _lib.LIB_PATH == lib_path
    arrs = {}
    for case, fn in CASES.items():
        for k, v in fn().items():
            arrs[f"{case}/{k}"] = np.ascontiguousarray(v)
            print(f"{case}/{k}: {arrs[f'{case}/{k}'].dtype} {arrs[f'{case}/{k}'].shape}")
    arrs["meta"] = np.array(f"recorded from commit {commit} (the library in front of csrc/dsx_reduce.h)")
    np.savez_compressed(path, **arrs)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main(*sys.argv[1:3])
