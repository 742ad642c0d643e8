"""Writes tests/golden/reduce_bits.npz: the outputs of the cases of tests/test_gpu_reduce_bits.py, on one MI355X,
from a library built from the commit IN FRONT of the change the cases guard (csrc/dsx_reduce.h for the first seven,
the row reduction and the PSNR accumulator for the later four) -- never from this tree's own library: a fixture made by
the code under test proves nothing.

    git worktree add /tmp/parent <commit> && bash /tmp/parent/diffsplitting_amd/csrc/build.sh
    DSX_LIB_PATH=/tmp/parent/diffsplitting_amd/libdsx.so python tools/gen_reduce_golden.py <commit> [out.npz] [case ...]

Without case names every case is recorded and the file is written anew.  With case names only those are recorded and
MERGED into the existing file: every array the file already holds is kept as it is (checked on the bytes after the
write; a named case that the file already holds is refused), and ``meta`` gains a sentence that names the commit of the
new group.

The Python side (wrappers, case list) is this tree's; only the library differs.  Only outputs are stored, a few KB per
case; the inputs come from the seeded generators of the test module."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library: both then share torch's HIP runtime, as in the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT = os.path.join(ROOT, "tests", "golden", "reduce_bits.npz")


def merge(old, new, note):
    """The arrays of ``old`` untouched, those of ``new`` added, ``meta`` = the old one and ``note``."""
    clash = sorted(set(old) & set(new))
    assert not clash, f"already recorded, not overwritten: {clash}"
    out = {k: v for k, v in old.items() if k != "meta"}
    out.update(new)
    out["meta"] = np.array("; ".join(([str(old["meta"])] if "meta" in old else []) + [note]))
    return out


def check_kept(path, old):
    """every array of ``old`` but meta is in the file at ``path`` with the same dtype, shape and bytes"""
    with np.load(path) as z:
        for k, v in old.items():
            if k != "meta":
                w = z[k]
                assert w.dtype == v.dtype and w.shape == v.shape and w.tobytes() == v.tobytes(), k


def main(commit, path=DEFAULT, *names):
    lib_path = os.environ.get("DSX_LIB_PATH")
    assert lib_path, "set DSX_LIB_PATH to the library built from the recorded commit"
    assert os.path.realpath(lib_path) != os.path.realpath(os.path.join(ROOT, "diffsplitting_amd", "libdsx.so")), \
        "the fixture is recorded from the parent's library, not from this tree's"
    from diffsplitting_amd import _lib
    from tests.reduce_cases import CASES
    assert _lib.LIB_PATH == lib_path
    unknown = [n for n in names if n not in CASES]
    assert not unknown, f"no such case: {unknown}; one of {list(CASES)}"
    arrs = {}
    for case in names or CASES:
        for k, v in CASES[case]().items():
            arrs[f"{case}/{k}"] = np.ascontiguousarray(v)
            print(f"{case}/{k}: {arrs[f'{case}/{k}'].dtype} {arrs[f'{case}/{k}'].shape}")
    old = {}
    if names:
        with np.load(path) as z:
            old = {k: z[k] for k in z.files}
        arrs = merge(old, arrs, f"{', '.join(names)}: recorded from commit {commit}")
    else:
        arrs["meta"] = np.array(f"recorded from commit {commit} (the library in front of csrc/dsx_reduce.h)")
    np.savez_compressed(path, **arrs)
    check_kept(path, old)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(old)} entries kept, meta: {arrs['meta']}")


if __name__ == "__main__":
    main(*sys.argv[1:])
