"""The cases of tests/golden/resize_pil.npz (written by PIL itself): the fixture, a case's input regenerated from its seed,
and the byte-for-byte check of a case's three outputs."""
import hashlib
import json
import os

import numpy as np

from tests.util import GOLDEN


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "resize_pil.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def make_input(seed, h, w, mode):
    """The input of a fixture case (tools/gen_resize_golden.py: make_input), regenerated from its seed."""
    c = 3 if mode == "RGB" else 1
    if seed is None:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * (ch + 1) + y * (3 - ch)) % 256 for ch in range(c)], axis=-1).astype(np.uint8)
    else:
        a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    return a if c == 3 else a[:, :, 0]


def check_case(z, i, m, outs):
    """0 differing bytes between `outs` = [lr, hr, sr] and case i of the fixture (bytes, or digest and strided grid)."""
    for key, o in zip(("lr", "hr", "sr"), outs):
        o = np.ascontiguousarray(o)
        if m["how"] == "full":
            exp = z[f"c{i}_{key}"]
            assert o.shape == exp.shape and int((o != exp).sum()) == 0, (m["name"], key)
        else:
            assert list(o.shape) == m[f"shape_{key}"], (m["name"], key)
            s = o.shape[0] // 32 if o.shape[0] >= 32 else 1
            assert np.array_equal(o[::s, ::s][:32, :32], z[f"c{i}_{key}_grid"]), (m["name"], key)
            assert hashlib.sha256(o.tobytes()).hexdigest() == m[f"sha256_{key}"], (m["name"], key)
