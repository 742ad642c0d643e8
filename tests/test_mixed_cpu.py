"""Mixed-input evaluation, the parts that need no GPU: the restatements of tests/mixed_ref.py against the fixture the
reference's own code produced (tests/golden/mix_range.npz, tools/gen_mix_range_golden.py) and against torch's float32
evaluation of the notebook expressions; the derived bound's sensitivity; the new entry points' host-side refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mixed_ref as MR
from tests.bits import same_bits
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_VALUES = [0.0, 0.1, 0.29, 0.35000000000000003, 0.5, 1.0]


def _case_c(g):
    """normalised float32 channels of two patches of fixture case c and its 100-step table"""
    mean, std = g["ds_mean_target"], g["ds_std_target"]
    t0 = MR.normalize(g["c_ch0"][:, :32, 16:48], mean[0], std[0])
    t1 = MR.normalize(g["c_ch1"][:, :32, 16:48], mean[1], std[1])
    return t0, t1, g["c_table_100"]


def test_restated_table_equals_the_reference_bitwise():
    g = load_golden("mix_range")
    for name in [str(c) for c in g["cases"]]:
        for n in [int(v) for v in g["timesteps"]]:
            tab = MR.range_table(g[f"{name}_ch0"], g[f"{name}_ch1"], n, g[f"{name}_mean_target"], g[f"{name}_std_target"])
            ref = g[f"{name}_table_{n}"]
            assert ref.shape == (n + 1, 2) and ref.dtype == np.float64
            assert same_bits(tab, ref), (name, n)
    # the fixture is what the issue asks for: an extreme on the first and the last pixel, an awkward pixel count
    a = g["a_table_100"]
    assert g["a_ch0"].reshape(-1)[0] == g["a_ch0"].max() and g["a_ch1"].reshape(-1)[-1] == g["a_ch1"].max()
    assert g["b_ch0"].size % 64 != 0 and a[0, 1] != a[100, 1]


def test_fp32_chain_equals_torch_float32_bitwise():
    """cells 40 / 43 of EvaluateJointIndiIterative.ipynb and cell 4 of time_prediction_evaluation.ipynb, evaluated by
    torch on a float32 tensor with Python / numpy-float64 scalars, exactly as written there."""
    g = load_golden("mix_range")
    t0, t1, table = _case_c(g)
    tar = torch.from_numpy(np.stack([t0, t1], axis=1))                     # (b, 2, p, p)
    tab = {i: [table[i, 0], table[i, 1]] for i in range(101)}
    for t in T_VALUES:
        inp1 = tar[:, :1] * (1 - t) + tar[:, 1:2] * t                     # get_inputs
        inp2 = tar[:, 1:2] * (1 - t) + tar[:, :1] * t
        minv, maxv = tab[int((1 - t) * 100)]                                # normalize_indi1
        c1 = 2 * (inp1 - minv) / (maxv - minv) - 1
        minv, maxv = tab[int(t * 100)]                                      # normalize_indi2
        c2 = 2 * (inp2 - minv) / (maxv - minv) - 1
        assert c1.dtype == torch.float32
        mix, cls = MR.chain_f32(t0, t1, t, MR.rows(table, t))
        assert same_bits(mix[0], inp1[:, 0].numpy()) and same_bits(mix[1], inp2[:, 0].numpy())
        assert same_bits(cls[0], c1[:, 0].numpy()) and same_bits(cls[1], c2[:, 0].numpy()), t
        mt = np.float64(t)                                                  # the sweep: np.arange values, channel 1
        inp = tar[:, :1] * mt + tar[:, 1:2] * (1 - mt)
        t_min, t_max = tab[int(mt * 100)]
        sw = 2 * (inp - t_min) / (t_max - t_min) - 1
        assert same_bits(cls[1], sw[:, 0].numpy()), t
    assert int(0.29 * 100) == 28                                            # the truncating row index is exercised


def test_fp32_chain_equals_the_reference_items_within_the_bound():
    """TimePredictorDataset items made by the reference class.  Made under numpy 1.x they are float32 and must be equal
    bitwise; under numpy 2 the reference's normalisation step runs in float64 on the float32 mix, so the chain's
    remaining roundings (difference, quotient, difference, the table constants) separate the two: within E_c."""
    g = load_golden("mix_range")
    mean, std, table = g["ds_mean_target"], g["ds_std_target"], g["c_table_100"]
    for k, idx in enumerate(g["item_indices"]):
        t = float(g["item_t"][k])
        t_int = int(round(t * 100))
        assert t == t_int / 100
        f, r = int(idx) // 4, int(idx) % 4                                  # patch_location (:215-225), 64 x 64, p = 32
        y, x = (r // 2) * 32, (r % 2) * 32
        t0 = MR.normalize(g["c_ch0"][f, y:y + 32, x:x + 32], mean[0], std[0])
        t1 = MR.normalize(g["c_ch1"][f, y:y + 32, x:x + 32], mean[1], std[1])
        lohi = (table[t_int, 0], table[t_int, 1]) * 2
        _, cls = MR.chain_f32(t0, t1, t, lohi)
        item = g["item_inp"][k]
        assert item.shape == (1, 32, 32)
        if item.dtype == np.float32:
            assert same_bits(cls[1], item[0])
        else:
            _, bound = MR.chain_bound(t0, t1, t, lohi)
            err = np.abs(cls[1].astype(np.float64) - item[0])
            print(f"item {idx}: max err {err.max():.3e}, bound there {bound[1].reshape(-1)[err.argmax()]:.3e}")
            assert (err <= bound[1]).all()


def test_bound_holds_and_is_sensitive():
    g = load_golden("mix_range")
    t0, t1, table = _case_c(g)
    for t in T_VALUES:
        lohi = MR.rows(table, t)
        mix, cls = MR.chain_f32(t0, t1, t, lohi)
        m64, c64 = MR.chain_f64(t0, t1, t, lohi)
        bm, bc = MR.chain_bound(t0, t1, t, lohi)
        assert (np.abs(mix - m64) <= bm).all() and (np.abs(cls - c64) <= bc).all(), t
    t = 0.29
    lohi = MR.rows(table, t)
    _, c64 = MR.chain_f64(t0, t1, t, lohi)
    _, bc = MR.chain_bound(t0, t1, t, lohi)
    n = len(table) - 1
    r0, r1 = int((1 - t) * n), int(t * n)
    assert r1 == 28
    neighbour = (table[r0 + 1][0], table[r0 + 1][1], table[r1 + 1][0], table[r1 + 1][1])     # row 29: round(t n)
    _, wrong_row = MR.chain_f32(t0, t1, t, neighbour)
    assert (np.abs(wrong_row - c64) > bc).mean() > 0.9
    _, swapped = MR.chain_f32(t0, t1, 1 - t, lohi)                                            # weights swapped
    assert (np.abs(swapped - c64) > bc).mean() > 0.9


def test_new_symbols_exported_and_abi_unchanged():
    from diffsplitting_amd import _lib
    for name in ("dsx_mix_range_blocks", "dsx_mix_range", "dsx_tiles_gather_mix", "dsx_tileplan_gather_mix"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert _lib.lib.dsx_abi_version() == 2
    assert _lib.lib.dsx_mix_range_blocks(1, 1) == 1
    assert 1 <= _lib.lib.dsx_mix_range_blocks(10 * 2048 * 2048, 100) <= 65535


def test_compat_import_line_resolves(tmp_path):
    code = ("from data.time_predictor_dataset import compute_input_normalization_dict, TimePredictorDataset\n"
            "import diffsplitting_amd.data.time_predictor_dataset as real\n"
            "assert compute_input_normalization_dict is real.compute_input_normalization_dict\n"
            "print('compat ok')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "diffsplitting_amd", "compat"), ROOT])
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compat ok" in r.stdout, r.stderr[-2000:]


def test_host_side_refusals():
    """Argument checks that must fail with a message before any device work (fake non-null device pointers: a call
    that got past the checks would not return an INVALID status with these messages)."""
    from diffsplitting_amd import _lib
    from diffsplitting_amd.data.split_dataset import DataLocation
    from diffsplitting_amd.data.time_predictor_dataset import TimePredictorDataset, compute_input_normalization_dict
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    fake = C.c_void_p(4096)
    d4 = lambda *v: (C.c_double * 4)(*v)
    out = (C.c_double * 4)()
    for n in (0, -3, 1025):
        assert lib.dsx_mix_range_blocks(1000, n) < 0 and "n_timesteps" in err()
        assert lib.dsx_mix_range(fake, fake, 1000, d4(0, 1, 0, 1), n, fake, out, None) < 0 and "n_timesteps" in err()
    assert lib.dsx_mix_range(fake, fake, 1000, d4(0, 0, 0, 1), 1, fake, out, None) < 0 and "zero standard deviation" in err()
    assert lib.dsx_mix_range(fake, fake, 1000, d4(0, 1, float("nan"), 1), 1, fake, out, None) < 0 and "finite" in err()
    assert lib.dsx_mix_range(fake, fake, 0, d4(0, 1, 0, 1), 1, fake, out, None) < 0
    i3 = lambda *v: (C.c_int64 * 3)(*v)
    args = (fake, fake, i3(1, 8, 8), i3(1, 4, 4), i3(0, 0, 0), None, 1)
    assert lib.dsx_tiles_gather_mix(*args, d4(0, 1, 0, 1), 0.5, None, None, None, None, None) < 0 and "NULL" in err()
    assert lib.dsx_tiles_gather_mix(*args, d4(0, 1, 0, 0), 0.5, None, fake, None, None, None) < 0 and "zero standard deviation" in err()
    assert lib.dsx_tiles_gather_mix(*args, d4(0, 1, 0, 1), 0.5, None, None, None, fake, None) < 0 and "lo, hi" in err()
    assert lib.dsx_tiles_gather_mix(*args, d4(0, 1, 0, 1), 0.5, d4(0, 1, 2, 2), None, None, fake, None) < 0 and "differ" in err()
    assert lib.dsx_tiles_gather_mix(*args, d4(0, 1, 0, 1), float("inf"), None, fake, None, None, None) < 0 and "finite" in err()
    assert lib.dsx_tileplan_gather_mix(None, fake, fake, 0, 1, 1, d4(0, 1, 0, 1), 0.5, None, None, None, None, None) < 0 and "NULL" in err()
    # the Python layer: the same refusals, and the training-time constructor arguments
    frames = {0: np.zeros((1, 8, 8), np.float32), 1: np.ones((1, 8, 8), np.float32)}
    one = np.array([1.0, 1.0])
    for n in (0, 1025):
        with pytest.raises(_lib.DsxError, match="n_timesteps"):
            compute_input_normalization_dict(frames, n, one, one)
    with pytest.raises(_lib.DsxError, match="std"):
        compute_input_normalization_dict(frames, 20, one, np.array([1.0, 0.0]))
    loc = DataLocation(arrays=(frames[0], frames[1]))
    with pytest.raises(_lib.DsxError, match="gaussian_noise_std_factor"):
        TimePredictorDataset("Hagen", loc, 4, gaussian_noise_std_factor=0.1)
    with pytest.raises(_lib.DsxError, match="enable_transforms"):
        TimePredictorDataset("Hagen", loc, 4, enable_transforms=True)
    with pytest.raises(_lib.DsxError, match="uncorrelated_channels"):
        TimePredictorDataset("Hagen", loc, 4, uncorrelated_channels=True)
