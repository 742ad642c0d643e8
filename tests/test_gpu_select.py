"""Order statistics by radix select (dsx_order_stats) and the integer-stack widening (dsx_frames_to_f32) on the
MI355X, against numpy float64 on the host (`-m gpu`).  The select's counts are integers, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N_SMALL = 37 * 41           # 1517
N_MID = 3 * 37 * 41         # 4551: (n - 1) * 0.5 is an integer


def _select(a, b, w0, w1, ranks):
    from diffsplitting_amd.data.split_dataset import order_stats_device
    ta = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tb = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return order_stats_device(ta, tb, w0, w1, ranks)


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 4000, size=N_SMALL).astype(np.float32)
    b = rng.integers(0, 65536, size=N_SMALL).astype(np.float32)
    return a, b


@pytest.mark.parametrize("weights", [(0.3, 0.7), (1.0, 1.0), None])
def test_full_sort_reproduced(pairs, weights):
    """All 1517 ranks equal numpy's sort of the float64 key.  With (0.3, 0.7) an fma on either product or a float32
    key changes tens to hundreds of the sorted entries (measured on the host for this size), so each of those
    mistakes fails here."""
    a, b = pairs
    ranks = np.arange(N_SMALL)
    if weights is None:
        want = np.sort(a.astype(np.float64))
        got = _select(a, None, 1.0, 0.0, ranks)
    else:
        want = np.sort(a.astype(np.float64) * weights[0] + b.astype(np.float64) * weights[1])
        got = _select(a, b, weights[0], weights[1], ranks)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    # ranks in any order, with repeats: each entry answers its own rank
    shuffled = np.random.default_rng(1).permutation(np.concatenate([ranks[::7], ranks[::7]]))
    again = _select(a, None, 1.0, 0.0, shuffled) if weights is None else _select(a, b, weights[0], weights[1], shuffled)
    assert np.array_equal(again, want[shuffled])


def test_single_source_with_sign():
    rng = np.random.default_rng(8)
    x = rng.normal(0.0, 1e3, size=N_MID).astype(np.float32)
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    x[:10] = np.array([0.0, -0.0, fmax, -fmax, tiny, -tiny, np.float32(1e-40), np.float32(-1e-40), 1.0, -1.0], np.float32)
    x = x[rng.permutation(N_MID)]
    n = N_MID
    ranks = np.unique(np.concatenate([[0, 1, n // 2, n - 2, n - 1], np.linspace(0, n - 1, 64).astype(np.int64)]))
    want = np.sort(x.astype(np.float64))[ranks]
    from diffsplitting_amd.data.split_dataset import order_stats_device
    tx = torch.from_numpy(x).cuda()
    assert tx[1:].data_ptr() % 16 == 4                             # a base that is not 16-byte aligned: the scalar form
    got = order_stats_device(tx[1:], tx[:-1], 1.0, 1.0, ranks[:-1])
    assert np.array_equal(got, np.sort(x[1:].astype(np.float64) + x[:-1].astype(np.float64))[ranks[:-1]])
    got = _select(x, None, 1.0, 0.0, ranks)
    assert np.array_equal(got, want)                               # by value: -0.0 == 0.0


def test_ties():
    same = np.full(N_MID, 1993.0, np.float32)
    assert np.array_equal(_select(same, None, 1.0, 0.0, [0, N_MID // 2, N_MID - 1]), [1993.0] * 3)
    two = np.full(N_MID, 5.0, np.float32)
    two[1234] = -3.0
    assert np.array_equal(_select(two, None, 1.0, 0.0, [0, 1, N_MID - 1]), [-3.0, 5.0, 5.0])
    two[1234] = 7.0
    assert np.array_equal(_select(two, two, 0.45, 0.55, [0, N_MID - 2, N_MID - 1]),
                          np.sort(two.astype(np.float64) * 0.45 + two.astype(np.float64) * 0.55)[[0, N_MID - 2, N_MID - 1]])
    assert np.array_equal(_select(np.array([-2.5], np.float32), None, 1.0, 0.0, [0]), [-2.5])          # count = 1
    assert np.array_equal(_select(np.array([2.0], np.float32), np.array([3.0], np.float32), 0.5, 2.0, [0, 0]), [7.0, 7.0])
    # 141171 elements, 60 % exactly 100.0: one bin above 65535 entries, several workgroups
    n = 3 * 211 * 223
    rng = np.random.default_rng(9)
    x = rng.integers(0, 65536, size=n).astype(np.float32)
    x[rng.permutation(n)[:int(n * 0.6)]] = 100.0
    s = np.sort(x.astype(np.float64))
    first, last = int(np.searchsorted(s, 100.0, "left")), int(np.searchsorted(s, 100.0, "right")) - 1
    assert last - first + 1 > 65535
    ranks = [0, first - 1, first, first + 1, (first + last) // 2, last - 1, last, last + 1, n - 1]
    assert np.array_equal(_select(x, None, 1.0, 0.0, ranks), s[ranks])
    y = rng.integers(0, 2000, size=n).astype(np.float32)
    sp = np.sort(x.astype(np.float64) * 0.45 + y.astype(np.float64) * 0.55)
    assert np.array_equal(_select(x, y, 0.45, 0.55, ranks), sp[ranks])


@pytest.mark.parametrize("weights", [[1, 1], [0.45, 0.55]])
def test_quantiles_equal_numpy_and_the_sort_path(weights):
    from diffsplitting_amd.data import split_dataset as SD
    rng = np.random.default_rng(10)
    ch0 = rng.gamma(2.0, 120.0, size=(3, 37, 41)).astype(np.float32)
    ch1 = np.floor(rng.gamma(3.0, 300.0, size=(3, 37, 41))).astype(np.float32)
    d0, d1 = ch0.reshape(-1).astype(np.float64), ch1.reshape(-1).astype(np.float64)
    t0, t1 = torch.from_numpy(ch0).cuda(), torch.from_numpy(ch1).cuda()
    for q in (0.0, 0.5, 0.98, 0.995, 1.0):
        nd = SD.compute_normalization_dict({0: t0, 1: t1}, weights, q_val=q)
        # the dict as it was built before the select: three sorts through quantile_device (unchanged)
        s0, s1 = SD.quantile_device(t0.reshape(-1), q), SD.quantile_device(t1.reshape(-1), q)
        si = SD.quantile_device(t0.reshape(-1).to(torch.float64) * weights[0] + t1.reshape(-1).to(torch.float64) * weights[1], q)
        old = {"mean_input": si / 2, "std_input": si / 2, "mean_target": np.array([s0 / 2, s1 / 2]),
               "std_target": np.array([s0 / 2, s1 / 2]), "target0_max": s0, "target1_max": s1, "input_max": si}
        ref = {"target0_max": np.quantile(d0, q), "target1_max": np.quantile(d1, q),
               "input_max": np.quantile(d0 * weights[0] + d1 * weights[1], q)}
        assert set(nd) == set(old)
        for k in old:
            assert isinstance(nd[k], type(old[k])) and np.asarray(nd[k]).dtype == np.float64, k
            assert np.array_equal(np.asarray(nd[k]), np.asarray(old[k])), (k, q)
        for k in ref:
            assert nd[k] == ref[k], (k, q)
        assert nd["mean_input"] == ref["input_max"] / 2 and nd["std_target"][1] == ref["target1_max"] / 2


def _widen(x, clip):
    from diffsplitting_amd.data.split_dataset import frames_to_device
    return frames_to_device(x, torch.device("cuda"), clip).cpu().numpy()


def test_widening():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 4000, size=N_MID).astype(np.uint16)
    x[:3] = (65535, 1993, 1994)
    for arr in (x, x[:N_MID - 3].reshape(4, -1), x[:5]):
        got = _widen(arr, 1993)
        assert got.dtype == np.float32 and got.shape == arr.shape
        assert np.array_equal(got, np.minimum(arr, 1993).astype(np.float32)) and got.max() == 1993.0
        assert np.array_equal(_widen(arr, None), arr.astype(np.float32))
    b = rng.integers(0, 256, size=N_MID).astype(np.uint8)
    assert np.array_equal(_widen(b, None), b.astype(np.float32))
    assert np.array_equal(_widen(b, 100), np.minimum(b, 100).astype(np.float32))
    # a destination that is not 16-byte aligned takes the scalar form: same values
    from diffsplitting_amd._lib import PIX_U16, check, lib
    src = torch.from_numpy(x.view(np.uint8)).cuda()
    dst = torch.zeros(N_MID + 1, dtype=torch.float32, device="cuda")
    check(lib.dsx_frames_to_f32(C.c_void_p(src.data_ptr()), PIX_U16, N_MID, 1993.0, C.c_void_p(dst.data_ptr() + 4),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert dst[0].item() == 0.0 and np.array_equal(dst[1:].cpu().numpy(), np.minimum(x, 1993).astype(np.float32))


def test_determinism(pairs):
    a, b = pairs
    ranks = np.arange(0, N_SMALL, 3)
    one, two = _select(a, b, 0.3, 0.7, ranks), _select(a, b, 0.3, 0.7, ranks)
    assert one.tobytes() == two.tobytes()
    x = np.random.default_rng(12).integers(0, 4000, size=N_MID).astype(np.uint16)
    assert _widen(x, 1993).tobytes() == _widen(x, 1993).tobytes()
