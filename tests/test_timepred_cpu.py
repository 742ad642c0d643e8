"""The TimePredictor entry points without a GPU: the new ABI symbol and its host-side refusals (fake non-NULL device
pointers: a call that got past the checks would not return INVALID with these messages), the argument refusals of the
two command lines, and the batching arithmetic of ``validation_loss`` against a torch restatement of the reference's
loop (time_prediction_training.py:135-140, 144)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.nets import dbl, i64, write_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsx_tiles_gather_mix_items"


def test_symbol_declared_registered_and_exported():
    from diffsplitting_amd import _lib
    with open(os.path.join(ROOT, "include", "dsx.h")) as f:
        header = f.read()
    assert f"int {NAME}(" in header
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 13
    assert hasattr(_lib.lib, NAME)
    assert _lib.lib.dsx_abi_version() == 2


def test_host_side_refusals_name_the_item():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    err = lambda: lib.dsx_last_error().decode()
    fake = C.c_void_p(4096)
    shape, patch = i64(2, 8, 9), i64(1, 4, 3)
    norm = dbl(0, 1, 0, 1)
    starts = i64(0, 0, 0, 1, 4, 6, 0, 1, 1)                              # item 1 is the last valid corner
    t3, rows3 = dbl(0.0, 0.5, 1.0), dbl(*([0, 1, 0, 2] * 3))

    def call(frames0=fake, frames1=fake, shape=shape, patch=patch, starts=starts, count=3, norm=norm, t=t3, lohi=rows3,
             target=None, mix=None, cls=fake):
        return lib.dsx_tiles_gather_mix_items(frames0, frames1, shape, patch, starts, count, norm, t, lohi, target, mix,
                                              cls, None)

    inf, nan = float("inf"), float("nan")
    # NULL pointers
    assert call(cls=None) < 0 and "every output pointer is NULL" in err()
    for kw in ("frames0", "frames1", "shape", "patch", "starts", "norm", "t"):
        assert call(**{kw: None}) < 0 and "null argument" in err(), kw
    assert call(lohi=None) < 0 and "(lo, hi)" in err()
    # statistics
    assert call(norm=dbl(0, 1, nan, 1)) < 0 and "finite" in err()
    assert call(norm=dbl(0, 0, 0, 1)) < 0 and "zero standard deviation" in err()
    # count
    for count in (-1, 65536):
        assert call(count=count) < 0 and "count" in err() and "65535" in err()
    # per item: t, rows, location -- the message names the item
    assert call(t=dbl(0.0, inf, 1.0)) < 0 and "item 1" in err() and "finite" in err()
    assert call(t=dbl(0.0, 0.5, nan), target=fake, cls=None, lohi=None) < 0 and "item 2" in err() and "finite" in err()
    assert call(lohi=dbl(0, 1, 0, 2, 0, 1, 3, 3, 0, 1, 0, 2)) < 0 and "item 1" in err() and "differ" in err()
    assert call(lohi=dbl(0, 1, 0, 2, 0, 1, 0, 2, inf, 1, 0, 2)) < 0 and "item 2" in err() and "channel 0" in err()
    for bad, item in ((i64(0, 0, 0, 1, 5, 6, 0, 1, 1), 1), (i64(0, 0, 0, 1, 4, 7, 0, 1, 1), 1), (i64(2, 0, 0, 1, 4, 6, 0, 1, 1), 0),
                      (i64(0, 0, 0, 1, 4, 6, 0, -1, 1), 2), (i64(0, 0, 0, 1, 4, 6, 0, 1, 2 ** 32), 2)):
        assert call(starts=bad) < 0 and f"item {item} " in err() and "outside the frames" in err(), list(bad)
    assert call(patch=i64(1, 9, 3)) < 0 and "does not fit" in err()
    # nothing to do is not an error, and needs no device
    assert call(count=0) == 0


def test_split_refuses_the_mixed_flags_where_they_do_not_apply(tmp_path):
    from diffsplitting_amd import split
    indi, joint = write_config(tmp_path, "indi"), write_config(tmp_path, "joint_indi")
    with pytest.raises(SystemExit, match="--mix-t.*joint_indi"):
        split.main(["-c", indi, "--mix-t", "0.3", "--t-from", "given"])
    for flag, value in (("--time-predictor", joint), ("--time-predictor-checkpoint", "x.pth"), ("--mmse", "2"),
                        ("--t-from", "given")):
        with pytest.raises(SystemExit, match=f"{flag}.*joint_indi"):
            split.main(["-c", indi, flag, value])
        with pytest.raises(SystemExit, match=f"{flag}.*--mix-t"):
            split.main(["-c", joint, flag, value])
    with pytest.raises(SystemExit, match="--t-from classifier.*--time-predictor"):
        split.main(["-c", joint, "--mix-t", "0.3"])
    for bad in ("-0.01", "1.5", "nan"):
        with pytest.raises(SystemExit, match=r"--mix-t.*\[0, 1\]"):
            split.main(["-c", joint, "--mix-t", bad, "--t-from", "given"])
    with pytest.raises(SystemExit, match="--mmse 0"):
        split.main(["-c", joint, "--mix-t", "0.3", "--t-from", "given", "--mmse", "0"])
    with pytest.raises(SystemExit, match="--validate"):
        split.main(["-c", joint, "--mix-t", "0.3", "--t-from", "given", "--validate"])


def test_time_prediction_refusals(tmp_path):
    from diffsplitting_amd import time_prediction as TP
    from diffsplitting_amd._lib import DsxError
    cfg = write_config(tmp_path, "UnetClassifier")
    with pytest.raises(SystemExit, match="--sweep 0"):
        TP.main(["-c", cfg, "--datapath", "--sweep", "0"])
    with pytest.raises(SystemExit, match="-p train"):
        TP.main(["-c", cfg, "--datapath", "-p", "train"])
    with pytest.raises(SystemExit, match="--datapath"):
        TP.main(["-c", cfg])
    with pytest.raises(DsxError, match="loss_type = 'huber'"):
        TP.validation_loss(None, None, 3, "huber")
    with pytest.raises(DsxError, match="loss_type = 'huber'"):
        TP.batch_losses(np.zeros(4, np.float32), np.zeros(4), 3, "huber")
    with pytest.raises(DsxError, match="loss_type = 'huber'"):            # from the config, before anything is built
        TP.main(["-c", write_config(tmp_path, "UnetClassifier", loss_type="huber"), "--datapath"])
    with pytest.raises(NotImplementedError, match="Tiled prediction"):
        TP.get_datasets({}, tiled_pred=True)


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_batching_arithmetic_equals_the_reference_loop(loss_type):
    """The reference: per batch ``loss_fn(y_pred, y.type(torch.float32)).item()`` in float32, ``np.mean`` over the
    batches.  ``batch_losses`` takes each batch mean in float64 from the same float32 values.  Bound per batch of n
    items: every term carries at most 2 roundings (difference, square), the float32 sum n - 1, the division one, all
    on non-negative terms -- |fp32 - fp64| <= (n + 2) * 2^-24 * (the fp64 mean), to first order (1 % slack for the
    higher orders); the mean over batches inherits the largest of them."""
    from diffsplitting_amd import time_prediction as TP
    loss_fn = torch.nn.L1Loss() if loss_type == "l1" else torch.nn.MSELoss()
    rng = np.random.default_rng(7)
    for n, batch in ((8, 3), (8, 4), (8, 8), (8, 1), (23, 5), (23, 64), (1, 3)):
        pred = rng.random(n).astype(np.float32)
        t = rng.integers(0, 100, n) / 100                                   # float64, as sample_t returns it
        ref = [loss_fn(torch.from_numpy(pred[i:i + batch]), torch.from_numpy(t[i:i + batch]).type(torch.float32)).item()
               for i in range(0, n, batch)]
        val_loss, per_batch = TP.batch_losses(pred, t, batch, loss_type)
        assert per_batch.dtype == np.float64 and per_batch.shape == (len(ref),) and isinstance(val_loss, float)
        bound = 1.01 * (min(n, batch) + 2) * 2.0 ** -24 * per_batch
        assert (np.abs(per_batch - np.array(ref)) <= bound).all(), (n, batch)
        assert abs(val_loss - np.mean(ref)) <= bound.max(), (n, batch)
        assert val_loss == float(np.mean(per_batch))
