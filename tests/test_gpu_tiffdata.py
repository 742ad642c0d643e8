"""The Hagen path from its .tif stacks on the MI355X (`-m gpu`): file -> device -> statistics -> tiles, get_datasets
with the training stack's statistics, and split.main from the config's datapath to a written hyperstack."""
import json
import os

import numpy as np
import pytest
import torch

from tests import nets
from tests import tiff_files as TF

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _stack(seed, top, shape=(3, 64, 64)):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, size=shape).astype(np.uint16)


def _same_dataset(a, b):
    na, nb = a.get_normalization_dict(), b.get_normalization_dict()
    assert set(na) == set(nb)
    for k in na:
        assert np.asarray(na[k]).dtype == np.asarray(nb[k]).dtype and np.array_equal(np.asarray(na[k]), np.asarray(nb[k])), k
    assert len(a) == len(b)
    ta, tb = a.tiles(range(len(a))), b.tiles(range(len(b)))
    for k in ("input", "target"):
        assert ta[k].dtype == torch.float32 and torch.equal(ta[k], tb[k]), k
    assert torch.equal(a._dev[0], b._dev[0]) and torch.equal(a._dev[1], b._dev[1])


def test_dataset_from_files_equals_dataset_from_arrays(tmp_path):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    a, b = _stack(1, 4000), _stack(2, 3000)
    assert (a > 1993).any() and (b > 1993).any()
    pa, pb = str(tmp_path / "ch0.tif"), str(tmp_path / "ch1.tif")
    TF.pil_tiff(pa, a)
    TF.pil_tiff(pb, b)
    from_files = SplitDataset("Hagen", DataLocation(channelwise_fpath=(pa, pb)), 32)
    host = [np.minimum(x, 1993).astype(np.float32) for x in (a, b)]              # today's host conversion
    from_arrays = SplitDataset("Hagen", DataLocation(arrays=tuple(host)), 32)
    assert len(from_files) == 3 * 2 * 2 and float(from_files._dev[0].max()) == 1993.0
    _same_dataset(from_files, from_arrays)
    # one (N,H,W,2) file through fpath: unclipped, as the reference's _load_data_fpath
    both = np.stack([a, b], axis=-1)
    pf = str(tmp_path / "both.tif")
    TF.struct_tiff(pf, list(both), rows_per_strip=24)
    from_fpath = SplitDataset("Hagen", DataLocation(fpath=pf), 32, channel_weights=[0.45, 0.55])
    unclipped = SplitDataset("Hagen", DataLocation(arrays=(a.astype(np.float32), b.astype(np.float32))), 32,
                             channel_weights=[0.45, 0.55])
    assert float(from_fpath._dev[0].max()) > 1993.0
    _same_dataset(from_fpath, unclipped)


def _config(tmp_path, val_shape=(2, 96, 160)):
    """Train stacks up to ~1500 counts, val stacks up to ~600: clearly different statistics."""
    paths = {}
    for part, top, shape, seed in (("train", 1500, (3, 64, 64), 3), ("val", 600, val_shape, 5)):
        for ch in (0, 1):
            p = str(tmp_path / f"{part}_ch{ch}.tif")
            TF.pil_tiff(p, _stack(seed + ch, top // (ch + 1), shape))
            paths[part, ch] = p
    ds = lambda part: {"name": "Hagen", "datapath": {"ch0": paths[part, 0], "ch1": paths[part, 1]},
                       "uncorrelated_channels": False}
    cfg = {"name": "tiny_hagen_tif", "phase": "train", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 64, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 1],
                        "train": ds("train"), "val": ds("val")},
           "model": nets.tiny_indi_section()}
    p = tmp_path / "tiny.json"
    p.write_text(json.dumps(cfg, indent=2))
    return cfg, str(p)


def _main(args):
    """split.main with torch's generators reset: the model's random initial weights and the sampler's noise seeds come
    from them, so equal arguments give equal predictions."""
    from diffsplitting_amd import split
    torch.manual_seed(1234)
    return split.main(args)


def _nd_equal(x, y):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in x) and set(x) == set(y)


def test_get_datasets_normalises_with_the_training_stack(tmp_path):
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset, SplitDatasetTiledPred
    from diffsplitting_amd.split import get_datasets
    from diffsplitting_amd._lib import DsxError
    cfg, _ = _config(tmp_path)
    opt = dict_to_nonedict(cfg)
    val_loc = DataLocation(channelwise_fpath=(cfg["datasets"]["val"]["datapath"]["ch0"], cfg["datasets"]["val"]["datapath"]["ch1"]))
    own = SplitDataset("Hagen", val_loc, 64, max_qval=0.98, channel_weights=[1, 1]).get_normalization_dict()
    train_set, val_set = get_datasets(opt)
    assert type(val_set) is SplitDataset and type(train_set) is SplitDataset
    assert _nd_equal(val_set.get_normalization_dict(), train_set.get_normalization_dict())
    assert not _nd_equal(val_set.get_normalization_dict(), own)
    assert train_set.get_normalization_dict()["target0_max"] > 2 * own["target0_max"]
    none, val_own = get_datasets(opt, norm_from="val")
    assert none is None and _nd_equal(val_own.get_normalization_dict(), own)
    _, tiled = get_datasets(opt, tiled_pred=True)
    assert type(tiled) is SplitDatasetTiledPred and _nd_equal(tiled.get_normalization_dict(), train_set.get_normalization_dict())
    assert tuple(tiled.plan.data_shape) == (2, 96, 160) and tuple(tiled.plan.grid_shape) == (1, 32, 32)
    assert len(tiled) == tiled.plan.total == 2 * 2 * 4               # ShiftBoundary: ceil((D - 32) / 32) per axis
    canvas = tiled.plan.stitch(tiled.tiles(range(len(tiled)))["target"])
    assert canvas.shape == (2, 96, 160, 2) and torch.equal(canvas, tiled.normalized_target_frames())
    bad = json.loads(json.dumps(cfg))
    bad["datasets"]["train"]["name"] = "cifar10"
    with pytest.raises(DsxError, match="cifar10"):
        get_datasets(dict_to_nonedict(bad))


def test_split_main_from_datapath_to_hyperstack(tmp_path):
    from PIL import Image
    from diffsplitting_amd import split
    from diffsplitting_amd.core.logger import dict_to_nonedict
    cfg, cfg_path = _config(tmp_path, val_shape=(2, 128, 128))
    base = ["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--steps", "2", "--batch-tiles", "4"]
    out_tif, out_npy = str(tmp_path / "pred.tif"), str(tmp_path / "pred.npy")
    pred = _main(base + ["--datapath", "--out", out_tif])
    assert pred.shape == (2, 128, 128, 2) and torch.isfinite(pred).all()
    train_set, _ = split.get_datasets(dict_to_nonedict(cfg))
    nd = train_set.get_normalization_dict()
    mean = torch.as_tensor(np.asarray(nd["mean_target"]).reshape(-1), dtype=torch.float32, device=pred.device)
    std = torch.as_tensor(np.asarray(nd["std_target"]).reshape(-1), dtype=torch.float32, device=pred.device)
    raw = (pred * std + mean).cpu().numpy()                           # raw counts, normalised with the TRAIN statistics
    with Image.open(out_tif) as im:
        assert im.n_frames == 4
        assert im.tag_v2[270] == "ImageJ=1.11a\nimages=4\nchannels=2\nframes=2\nhyperstack=true\nmode=grayscale\n"
        for n in range(2):
            for c in range(2):
                im.seek(n * 2 + c)                                    # frame-major, channel-minor
                page = np.array(im)
                assert page.dtype == np.float32 and np.array_equal(page, raw[n, :, :, c]), (n, c)
    pred2 = _main(base + ["--datapath", "--out", out_npy])
    assert torch.equal(pred2, pred)
    saved = np.load(out_npy)
    assert saved.dtype == np.float32 and saved.shape == (2, 128, 128, 2) and np.array_equal(saved, raw)
    # --norm-from val: other statistics, hence another input and another prediction
    pred_val = _main(base + ["--datapath", "--norm-from", "val"])
    assert pred_val.shape == pred.shape and not torch.equal(pred_val, pred)
    # --frames accepts the (N,H,W,2) .tif as it accepts the .npy
    both = np.stack([_stack(5, 600, (2, 128, 128)), _stack(6, 300, (2, 128, 128))], axis=-1)
    TF.struct_tiff(str(tmp_path / "both.tif"), list(both))
    np.save(tmp_path / "both.npy", both)
    p_tif = _main(base + ["--frames", str(tmp_path / "both.tif")])
    p_npy = _main(base + ["--frames", str(tmp_path / "both.npy")])
    assert torch.equal(p_tif, p_npy) and torch.equal(p_tif, pred_val)  # the same val frames with their own statistics


def test_synthetic_default_is_untouched(tmp_path):
    """Without the new flags the entry point does what it did: synthetic frames, the arrays path, the same canvas as
    the dataset built by hand from those frames."""
    _, cfg_path = _config(tmp_path)
    args = ["-c", cfg_path, "-p", "val", "-gpu", "0", "-rootdir", str(tmp_path), "--synthetic", "2,128,128", "--steps", "2",
            "--batch-tiles", "4"]
    one, two = _main(args), _main(args)
    assert one.shape == (2, 128, 128, 2) and torch.isfinite(one).all() and torch.equal(one, two)
    assert not os.path.exists(tmp_path / "pred.tif")
