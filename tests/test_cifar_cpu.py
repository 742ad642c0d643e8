"""The CIFAR data path without a GPU: the pickle loader against the class stacks the reference's loader wrote
(tests/golden/cifar_items.npz, tools/gen_cifar_golden.py), its refusals, SplitDataset('cifar10') on the host (length,
patch locations, normalisation dict), the refusals that concern colour frames, get_datasets on a cifar10 config and the
reference's import path."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import cifar_files as CF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset(directory, patch, **kw):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    return SplitDataset("cifar10", DataLocation(directory=directory), patch, max_qval=1.0, device="cpu", **kw)


def _colour_arrays(cc=3, n=2, hw=(8, 8)):
    rng = np.random.default_rng(cc)
    return tuple(rng.integers(0, 256, size=(n, cc) + hw, dtype=np.uint8) for _ in range(2))


# ----------------------------------------------------------------------------- the loader
def test_loader_equals_the_reference_on_one_file_directories(tmp_path):
    from diffsplitting_amd.data import cifar10
    g = CF.fixture()
    for name in CF.names():
        d = CF.write_dir(tmp_path / name, [name])
        imgs, labels = cifar10.load_cifar10_data(os.path.join(d, name))
        assert imgs.dtype == np.uint8 and imgs.shape == (len(labels), 3, 32, 32)
        assert np.array_equal(imgs.reshape(len(labels), -1), g[f"{name}_data"]) and list(labels) == list(g[f"{name}_labels"])
        got = cifar10.load_train_val_data(d, [1, 7])
        assert sorted(got) == [0, 1]
        for c in (0, 1):
            assert got[c].dtype == np.uint8 and np.array_equal(got[c], g[f"{name}_class{c}"]), (name, c)
    assert cifar10.testing_files() == ["test_batch"]
    assert isinstance(cifar10.unpickle(os.path.join(d, name)), dict)


def test_a_directory_is_read_in_sorted_name_order(tmp_path):
    from diffsplitting_amd.data import cifar10
    g = CF.fixture()
    two = ["test_batch", "data_batch_2"]                              # written in the other order
    d = CF.write_dir(tmp_path / "two", two)
    assert cifar10.training_files(d) == sorted(two)
    got = cifar10.load_train_val_data(d, [1, 7])
    for c in (0, 1):
        assert np.array_equal(got[c], np.concatenate([g[f"{n}_class{c}"] for n in sorted(two)]))
    swapped = cifar10.load_train_val_data(d, [7, 1])                  # the label list is the caller's
    assert np.array_equal(swapped[0], got[1]) and np.array_equal(swapped[1], got[0])


def test_bad_files_are_refused_by_name(tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import cifar10
    g = CF.fixture()
    data, labels = g["test_batch_data"], g["test_batch_labels"]

    def directory(tag, write):
        d = tmp_path / tag
        CF.write_dir(d, ["data_batch_1"])
        write(str(d / "zz_bad"))
        return str(d)

    def dump(obj):
        return lambda p: pickle.dump(obj, open(p, "wb"), protocol=2)

    cases = {
        "text": (lambda p: open(p, "w").write("not a pickle\n"), "not a pickle"),
        "truncated": (lambda p: open(p, "wb").write(pickle.dumps({b"data": data, b"labels": list(labels)}, protocol=2)[:100]),
                      "not a pickle"),
        "subdir": (lambda p: os.makedirs(p), "not a pickle"),
        "list": (dump([1, 2, 3]), "b'data' and b'labels'"),
        "nodata": (dump({b"labels": [1, 7]}), "b'data' and b'labels'"),
        "nolabels": (dump({b"data": data}), "b'data' and b'labels'"),
        "rowlen": (dump({b"data": data[:, :3071], b"labels": [int(x) for x in labels]}), "3072"),
        "dtype": (dump({b"data": data.astype(np.int16), b"labels": [int(x) for x in labels]}), "uint8"),
        "count": (dump({b"data": data, b"labels": [int(x) for x in labels][:-1]}), "labels for"),
    }
    for tag, (write, what) in cases.items():
        with pytest.raises(DsxError, match="zz_bad") as e:
            cifar10.load_train_val_data(directory(tag, write), [1, 7])
        assert what in str(e.value), (tag, str(e.value))
    d = tmp_path / "nohorse"
    os.makedirs(d)
    keep = labels != 7
    CF.write_batch(str(d / "b"), data[keep], labels[keep])
    with pytest.raises(DsxError, match="no image of label 7"):
        cifar10.load_train_val_data(str(d), [1, 7])
    os.makedirs(tmp_path / "empty")
    with pytest.raises(DsxError, match="holds no file"):
        cifar10.load_train_val_data(str(tmp_path / "empty"), [1, 7])
    with pytest.raises(DsxError, match="not a directory"):
        cifar10.load_train_val_data(str(tmp_path / "missing"), [1, 7])


# ----------------------------------------------------------------------------- the dataset on the host
def test_dataset_length_locations_and_normalisation_dict(tmp_path):
    g = CF.fixture()
    d = CF.write_dir(tmp_path / "all")
    for wname, w in (("w11", [1, 1]), ("w103", [1, 0.3])):
        for p in (32, 16):
            ds = _dataset(d, p, channel_weights=w)
            assert ds._frameN == int(g["frame_n"]) == 13 and len(ds) == int(g[f"len_p{p}"])
            assert ds._planes == 3 and ds._data_shape == (13, 3, 32, 32)
            tag = f"p{p}_{wname}"
            assert [tuple(int(v) for v in ds.patch_location(int(i))) for i in g[f"{tag}_indices"]] == \
                [tuple(r) for r in g[f"{tag}_locations"].tolist()]
            nd, want = ds.get_normalization_dict(), CF.normalization_dict(f"nd_{wname}")
            assert set(nd) == set(want)
            for k in want:
                assert np.array_equal(np.asarray(nd[k], dtype=np.float64).reshape(-1), want[k].reshape(-1)), (tag, k)
            assert isinstance(nd["mean_input"], np.float64) and nd["mean_target"].shape == (6, 1, 1)
    # the class stacks on the host side are the loader's, cut to min(n0, n1)
    car = np.concatenate([g[f"{n}_class0"] for n in CF.names()])[:13]
    assert np.array_equal(ds._dev[0].numpy(), car.astype(np.float32))
    # a caller-supplied dict is kept as given
    ds = _dataset(d, 32, normalization_dict=CF.normalization_dict("custom_nd"))
    assert np.array_equal(ds.get_normalization_dict()["std_target"].reshape(-1), g["custom_nd_std_target"])


def test_arrays_with_colour_planes():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDataset
    a, b = _colour_arrays(cc=5, n=3)
    ds = SplitDataset("cifar10", DataLocation(arrays=(a, b[:2])), 4, device="cpu")
    assert ds._planes == 5 and len(ds) == 2 * 4 and ds.get_normalization_dict()["mean_target"].shape == (10, 1, 1)
    with pytest.raises(DsxError, match="1..8"):
        SplitDataset("cifar10", DataLocation(arrays=_colour_arrays(cc=9)), 4, device="cpu")
    with pytest.raises(DsxError, match="one shape"):
        SplitDataset("cifar10", DataLocation(arrays=(a, b[:, :3])), 4, device="cpu")
    with pytest.raises(DsxError, match="10 mean_target"):            # a grey dict on colour frames
        SplitDataset("cifar10", DataLocation(arrays=(a, b)), 4, device="cpu",
                     normalization_dict={"mean_input": 1.0, "std_input": 1.0, "mean_target": np.ones(2), "std_target": np.ones(2)})
    with pytest.raises(DsxError, match="directory"):
        SplitDataset("cifar10", DataLocation(fpath="frames.tif"), 4, device="cpu")


# ----------------------------------------------------------------------------- refusals (nothing touches the GPU)
def test_refusals_on_colour_frames(tmp_path, monkeypatch):
    from diffsplitting_amd import _lib
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.data import split_dataset as SD
    from diffsplitting_amd.data.split_dataset_tiledpred import SplitDatasetTiledPred
    from diffsplitting_amd.data.time_predictor_dataset import TimePredictorDataset

    def no_gpu(*a, **k):
        raise AssertionError("the refusal must come before anything touches the GPU")

    monkeypatch.setattr(SD, "frames_to_device", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    loc = SD.DataLocation(arrays=_colour_arrays())
    d = CF.write_dir(tmp_path / "all")
    for location in (loc, SD.DataLocation(directory=d)):
        with pytest.raises(DsxError, match="input_from_normalized_target.*FIRST image"):
            SD.SplitDataset("cifar10", location, 8, input_from_normalized_target=True)
        with pytest.raises(DsxError, match="SplitDatasetTiledPred.*three-dimensional"):
            SplitDatasetTiledPred("cifar10", location, 8, grid_size=4)
        with pytest.raises(DsxError, match="TimePredictorDataset.*grey"):
            TimePredictorDataset("cifar10", location, 8)
    with pytest.raises(DsxError, match="albumentations"):            # as before
        SD.SplitDataset("cifar10", loc, 8, enable_transforms=True)
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    ds = SD.SplitDataset("cifar10", loc, 8, device="cpu")
    table = {t: [-1.0, 1.0] for t in range(3)}
    with pytest.raises(DsxError, match="mixed_tiles on frames with colour planes"):
        ds.mixed_tiles([0], 0.5, table)
    with pytest.raises(DsxError, match="mixed_tiles_at on frames with colour planes"):
        ds.mixed_tiles_at([(0, 0, 0)], 0.5)
    unc = SD.SplitDataset("cifar10", loc, 8, device="cpu", uncorrelated_channels=True)
    with pytest.raises(DsxError, match="uncorrelated_channels"):     # as before
        unc.tiles([0])


# ----------------------------------------------------------------------------- get_datasets
def test_get_datasets_on_a_cifar_config(tmp_path):
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.split_dataset import SplitDataset
    from diffsplitting_amd.split import get_datasets
    import json
    g = CF.fixture()
    cfg, _ = CF.config(tmp_path)
    train_set, val_set = get_datasets(dict_to_nonedict(cfg), device="cpu")
    assert type(train_set) is SplitDataset and type(val_set) is SplitDataset
    assert train_set._frameN == 5 and train_set._uncorrelated_channels           # data_batch_1 alone: 8 cars, 5 horses
    assert val_set._frameN == 13 and len(val_set) == 13 and val_set._planes == 3 and not val_set._uncorrelated_channels
    want = CF.normalization_dict("nd_w11")
    for k, v in val_set.get_normalization_dict().items():
        assert np.array_equal(np.asarray(v, dtype=np.float64).reshape(-1), want[k].reshape(-1)), k
    assert np.array_equal(val_set._dev[1].numpy(), np.concatenate([g[f"{n}_class1"] for n in CF.names()]).astype(np.float32))
    none, val_own = get_datasets(dict_to_nonedict(cfg), norm_from="val", device="cpu")
    assert none is None
    for k, v in val_own.get_normalization_dict().items():            # uint8 data: the same numbers from either set
        assert np.array_equal(np.asarray(v, dtype=np.float64).reshape(-1), want[k].reshape(-1)), k
    with pytest.raises(DsxError, match="three-dimensional"):
        get_datasets(dict_to_nonedict(cfg), tiled_pred=True, device="cpu")
    gone = json.loads(json.dumps(cfg))
    gone["datasets"]["train"]["datapath"] = str(tmp_path / "no_such_dir")
    with pytest.raises(DsxError, match="no_such_dir.*--norm-from val"):
        get_datasets(dict_to_nonedict(gone), device="cpu")
    assert get_datasets(dict_to_nonedict(gone), norm_from="val", device="cpu")[1]._frameN == 13
    gone["datasets"]["val"]["datapath"] = {"ch0": "a.tif", "ch1": "b.tif"}
    with pytest.raises(DsxError, match="cifar10.*datasets.val.datapath"):
        get_datasets(dict_to_nonedict(gone), norm_from="val", device="cpu")
    joint = json.loads(json.dumps(cfg))
    joint["model"]["which_model_G"] = "joint_indi"
    with pytest.raises(DsxError, match="input_from_normalized_target"):
        get_datasets(dict_to_nonedict(joint), device="cpu")


def test_new_entry_point_is_declared_and_the_abi_version_stays():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    assert "dsx_tiles_gather_norm_planes" in _lib.SIGNATURES and "int dsx_tiles_gather_norm_planes(" in header
    assert "#define DSX_ABI_VERSION 2" in header and _lib.lib.dsx_abi_version() == 2


def test_reference_import_path(tmp_path):
    """``from data.cifar10 import load_train_val_data`` (the reference's data/split_dataset.py:8) with
    diffsplitting_amd/compat on PYTHONPATH, from a working directory outside the repository."""
    d = CF.write_dir(tmp_path / "one", ["test_batch"])
    code = ("from data.cifar10 import load_train_val_data, unpickle, load_cifar10_data, training_files, testing_files\n"
            "import sys, diffsplitting_amd.data.cifar10 as real\n"
            "assert load_train_val_data is real.load_train_val_data\n"
            "got = load_train_val_data(sys.argv[1], [1, 7])\n"
            "print('compat ok', got[0].shape, got[1].shape)\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "diffsplitting_amd", "compat"), ROOT])
    r = subprocess.run([sys.executable, "-c", code, d], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compat ok (7, 3, 32, 32) (3, 3, 32, 32)" in r.stdout, r.stderr[-2000:]
