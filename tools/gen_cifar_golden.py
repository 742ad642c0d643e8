"""Writes tests/golden/cifar_items.npz with the REFERENCE's own code: ``data.cifar10.load_train_val_data`` and
``data.split_dataset.SplitDataset('cifar10', ...)`` on three small synthetic CIFAR-format batch files.

    python tools/gen_cifar_golden.py /path/to/reference/checkout

The reference module imports ``albumentations`` and ``skimage.io`` at module level and calls neither with
``enable_transforms=False``: empty stand-in modules of those names let it import where they are not installed
(as tools/gen_mix_range_golden.py does).  The batch files are pickled into a temporary directory from the arrays the
fixture stores; no pickle is committed.  The reference lists a directory in ``os.listdir`` order, which is arbitrary;
for the three-file directory its ``training_files`` is replaced by the sorted listing, the one stated departure of
diffsplitting_amd/data/cifar10.py, so that the items pair the same images everywhere.  The per-file class stacks come
from one-file directories and do not depend on any order.  Only inputs and outputs are stored; nothing of the
reference is copied.  The fixture records the numpy version.
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("data_batch_1", "data_batch_2", "test_batch")
COUNTS = (24, 22, 18)                                                # 64 images in all
WEIGHTS = {"w11": [1, 1], "w103": [1, 0.3]}
CUSTOM = {"mean_input": np.float64(171.25), "std_input": np.float64(93.5),
          "mean_target": np.array([101.0, 117.5, 130.25, 99.0, 140.75, 122.125]),
          "std_target": np.array([61.0, 57.5, 70.25, 66.0, 52.75, 63.125]),
          "target0_max": 255, "target1_max": 255, "input_max": 331.5}


def batches():
    """name -> (data (n, 3072) uint8, labels list).  Coarse 8 x 8 colour blocks (the file stays small) with one fully
    random image per class; labels 1 and 7 occur unequally, every other label occurs; both classes hold 0 and 255."""
    rng = np.random.default_rng(1007)
    out = {}
    for name, n in zip(FILES, COUNTS):
        coarse = rng.integers(0, 256, size=(n, 3, 8, 8), dtype=np.uint8)
        imgs = np.kron(coarse, np.ones((4, 4), dtype=np.uint8))
        speck = rng.random(imgs.shape) < 0.05
        imgs[speck] = rng.integers(0, 256, size=int(speck.sum()), dtype=np.uint8)
        labels = rng.permutation(np.resize(np.array([1, 1, 1, 7, 7, 0, 2, 3, 1, 4, 5, 7, 6, 8, 9, 1]), n))
        out[name] = [imgs, labels]
    imgs, labels = out[FILES[0]]
    i1, i7 = np.where(labels == 1)[0], np.where(labels == 7)[0]
    imgs[i1[0]] = rng.integers(0, 256, size=(3, 32, 32), dtype=np.uint8)
    imgs[i7[0]] = rng.integers(0, 256, size=(3, 32, 32), dtype=np.uint8)
    imgs[i1[0], 0, 0, 0], imgs[i1[0], 2, 31, 31] = 0, 255           # the extremes on the first and the last pixel
    imgs[i7[0], 0, 0, 0], imgs[i7[0], 2, 31, 31] = 255, 0
    return {k: (v[0].reshape(len(v[0]), -1), [int(x) for x in v[1]]) for k, v in out.items()}


def write_batches(directory, names, data):
    os.makedirs(directory, exist_ok=True)
    for name in names:
        with open(os.path.join(directory, name), "wb") as f:
            pickle.dump({b"batch_label": name.encode(), b"labels": data[name][1], b"data": data[name][0],
                         b"filenames": [b"%d.png" % i for i in range(len(data[name][1]))]}, f, protocol=2)


def main(ref):
    for name in ("albumentations", "skimage", "skimage.io"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.io"].imread = None
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    sys.path.insert(0, ref)
    import data.cifar10 as ref_c
    import data.split_dataset as ref_sd

    data = batches()
    out = {"numpy_version": np.array(np.__version__), "files": np.array(FILES)}
    with tempfile.TemporaryDirectory() as tmp:
        for name in FILES:
            out[f"{name}_data"], out[f"{name}_labels"] = data[name][0], np.array(data[name][1], dtype=np.int64)
            write_batches(os.path.join(tmp, name + "_alone"), [name], data)
            stacks = ref_c.load_train_val_data(os.path.join(tmp, name + "_alone"), [1, 7])
            out[f"{name}_class0"], out[f"{name}_class1"] = stacks[0], stacks[1]
            assert stacks[0].dtype == np.uint8 and stacks[0].shape[1:] == (3, 32, 32)
        n0 = sum(len(out[f"{n}_class0"]) for n in FILES)
        n1 = sum(len(out[f"{n}_class1"]) for n in FILES)
        assert n0 != n1 and min(n0, n1) >= 8, (n0, n1)
        for c in (0, 1):
            both = np.concatenate([out[f"{n}_class{c}"] for n in FILES])
            assert both.min() == 0 and both.max() == 255
        every = os.path.join(tmp, "all")
        write_batches(every, FILES, data)
        ref_c.training_files = lambda datadir: sorted(os.listdir(datadir))      # see the module docstring
        loc = ref_sd.DataLocation(directory=every)
        frame_n = min(n0, n1)
        out["frame_n"] = np.array(frame_n)

        def items(tag, ds, indices):
            got = [ds[i] for i in indices]
            out[f"{tag}_indices"] = np.array(indices)
            out[f"{tag}_locations"] = np.array([ds.patch_location(i) for i in indices])
            out[f"{tag}_input"] = np.stack([g["input"] for g in got])
            out[f"{tag}_target"] = np.stack([g["target"] for g in got])
            assert out[f"{tag}_input"].dtype == np.float32 and out[f"{tag}_target"].dtype == np.float32

        for wname, w in WEIGHTS.items():
            for p in (32, 16):
                ds = ref_sd.SplitDataset("cifar10", loc, p, max_qval=1.0, channel_weights=w, enable_transforms=False)
                n = len(ds)
                out[f"len_p{p}"] = np.array(n)
                nd = ds.get_normalization_dict()
                for k in ("mean_input", "std_input", "target0_max", "target1_max", "input_max"):
                    out[f"nd_{wname}_{k}"] = np.float64(nd[k])
                out[f"nd_{wname}_mean_target"] = nd["mean_target"].reshape(-1)
                out[f"nd_{wname}_std_target"] = nd["std_target"].reshape(-1)
                items(f"p{p}_{wname}", ds, [0, n - 3, 2, n - 3, n - 1] if p == 32 else [1, n - 2, 6, 11, 6, n - 1])
                if p == 32 and wname == "w11":
                    items("first8", ds, list(range(8)))              # what the driver test feeds
        ds = ref_sd.SplitDataset("cifar10", loc, 32, max_qval=1.0, channel_weights=[1, 0.3], enable_transforms=False,
                                 normalization_dict=dict(CUSTOM))
        for k, v in CUSTOM.items():
            out[f"custom_nd_{k}"] = np.asarray(v, dtype=np.float64)
        items("custom", ds, [3, frame_n - 1, 3, 0])
        ds = ref_sd.SplitDataset("cifar10", loc, 16, max_qval=1.0, target_channel_idx=4, enable_transforms=False)
        items("tci4", ds, [5, 0, 4 * frame_n - 1, 5])
        assert out["tci4_target"].shape[1:] == (1, 16, 16)
    path = os.path.join(ROOT, "tests", "golden", "cifar_items.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}, {frame_n} pairs ({n0} / {n1})")


if __name__ == "__main__":
    main(sys.argv[1])
