"""Writes tests/golden/mix_range.npz with the REFERENCE's own code: the range tables of
``compute_input_normalization_dict`` and a few ``TimePredictorDataset`` items (data/time_predictor_dataset.py).

    python tools/gen_mix_range_golden.py /path/to/reference/checkout

The reference module imports ``albumentations`` and ``skimage.io`` at module level and calls neither on these paths:
empty stand-in modules of those names let it import where they are not installed.  ``data.split_dataset.load_data`` is
replaced by a function that returns the in-memory frames.  Only inputs and outputs are stored; nothing of the
reference is copied.  The fixture records the numpy version: under numpy 2 the items' min-max normalisation runs in
float64 (``img - np.float64(...)`` promotes), under numpy 1.x in float32; the tables are float64 either way.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_ITEMS = 7
ITEM_INDICES = [0, 3, 5, 7, 2]
TIMESTEPS = [1, 20, 100]


def frames(rng, shape, k, scale):
    return np.minimum(rng.gamma(k, scale, size=shape), 65535).astype(np.uint16)


def cases():
    """name -> (ch0, ch1) integer-valued uint16 frame stacks."""
    rng = np.random.default_rng(20241)
    a0, a1 = frames(rng, (3, 96, 80), 2.0, 120.0), frames(rng, (3, 96, 80), 3.0, 60.0)
    a0[0, 0, 0], a1[0, 0, 0] = 4000, 0                      # the extremes of both ends of the table sit on the very
    a0[-1, -1, -1], a1[-1, -1, -1] = 0, 4100                # first and the very last pixel
    b0, b1 = frames(rng, (2, 37, 53), 2.0, 200.0), frames(rng, (2, 37, 53), 2.5, 90.0)   # 3922 pixels: no block size divides
    c0, c1 = frames(rng, (2, 64, 64), 2.0, 150.0), frames(rng, (2, 64, 64), 3.0, 70.0)   # square: the dataset's grid formula
    return {"a": (a0, a1), "b": (b0, b1), "c": (c0, c1)}


def main(ref):
    for name in ("albumentations", "skimage", "skimage.io"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.io"].imread = None
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    sys.path.insert(0, ref)
    import data.split_dataset as ref_sd
    import data.time_predictor_dataset as ref_tp

    out = {"numpy_version": np.array(np.__version__), "timesteps": np.array(TIMESTEPS), "cases": np.array(sorted(cases()))}
    for name, (ch0, ch1) in cases().items():
        dd = {0: [x for x in ch0], 1: [x for x in ch1]}
        nd = ref_sd.compute_normalization_dict(dd, [1, 1], q_val=0.98)
        out[f"{name}_ch0"], out[f"{name}_ch1"] = ch0, ch1
        out[f"{name}_mean_target"], out[f"{name}_std_target"] = nd["mean_target"], nd["std_target"]
        for n in TIMESTEPS:
            tab = ref_tp.compute_input_normalization_dict(dd, n, nd["mean_target"], nd["std_target"])
            out[f"{name}_table_{n}"] = np.array([[tab[t][0], tab[t][1]] for t in range(n + 1)], dtype=np.float64)
        f32 = ref_tp.compute_input_normalization_dict({0: [x.astype(np.float32) for x in ch0], 1: [x.astype(np.float32) for x in ch1]},
                                                      20, nd["mean_target"], nd["std_target"])
        assert np.array_equal(np.array([f32[t] for t in range(21)]), out[f"{name}_table_20"])   # uint16 == float32 frames

    # dataset items: the reference class on case c, patch 32
    ch0, ch1 = cases()["c"]
    ref_sd.load_data = lambda data_type, dataloc: {0: [x for x in ch0], 1: [x for x in ch1]}
    ds = ref_tp.TimePredictorDataset("Hagen", ref_sd.DataLocation(fpath="in-memory"), 32, max_qval=0.98)
    tab = ds.input_normalization_dict
    assert np.array_equal(np.array([tab[t] for t in range(101)]), out["c_table_100"])
    nd = ds.get_normalization_dict()
    for k in ("mean_input", "std_input", "target0_max", "target1_max", "input_max"):
        out[f"ds_{k}"] = np.float64(nd[k])
    out["ds_mean_target"], out["ds_std_target"] = nd["mean_target"].reshape(-1), nd["std_target"].reshape(-1)
    np.random.seed(SEED_ITEMS)
    items = [ds[i] for i in ITEM_INDICES]
    out["item_seed"], out["item_indices"] = np.array(SEED_ITEMS), np.array(ITEM_INDICES)
    out["item_t"] = np.array([t for _, t in items], dtype=np.float64)
    out["item_inp"] = np.stack([inp for inp, _ in items])            # float64 under numpy 2, float32 under numpy 1.x
    path = os.path.join(ROOT, "tests", "golden", "mix_range.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}, items {out['item_inp'].dtype}")


if __name__ == "__main__":
    main(sys.argv[1])
