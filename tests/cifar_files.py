"""CIFAR-format batch files for the tests, pickled from the arrays of tests/golden/cifar_items.npz (the fixture the
reference's own loader and dataset wrote: tools/gen_cifar_golden.py).  No pickle is committed."""
import json
import os
import pickle

import numpy as np

from tests.util import GOLDEN, load_golden

_FIXTURE = None


def fixture():
    """The fixture, loaded once and shared read-only."""
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = load_golden("cifar_items")
        for v in _FIXTURE.values():
            v.setflags(write=False)
    return _FIXTURE


def names():
    return [str(n) for n in fixture()["files"]]


def write_batch(path, data, labels):
    with open(path, "wb") as f:
        pickle.dump({b"batch_label": b"synthetic", b"labels": [int(x) for x in labels], b"data": np.asarray(data),
                     b"filenames": [b"%d.png" % i for i in range(len(labels))]}, f, protocol=2)


def write_dir(directory, which=None):
    """The fixture's batch files ``which`` (default: all three) as pickles in ``directory``; returns it as str."""
    g = fixture()
    os.makedirs(directory, exist_ok=True)
    for name in (which or names()):
        write_batch(os.path.join(str(directory), name), g[f"{name}_data"], g[f"{name}_labels"])
    return str(directory)


def normalization_dict(prefix):
    g = fixture()
    keys = ("mean_input", "std_input", "mean_target", "std_target", "target0_max", "target1_max", "input_max")
    return {k: g[f"{prefix}_{k}"] for k in keys}


def gather_planes(f0, f1, shape4, patch, loc, w, mean_inp, std_inp, mt, st, tin, ttar, count=None):
    """dsx_tiles_gather_norm_planes called directly (tensors or raw addresses) -> its status"""
    import ctypes as C
    import torch
    from diffsplitting_amd._lib import lib
    loc = np.ascontiguousarray(np.asarray(loc, dtype=np.int64).reshape(-1, 3))
    mt, st = np.ascontiguousarray(mt, dtype=np.float64), np.ascontiguousarray(st, dtype=np.float64)
    pd = C.POINTER(C.c_double)
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return lib.dsx_tiles_gather_norm_planes(ptr(f0), ptr(f1), (C.c_int64 * 4)(*shape4), (C.c_int64 * 2)(*patch),
                                            loc.ctypes.data_as(C.POINTER(C.c_int64)), None,
                                            loc.shape[0] if count is None else count, float(w[0]), float(w[1]),
                                            float(mean_inp), float(std_inp), mt.ctypes.data_as(pd), st.ctypes.data_as(pd),
                                            ptr(tin), ptr(ttar), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def numpy_items(a, b, loc, ph, pw, w, mean_inp, std_inp, mt, st):
    """The reference's item (data/split_dataset.py:248-272) in numpy: fp32 crops, the target against the (2 Cc, 1, 1)
    float64 statistics, the fp32 weighted sum against the float64 input statistics, each rounded to fp32 once."""
    tin, ttar = [], []
    for n, y, x in loc:
        p1 = a[n][..., y:y + ph, x:x + pw].astype(np.float32)
        p2 = b[n][..., y:y + ph, x:x + pw].astype(np.float32)
        target = np.concatenate([p1, p2], axis=0)
        ttar.append(((target.astype(np.float64) - mt.reshape(-1, 1, 1)) / st.reshape(-1, 1, 1)).astype(np.float32))
        mix = np.float32(w[0]) * p1 + np.float32(w[1]) * p2
        assert mix.dtype == np.float32
        tin.append(((mix.astype(np.float64) - np.float64(mean_inp)) / np.float64(std_inp)).astype(np.float32))
    return np.stack(tin), np.stack(ttar)


def model_section(which="indi"):
    """The committed model section of BASELINE's C1 (config/splitting_cifar10_indi.json); ``which='ddpm'``: the three
    settings in which config/splitting_cifar10.json differs -- the conditional DDPM, 9 input channels, n = 3."""
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        m = json.load(f)["model"]["splitting_cifar10_indi"]
    if which == "ddpm":
        m["which_model_G"] = "ddpm"
        m["unet"]["in_channel"] = 9
        m["diffusion"]["conditional"] = True
        for phase in ("train", "val"):
            m["beta_schedule"][phase]["n_timestep"] = 3
    return m


def config(tmp_path, which="indi", train_dir=None, val_dir=None):
    """A cifar10 config as the reference's (datasets section of config/splitting_cifar10*.json) on synthetic
    directories -> (dict, path)."""
    train_dir = train_dir or write_dir(tmp_path / "train", names()[:1])
    val_dir = val_dir or write_dir(tmp_path / "val")
    cfg = {"name": "splitting", "phase": "train", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"upper_clip": False, "patch_size": 32, "max_qval": 1.0,
                        "train": {"name": "cifar10", "datapath": train_dir, "datatype": "img", "batch_size": 16,
                                  "num_workers": 4, "use_shuffle": True, "uncorrelated_channels": True},
                        "val": {"name": "cifar10", "patch_size": 32, "datapath": val_dir, "datatype": "img"}},
           "model": model_section(which)}
    p = tmp_path / f"cifar_{which}.json"
    p.write_text(json.dumps(cfg, indent=2))
    return cfg, str(p)
