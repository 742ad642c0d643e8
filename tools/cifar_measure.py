"""Times the whole-set evaluation of a cifar10 config on the MI355X: ``split -c <C1 config> --datapath`` over a
synthetic directory of PAIRS car / horse pairs (random uint8 images in CIFAR-format batch files, random-init C1 model,
n = 20), in fp32 and bf16.

    python tools/cifar_measure.py [PAIRS=1000] [BATCH=100] [REPEATS=3]

Per dtype one warm call, then REPEATS timed ones, the dtypes alternating.  Two figures per call: the evaluation window
``split`` logs itself (items -> sampler -> report, between two device synchronisations) and the wall time of the whole
call (config, pickles, upload, model creation, evaluation).  Prints the medians as one JSON line.
"""
import json
import logging
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_directory(directory, pairs, files=2):
    rng = np.random.default_rng(0)
    os.makedirs(directory)
    per = -(-pairs // files)
    for k in range(files):
        n = 2 * min(per, pairs - k * per)
        with open(os.path.join(directory, f"data_batch_{k + 1}"), "wb") as f:
            pickle.dump({b"labels": [1, 7] * (n // 2), b"data": rng.integers(0, 256, size=(n, 3072), dtype=np.uint8)}, f,
                        protocol=2)


class _Window(logging.Handler):
    def __init__(self):
        super().__init__()
        self.seconds = []

    def emit(self, record):
        if str(record.msg).startswith("validation: %d items"):
            self.seconds.append(float(record.args[2]))


def main(pairs=1000, batch=100, repeats=3):
    import torch
    from diffsplitting_amd import split
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        model = json.load(f)["model"]["splitting_cifar10_indi"]
    window = _Window()
    logging.getLogger("base").addHandler(window)
    walls = {"f32": [], "bf16": []}
    evals = {"f32": [], "bf16": []}
    with tempfile.TemporaryDirectory() as tmp:
        val = os.path.join(tmp, "val")
        write_directory(val, pairs)
        part = {"name": "cifar10", "datapath": val, "datatype": "img"}
        cfg = {"name": "splitting", "phase": "train", "gpu_ids": [0],
               "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
               "datasets": {"upper_clip": False, "patch_size": 32, "max_qval": 1.0, "train": part, "val": part}, "model": model}
        path = os.path.join(tmp, "c1.json")
        with open(path, "w") as f:
            json.dump(cfg, f)
        argv = ["-c", path, "-p", "val", "-gpu", "0", "-rootdir", tmp, "--datapath", "--batch-tiles", str(batch)]
        for rep in range(repeats + 1):
            for dtype in ("f32", "bf16"):
                torch.manual_seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                split.main(argv + ["--dtype", dtype])
                torch.cuda.synchronize()
                if rep:                                              # rep 0 warms this dtype up
                    walls[dtype].append(time.perf_counter() - t0)
                    evals[dtype].append(window.seconds[-1])
    med = statistics.median
    print(json.dumps({"pairs": pairs, "batch": batch, "steps": model["beta_schedule"]["val"]["n_timestep"], "repeats": repeats,
                      "device": torch.cuda.get_device_name(0),
                      **{f"{d}_eval_s": round(med(evals[d]), 4) for d in evals},
                      **{f"{d}_eval_all_s": [round(v, 4) for v in evals[d]] for d in evals},
                      **{f"{d}_wall_s": round(med(walls[d]), 4) for d in walls}}))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
