"""Times the TimePredictor's validation loop and classifier sweep on the MI355X at BASELINE C5's own size: patch 512,
the network of config/splitting_hagen_time_predictor.json (1 -> 1, inner 16, mults [1, 2, 4, 8], GroupNorm 16, one
ResnetBlock per level, no attention), random-init weights, synthetic uint16 frames of 2048 x 2048.

    python tools/timepred_measure.py [FRAMES=2] [BATCH=8] [RATIOS=4] [REPEATS=3]

Two paths, timed in the same process, alternating, one warm call each first:
  batched   ``validation_loss`` (one dsx_tiles_gather_mix_items launch + one batched forward per BATCH items) and
            ``evaluate_time_predictor`` (BATCH tiles per launch) over RATIOS + 1 mixing ratios
  per item  the only path before them: a loop over ``ds[i]`` (one gather launch, one copy to the host per item) with one
            forward per item; for the sweep ``mixed_tiles([i], t)`` and one forward per tile
Prints items/s (medians) as one JSON line.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = {"loss_type": "l2", "which_model_G": "UnetClassifier",
         "unet": {"in_channel": 1, "out_channel": 1, "inner_channel": 16, "norm_groups": 16,
                  "channel_multiplier": [1, 2, 4, 8], "attn_res": [], "res_blocks": 1, "dropout": 0.2}}
PATCH = 512


def main(frames=2, batch=8, ratios=4, repeats=3):
    import torch
    from diffsplitting_amd import time_prediction as TP
    from diffsplitting_amd.core.logger import dict_to_nonedict
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    from diffsplitting_amd.data.tiled_predict import evaluate_time_predictor
    from diffsplitting_amd.data.time_predictor_dataset import TimePredictorDataset, compute_input_normalization_dict
    torch.set_grad_enabled(False)
    rng = np.random.default_rng(0)
    ch = [np.minimum(rng.gamma(k, s, size=(frames, 2048, 2048)), 1993).astype(np.uint16) for k, s in ((2.0, 150.0), (3.0, 70.0))]
    torch.manual_seed(0)
    model = TP.build_time_predictor(dict_to_nonedict({"model": MODEL, "datasets": {"patch_size": PATCH}}))
    ds = TimePredictorDataset("Hagen", DataLocation(arrays=tuple(ch)), PATCH, max_qval=0.995)
    tiled = SplitDatasetTiledPred("Hagen", DataLocation(arrays=tuple(ch)), PATCH, grid_size=PATCH // 2,
                                  normalization_dict=ds.get_normalization_dict())
    gt = np.arange(0, 1.01, 1 / ratios)[:ratios + 1]
    table = compute_input_normalization_dict(tiled._data_dict, ratios, tiled._mean_target, tiled._std_target)

    def loop_batched():
        np.random.seed(1)
        return TP.validation_loss(model, ds, batch, "l2")[0]

    def loop_per_item():
        np.random.seed(1)
        losses = []
        for i0 in range(0, len(ds), batch):                           # the reference's loop with today's items
            items = [ds[i] for i in range(i0, min(i0 + batch, len(ds)))]
            pred = torch.cat([model(torch.from_numpy(x[None]).cuda()) for x, _ in items]).cpu().numpy()
            y = np.array([t for _, t in items]).astype(np.float32)
            losses.append(np.mean((pred.astype(np.float64) - y) ** 2))
        return float(np.mean(losses))

    def sweep_batched():
        return evaluate_time_predictor(tiled, model, num_timesteps=ratios, batch_tiles=batch)[1]

    def sweep_per_item():
        out = np.empty((ratios + 1, len(tiled)), dtype=np.float32)
        for k, t in enumerate(gt):
            for i in range(len(tiled)):
                cls = tiled.mixed_tiles([i], float(t), table, want=("cls",))["cls"]
                out[k, i] = model(cls[:, 1:2]).item()
        return float(np.sqrt(((out - gt.reshape(-1, 1)) ** 2).mean(axis=1).mean()))

    paths = {"loop_batched": (loop_batched, len(ds)), "loop_per_item": (loop_per_item, len(ds)),
             "sweep_batched": (sweep_batched, (ratios + 1) * len(tiled)), "sweep_per_item": (sweep_per_item, (ratios + 1) * len(tiled))}
    seconds, values = {k: [] for k in paths}, {}
    for rep in range(repeats + 1):
        for name, (fn, _) in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[name] = fn()
            torch.cuda.synchronize()
            if rep:                                                   # rep 0 warms the path up (executors, tables)
                seconds[name].append(time.perf_counter() - t0)
    med = statistics.median
    print(json.dumps({"frames": frames, "patch": PATCH, "batch": batch, "ratios": ratios + 1, "repeats": repeats,
                      "items": len(ds), "tiles": len(tiled), "device": torch.cuda.get_device_name(0),
                      **{f"{k}_items_per_s": round(n / med(seconds[k]), 2) for k, (_, n) in paths.items()},
                      **{f"{k}_s": [round(v, 4) for v in seconds[k]] for k in paths},
                      "val_loss": [values["loop_batched"], values["loop_per_item"]],
                      "rmse": [values["sweep_batched"], values["sweep_per_item"]]}))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:5]])
