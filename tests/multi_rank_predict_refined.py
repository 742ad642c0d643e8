"""Child program of test_refined_prediction_does_not_depend_on_the_sharding (tests/test_gpu_refine.py), one process per
rank: every rank runs predict_tiled_refined (one refinement round, per-sample noise streams, two MMSE repeats) on its
shard of the tiles -- the per-round table is completed by one all-gather, the canvas is exchanged --; then the same rank
runs all tiles alone (world-size-1 semantics, no collective) and compares canvas, PSNR, start times and the whole
report, bitwise.  A tile's noise depends on (seed, tile, round, repeat) only and a plane's moments on the plane only, so
nothing depends on the sharding."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from diffsplitting_amd import parallel
    from diffsplitting_amd.data.tiled_predict import predict_tiled_refined
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    from tests.bits import same_bits
    from tests.mixed_util import dataset, networks
    from tests.rank_worker import finish, start
    rank, world = start()
    i1, i2, tp, _, _ = networks(1)
    ds, _, _ = dataset((2, 64, 64), 5)                              # patch 32, grid 16: 18 tiles
    total = len(ds)
    netG = types.SimpleNamespace(indi1=i1, indi2=i2, noise_source=None,
                                 second_ids=lambda ids: [int(v) | (1 << 39) for v in ids])
    table = compute_input_normalization_dict(ds._data_dict, 100, ds._mean_target, ds._std_target)

    def run():                                                       # batches of 3: full for 1, 2 and 3 ranks
        return predict_tiled_refined(netG, tp, ds, 0.29, num_timesteps=1, mmse_count=2, batch_tiles=3, rounds=1,
                                     scope="frame", table=table, seed=11)

    (canvas, psnr), pred_t, rep = run()
    saved = parallel.rank, parallel.world_size
    parallel.rank, parallel.world_size = (lambda: 0), (lambda: 1)
    try:
        (canvas1, psnr1), pred_t1, rep1 = run()
    finally:
        parallel.rank, parallel.world_size = saved
    checks = {"canvas": same_bits(canvas, canvas1),
              "psnr": torch.equal(psnr, psnr1), "pred_t": torch.equal(pred_t, pred_t1),
              "complete": bool(torch.isfinite(pred_t).all()), "rounds": len(rep["rounds"]) == len(rep1["rounds"]) == 2}
    for q, (a, b) in enumerate(zip(rep["rounds"], rep1["rounds"])):
        for key in ("start", "moments", "curves", "t_star", "chosen", "mean_curves"):
            checks[f"round {q} {key}"] = same_bits(np.asarray(a[key]), np.asarray(b[key]))
    checks["round 1 differs from round 0"] = not same_bits(rep["rounds"][0]["moments"], rep["rounds"][1]["moments"])
    ok = world in (2, 3) and total % (3 * world) == 0 and all(checks.values())
    finish(ok, "PREDICT_REFINED", total, world, detail=checks)


if __name__ == "__main__":
    main()
