"""Child program of test_two_ranks_mixed_prediction_equals_one_rank (tests/test_gpu_timepred.py), one process per rank:
every rank runs predict_tiled_mixed on its shard of the tiles (the TimePredictor chooses every tile's start time), the
canvas is exchanged and pred_t gathered; then the same rank runs all tiles alone (world-size-1 semantics, no
collective) and compares.  The noise of a tile depends on its id only, so the result does not depend on the sharding."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from diffsplitting_amd import parallel
    from diffsplitting_amd.data.tiled_predict import gather_pred_t, predict_tiled_mixed
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    from tests.mixed_util import dataset, networks
    from tests.rank_worker import finish, start
    rank, world = start()
    i1, i2, tp, _, _ = networks(1)
    ds, _, _ = dataset((2, 64, 64), 5)                              # patch 32, grid 16: 18 tiles
    total = len(ds)
    netG = types.SimpleNamespace(indi1=i1, indi2=i2, noise_source=None)
    table = compute_input_normalization_dict(ds._data_dict, 100, ds._mean_target, ds._std_target)

    def source(which, ids):
        """Per tile, in the order the sampler asks: the start draw, then the draw of the one step."""
        draws = []
        for tile in ids:
            g = torch.Generator().manual_seed(1000 * tile + which)
            draws += [torch.randn(1, 1, 32, 32, generator=g) for _ in range(2)]
        it = iter(draws)
        return lambda shape: next(it)

    def run(ids):
        i1.noise_source, i2.noise_source = source(1, ids), source(2, ids)
        return predict_tiled_mixed(netG, tp, ds, 0.29, num_timesteps=1, mmse_count=1, batch_tiles=4, table=table)

    mine = parallel.shard_ids(total, rank, world)
    (canvas, psnr), pred_t = run(mine)
    full_t = gather_pred_t(pred_t)
    # the same on this rank alone: every tile, no collective
    saved = parallel.rank, parallel.world_size
    parallel.rank, parallel.world_size = (lambda: 0), (lambda: 1)
    try:
        (canvas1, psnr1), pred_t1 = run(list(range(total)))
    finally:
        parallel.rank, parallel.world_size = saved
    others = [i for i in range(total) if i not in mine]
    checks = {"canvas": torch.equal(canvas, canvas1), "psnr": torch.equal(psnr, psnr1),
              "own rows": torch.equal(pred_t[mine], pred_t1[mine]),
              "other rows are NaN": bool(torch.isnan(pred_t[others]).all()),
              "one rank is complete": bool(torch.isfinite(pred_t1).all()),
              "gathered": bool(torch.isfinite(full_t).all()) and torch.equal(full_t, pred_t1)}
    ok = world == 2 and all(checks.values())
    finish(ok, "PREDICT_MIXED", total, world, detail=checks)


if __name__ == "__main__":
    main()
