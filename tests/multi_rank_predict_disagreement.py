"""Child program of test_gpu_disagreement (one process per rank): every rank predicts its share of the tiles of a Gaussian
(sr3) tiled prediction with ``predict_stack(disagreement=True)`` (dpmpp2m over 4 rows, per-tile streams), once under crop
-- the whole tiles then take one more all-gather -- and once under blend, where the measure reads the buffer the blend
reads.  Every rank checks, bitwise, that map, rows and scores equal ``TilePlan.disagreement`` of the one-rank tiles restated
in this process (batches in REVERSED order), and that 'mean' keeps the bits of the call without the option."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 5


def main():
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from tests import tiled_util as T
    from tests.bits import same_bits
    from tests.rank_worker import finish, start
    rank, world = start()
    smp = T.sr3()
    stack = T.stack((2, 64, 96), 32, 16, seed=4)
    plan = stack.plan
    assert plan.total == 30 and plan.total % (BATCH * world) == 0    # every batch is full on every rank
    solver = T.SOLVERS["dpmpp2m"]
    tiles = {}
    for i in reversed(range(0, plan.total, BATCH)):
        chunk = list(range(i, i + BATCH))
        tiles[i] = T.run(smp, stack.tiles(chunk)["input"], solver, seed=T.SEED, sample_ids=chunk)
    want = plan.disagreement(torch.cat([tiles[i] for i in sorted(tiles)]), band=5)
    ok, detail = bool((want["count"] > 0).all() and (want["sum_var"] > 0).all()), []
    for stitch in ("crop", "blend"):
        kw = dict(batch_tiles=BATCH, solver=solver, seed=T.SEED, stitch=stitch, window="hann")
        plain, _ = predict_stack(smp, stack, **kw)
        got, _ = predict_stack(smp, stack, disagreement=True, seam_band=5, **kw)
        same = {k: same_bits(got["disagreement"][k], want[k]) for k in want}
        same["mean"] = same_bits(got["mean"], plain["mean"])
        ok = ok and all(same.values())
        detail.append(f"{stitch}: {same}")
    finish(ok, "PREDICT_DISAGREEMENT", plan.total, world, detail="; ".join(detail))


if __name__ == "__main__":
    main()
