"""Child program of test_gpu_blend (one process per rank): every rank predicts its share of the tiles of a Gaussian (sr3)
tiled prediction with ``predict_stack(stitch="blend")`` (dpmpp2m over 4 rows, per-tile streams), keeps its whole tiles
in its slot, one all-gather of the slots, every rank blends; every rank then checks the canvas, bitwise, against the
one-rank tiles restated in this process (batches in REVERSED order) under the numpy restatement of the blend -- and
that the cropped stitch gives another canvas, so the comparison can fail."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 5


def main():
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from tests import blend_ref
    from tests import tiled_util as T
    from tests.bits import same_bits
    from tests.rank_worker import finish, start
    rank, world = start()
    smp = T.sr3()
    stack = T.stack((2, 64, 96), 32, 16, seed=4)
    plan = stack.plan
    assert plan.total == 30 and plan.total % (BATCH * world) == 0    # every batch is full on every rank
    solver = T.SOLVERS["dpmpp2m"]
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=T.SEED, stitch="blend", window="hann")
    tiles = {}
    for i in reversed(range(0, plan.total, BATCH)):
        chunk = list(range(i, i + BATCH))
        tiles[i] = T.run(smp, stack.tiles(chunk)["input"], solver, seed=T.SEED, sample_ids=chunk)
    tiles = torch.cat([tiles[i] for i in sorted(tiles)])
    want = torch.from_numpy(blend_ref.blend_ref(plan, tiles.cpu().numpy(), *blend_ref.window_pair(plan, "hann")))
    same = same_bits(got["mean"].cpu(), want)
    differs = not torch.equal(plan.stitch(tiles).cpu(), want)
    ok = same and differs
    finish(ok, "PREDICT_BLEND", plan.total, world,
           detail=f"blend equal {same}, crop differs {differs}")


if __name__ == "__main__":
    main()
