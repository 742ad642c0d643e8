"""Child program of test_gpu_field_ranks (one process per rank): every rank predicts its share of the tiles of a Gaussian
(sr3) tiled prediction with frame-keyed noise (``predict_stack(noise="field")``, ddim with eta = 0.5: a stochastic
initial state and three stochastic rows), one all-gather, every rank stitches; every rank then checks the result,
bitwise, against the one-rank prediction restated in this process through ``noise_source`` with the tile batches taken
in REVERSED order -- and that per-tile streams give another canvas, so the comparison can fail."""
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
    solver = T.SOLVERS["ddim"]
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=T.SEED, noise="field")
    want = plan.stitch(T.restated_field(smp, stack, solver, BATCH))
    same = same_bits(got["mean"], want)
    streams, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=T.SEED)
    differs = not torch.equal(streams["mean"], want)
    ok = same and differs
    finish(ok, "PREDICT_FIELD", plan.total, world,
           detail=f"field equal {same}, streams differ {differs}")


if __name__ == "__main__":
    main()
