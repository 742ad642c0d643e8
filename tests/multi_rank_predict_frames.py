"""Child program of test_gpu_frames (one process per rank): every rank runs ``predict_stack_frames`` with the tiny InDI
sampler on its share of the tiles -- per row one all-gather of whole x0 tiles and one ``blend_step`` on every rank --
and then checks its frames, bitwise, against the one-rank restatement made in this process (tests/tiled_util.py:
numpy cuts, ``denoise_fn`` in batches of consecutive tiles, the step on the host) -- and that the unfused blended run gives
other frames, so the comparison can fail."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 5


def main():
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames
    from tests import tiled_util as T
    from tests.bits import same_bits
    from tests.rank_worker import finish, start
    rank, world = start()
    netG = T.indi()
    stack = T.stack((2, 64, 96), 32, 16, seed=4)
    plan = stack.plan
    assert plan.total == 30 and plan.total % (BATCH * world) == 0    # every batch is full on every rank
    got, _ = predict_stack_frames(netG, stack, batch_tiles=BATCH, num_timesteps=3, seed=T.SEED, window="hann")
    batches = [(list(range(i, i + BATCH)), BATCH) for i in range(0, plan.total, BATCH)]
    want = torch.from_numpy(T.restated_frames(netG, stack, 3, batches, window="hann"))
    same = same_bits(got["mean"].cpu(), want)
    unfused, _ = predict_stack(netG, stack, batch_tiles=BATCH, num_timesteps=3, seed=T.SEED, noise="field", stitch="blend",
                               window="hann")
    differs = not torch.equal(unfused["mean"].cpu(), want)
    ok = same and differs
    finish(ok, "PREDICT_FRAMES", plan.total, world,
           detail=f"frames equal {same}, unfused differs {differs}")


if __name__ == "__main__":
    main()
