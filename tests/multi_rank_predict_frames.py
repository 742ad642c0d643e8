"""Child program of test_gpu_frames (one process per rank): every rank runs ``predict_stack_frames`` with the tiny InDI
sampler on its share of the tiles -- per row one all-gather of whole x0 tiles and one ``blend_step`` on every rank --
and then checks its frames, bitwise, against the one-rank restatement made in this process (tests/test_gpu_frames.py:
numpy cuts, ``denoise_fn`` in batches of consecutive tiles, the step on the host) -- and that the unfused blended run gives
other frames, so the comparison can fail."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 5


def main():
    from diffsplitting_amd import parallel
    from diffsplitting_amd.data.tiled_predict import predict_stack, predict_stack_frames
    from tests import test_gpu_field as T
    from tests import test_gpu_frames as F
    import torch.distributed as dist
    torch.set_grad_enabled(False)
    rank, world = parallel.init(os.environ.get("DSX_DIST_BACKEND") or "nccl")   # (sets the rank's device)
    netG = T._indi()
    stack = T._stack((2, 64, 96), 32, 16, seed=4)
    plan = stack.plan
    assert plan.total == 30 and plan.total % (BATCH * world) == 0    # every batch is full on every rank
    got, _ = predict_stack_frames(netG, stack, batch_tiles=BATCH, num_timesteps=3, seed=T.SEED, window="hann")
    batches = [(list(range(i, i + BATCH)), BATCH) for i in range(0, plan.total, BATCH)]
    want = torch.from_numpy(F._restated(netG, stack, 3, batches, window="hann"))
    same = T.same_bits(got["mean"].cpu(), want)
    unfused, _ = predict_stack(netG, stack, batch_tiles=BATCH, num_timesteps=3, seed=T.SEED, noise="field", stitch="blend",
                               window="hann")
    differs = not torch.equal(unfused["mean"].cpu(), want)
    ok = same and differs
    flag = torch.tensor([1 if ok else 0], device="cuda" if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if not ok:
        print(f"rank {rank}: frames equal {same}, unfused differs {differs}", file=sys.stderr)
    if rank == 0:
        print("PREDICT_FRAMES_OK" if int(flag.item()) == 1 else "PREDICT_FRAMES_MISMATCH", plan.total, world)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
