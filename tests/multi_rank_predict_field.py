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
    from diffsplitting_amd import parallel
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from tests import test_gpu_field as T
    import torch.distributed as dist
    torch.set_grad_enabled(False)
    rank, world = parallel.init(os.environ.get("DSX_DIST_BACKEND") or "nccl")   # (sets the rank's device)
    smp = T._sr3()
    stack = T._stack((2, 64, 96), 32, 16, seed=4)
    plan = stack.plan
    assert plan.total == 30 and plan.total % (BATCH * world) == 0    # every batch is full on every rank
    solver = T.SOLVERS["ddim"]
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=T.SEED, noise="field")
    want = plan.stitch(T._restated_field(smp, stack, solver, BATCH))
    same = T.same_bits(got["mean"], want)
    streams, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=T.SEED)
    differs = not torch.equal(streams["mean"], want)
    ok = same and differs
    flag = torch.tensor([1 if ok else 0], device="cuda" if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if not ok:
        print(f"rank {rank}: field equal {same}, streams differ {differs}", file=sys.stderr)
    if rank == 0:
        print("PREDICT_FIELD_OK" if int(flag.item()) == 1 else "PREDICT_FIELD_MISMATCH", plan.total, world)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
