"""The rank harness of the sharding tests, in two halves.

A parent test calls ``run_ranks``: a fresh ``python -c`` child that calls ``parallel.self_launch``, which starts the
ranks as fresh children of its own -- no process that has initialised the GPU replaces its program.  A worker program
(tests/multi_*.py) puts the repository root on ``sys.path``, opens with ``rank, world = start()`` and closes with
``finish(ok, token, ...)``."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER_VARS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")


def run_ranks(script_name, world, backend=None, launch_timeout=None, timeout=600):
    """``world`` ranks of tests/``script_name`` (or of an absolute path) under ``parallel.self_launch`` with
    ``launch_timeout``, the launcher's variables scrubbed from the environment, DSX_DIST_BACKEND set only when a
    ``backend`` is given; the CompletedProcess of the launching child (rank 0's stdout, every rank's stderr)."""
    limit = "" if launch_timeout is None else ", timeout=%d" % launch_timeout
    code = ("import sys; sys.path.insert(0, %r)\nfrom diffsplitting_amd import parallel\n"
            "sys.exit(parallel.self_launch(%d, [%r]%s))\n" % (ROOT, world, os.path.join(ROOT, "tests", script_name), limit))
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER_VARS}
    if backend is not None:
        env["DSX_DIST_BACKEND"] = backend
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)


def start():
    """A rank's opening: no autograd in this process, the process group (which sets the rank's device); (rank, world)."""
    import torch
    from diffsplitting_amd import parallel
    torch.set_grad_enabled(False)
    return parallel.init(os.environ.get("DSX_DIST_BACKEND") or "nccl")


def finish(ok, token, *info, detail=None):
    """A rank's closing: a failing rank prints ``detail`` to stderr, the flags are reduced with MIN, rank 0 prints
    ``<token>_OK`` or ``<token>_MISMATCH`` followed by ``info``, barrier, the group is destroyed, exit 0 only if every
    rank was ok."""
    import torch
    import torch.distributed as dist
    if not ok and detail is not None:
        print(f"[rank {dist.get_rank()}] {detail}", file=sys.stderr)
    flag = torch.tensor([1 if ok else 0], device="cuda" if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if dist.get_rank() == 0:
        print(f"{token}_OK" if int(flag.item()) == 1 else f"{token}_MISMATCH", *info)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)
