"""predict_stack across ranks (`-m gpu`): the sharded prediction of an input-only stack, mean and spread over two
posterior samples, equals the one-rank result bitwise on every rank, on the hardware that is there (fresh ranks sharing
the one GPU, gloo transport)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 3])
def test_input_stack_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout): a uint16 stack (3, 96, 160), patch 64, grid 32 -> 24
    tiles, batch_tiles 4 (every batch full for worlds 1, 2, 3), 2 steps, 2 samples, seed 11.  On every rank the mean and
    the spread canvas equal the one-rank result, bitwise (the worker checks both: tests/multi_rank_predict_input.py)."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom diffsplitting_amd import parallel\n"
            "sys.exit(parallel.self_launch(%d, [%r], timeout=300))\n"
            % (ROOT, world, os.path.join(ROOT, "tests", "multi_rank_predict_input.py")))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["DSX_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "PREDICT_INPUT_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
