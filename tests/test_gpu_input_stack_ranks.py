"""predict_stack across ranks (`-m gpu`): the sharded prediction of an input-only stack, mean and spread over two
posterior samples, equals the one-rank result bitwise on every rank, on the hardware that is there (fresh ranks sharing
the one GPU, gloo transport)."""
import pytest

from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3])
def test_input_stack_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout): a uint16 stack (3, 96, 160), patch 64, grid 32 -> 24
    tiles, batch_tiles 4 (every batch full for worlds 1, 2, 3), 2 steps, 2 samples, seed 11.  On every rank the mean and
    the spread canvas equal the one-rank result, bitwise (the worker checks both: tests/multi_rank_predict_input.py)."""
    r = run_ranks("multi_rank_predict_input.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_INPUT_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
