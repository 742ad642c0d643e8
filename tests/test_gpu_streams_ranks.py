"""Per-sample noise streams across ranks (`-m gpu`): the sharded tiled prediction with real noise (e = 0.01) equals the
one-rank prediction bitwise, on the hardware that is there (fresh ranks sharing the one GPU, gloo transport)."""
import pytest

from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3])
def test_seeded_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout): frames (3, 96, 160), patch 64, grid 32 -> 24 tiles,
    batch_tiles 4 (every batch full for worlds 1, 2, 3), 2 steps, seed 11.  On every rank the stitched prediction equals
    the one-rank prediction with the batches in reversed order, bitwise; without the seed it does not (the worker checks
    both: tests/multi_rank_predict_seeded.py)."""
    r = run_ranks("multi_rank_predict_seeded.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_SEEDED_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
