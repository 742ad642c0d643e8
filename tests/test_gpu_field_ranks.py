"""Frame-keyed noise across ranks (`-m gpu`): the sharded Gaussian tiled prediction with ``noise="field"`` equals the
one-rank prediction bitwise, on the hardware that is there (fresh ranks sharing the one GPU, gloo transport)."""
import pytest

from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3])
def test_field_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout): frames (2, 64, 96), patch 32, grid 16 -> 30 tiles,
    batch_tiles 5 (every batch full for worlds 1, 2, 3), sr3 with ddim over 4 rows, eta = 0.5.  On every rank the
    stitched prediction equals the one-rank restatement with the batches in reversed order, bitwise; with per-tile
    streams it does not (the worker checks both: tests/multi_rank_predict_field.py)."""
    r = run_ranks("multi_rank_predict_field.py", world, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_FIELD_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
