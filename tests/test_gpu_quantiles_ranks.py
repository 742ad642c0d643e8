"""predict_stack(quantiles=) across ranks (`-m gpu`): the sharded quantile canvases of an input-only stack equal the
one-rank result bitwise on every rank, on the hardware that is there (fresh ranks sharing the one GPU, gloo transport)."""
import pytest

from tests.rank_worker import run_ranks

pytestmark = pytest.mark.gpu


def test_quantile_canvases_do_not_depend_on_the_sharding():
    """Two fresh ranks (parallel.self_launch, under its timeout): a uint16 stack (3, 96, 160), patch 64, grid 32 -> 24
    tiles, batch_tiles 4, 2 steps, 3 samples, seed 11, quantiles (0.1, 0.5, 1.0).  On every rank the three canvases equal
    the one-rank restatement, bitwise (the worker checks them: tests/multi_rank_predict_quantiles.py)."""
    r = run_ranks("multi_rank_predict_quantiles.py", 2, backend="gloo", launch_timeout=300, timeout=400)
    assert r.returncode == 0 and "PREDICT_QUANTILES_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
