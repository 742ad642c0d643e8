"""Frame-keyed noise across ranks (`-m gpu`): the sharded Gaussian tiled prediction with ``noise="field"`` equals the
one-rank prediction bitwise, on the hardware that is there (fresh ranks sharing the one GPU, gloo transport)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 3])
def test_field_prediction_does_not_depend_on_the_sharding(world):
    """`world` fresh ranks (parallel.self_launch, under its timeout): frames (2, 64, 96), patch 32, grid 16 -> 30 tiles,
    batch_tiles 5 (every batch full for worlds 1, 2, 3), sr3 with ddim over 4 rows, eta = 0.5.  On every rank the
    stitched prediction equals the one-rank restatement with the batches in reversed order, bitwise; with per-tile
    streams it does not (the worker checks both: tests/multi_rank_predict_field.py)."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom diffsplitting_amd import parallel\n"
            "sys.exit(parallel.self_launch(%d, [%r], timeout=300))\n"
            % (ROOT, world, os.path.join(ROOT, "tests", "multi_rank_predict_field.py")))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["DSX_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "PREDICT_FIELD_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
