"""The shared test helpers themselves, without a GPU: what tests/bits.py calls bit-equal, and the environment that
tests/rank_worker.py hands to the ranks it launches."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import rank_worker
from tests.bits import bits, same_bits

TORCH_FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
NUMPY_FLOATS = [np.float16, np.float32, np.float64]


def _both_nans(dtype):
    """two NaNs of ``dtype`` that differ in one payload bit, as a pair of one-element tensors or arrays"""
    if isinstance(dtype, torch.dtype):
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[torch.empty((), dtype=dtype).element_size()]
        quiet = torch.tensor([float("nan")], dtype=dtype)
        return quiet, (quiet.view(ints) | 1).view(dtype)
    quiet = np.array([np.nan], dtype=dtype)
    return quiet, (bits(quiet) | 1).view(dtype)


@pytest.mark.parametrize("dtype", TORCH_FLOATS + NUMPY_FLOATS, ids=str)
def test_same_bits_is_about_bits(dtype):
    make = (lambda v: torch.tensor(v, dtype=dtype)) if isinstance(dtype, torch.dtype) else (lambda v: np.array(v, dtype=dtype))
    x = make([[1.5, -2.0, 0.0], [3.0, 0.25, -0.0]])
    assert same_bits(x, make([[1.5, -2.0, 0.0], [3.0, 0.25, -0.0]]))
    assert bits(x).shape == x.shape
    assert same_bits(x.T, make([[1.5, 3.0], [-2.0, 0.25], [0.0, -0.0]]))           # a view that is not contiguous
    assert not same_bits(x, make([[1.5, -2.0, 0.0], [3.0, 0.25, 0.5]]))
    # +0.0 and -0.0 compare equal as numbers and differ in the sign bit
    assert bool((make([0.0]) == make([-0.0])).all()) and not same_bits(make([0.0]), make([-0.0]))
    # a NaN is never equal as a number; the same payload is the same bits, another payload is not
    quiet, other = _both_nans(dtype)
    assert bool((quiet != quiet).all()) and bool((other != other).all())
    assert same_bits(quiet, quiet.copy() if isinstance(quiet, np.ndarray) else quiet.clone())
    assert not same_bits(quiet, other)
    # shape: the same elements in another shape, and a 0-d value against a one-element vector
    assert not same_bits(x, x.reshape(3, 2)) and not same_bits(x, x.reshape(-1))
    assert not same_bits(make(1.0), make([1.0])) and same_bits(make(1.0), make(1.0))


def test_same_bits_refuses_equal_bytes_of_another_dtype():
    f = torch.tensor([1.0, -0.0, 3.5])
    i = f.view(torch.int32)
    assert torch.equal(bits(f), bits(i)) and not same_bits(f, i) and same_bits(f.view(torch.int32), i)
    assert np.array_equal(bits(f.numpy()), bits(i.numpy())) and not same_bits(f.numpy(), i.numpy())
    assert not same_bits(np.zeros(3, np.int64), np.zeros(3, np.float64))
    assert not same_bits(torch.zeros(2, dtype=torch.float16), torch.zeros(2, dtype=torch.bfloat16))
    assert bits(f)[1].item() == struct.unpack("<i", struct.pack("<f", -0.0))[0]
    with pytest.raises(TypeError):                                                  # a tensor against an array: say which
        same_bits(f, f.numpy())


@pytest.mark.parametrize("backend", [None, "gloo"])
def test_run_ranks_scrubs_the_launcher_variables(monkeypatch, backend):
    """What run_ranks hands to the launching child: the parent's own launcher variables are gone from its environment
    (it would take itself for a rank), the backend variable is there only when asked for, the rest is passed on."""
    seen = {}
    monkeypatch.setattr(rank_worker.subprocess, "run", lambda argv, **kw: seen.update(argv=argv, **kw) or "done")
    for name in rank_worker.LAUNCHER_VARS:
        monkeypatch.setenv(name, "77")
    monkeypatch.setenv("DSX_DIST_BACKEND", "nccl")
    monkeypatch.setenv("DSX_KEPT", "1")
    timeouts = dict(launch_timeout=300) if backend else {}
    assert rank_worker.run_ranks("multi_rank_predict_field.py", 3, backend=backend, timeout=400, **timeouts) == "done"
    assert set(rank_worker.LAUNCHER_VARS) == {"WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"}
    assert not set(rank_worker.LAUNCHER_VARS) & set(seen["env"]) and seen["env"]["DSX_KEPT"] == "1"
    assert seen["env"]["DSX_DIST_BACKEND"] == (backend or "nccl")                    # not given: the caller's own stays
    worker = os.path.join(rank_worker.ROOT, "tests", "multi_rank_predict_field.py")
    assert seen["argv"][1] == "-c" and os.path.exists(worker)
    assert f"self_launch(3, [{worker!r}]{', timeout=300' if backend else ''}))" in seen["argv"][2]       # 3 ranks of that worker
    assert seen["timeout"] == 400 and seen["capture_output"] and seen["text"]
    assert all(os.environ[name] == "77" for name in rank_worker.LAUNCHER_VARS)      # the parent's own are left alone


def test_run_ranks_starts_fresh_ranks(tmp_path, monkeypatch):
    """Two ranks that only print their environment (no device, no process group): rank 0's stdout comes back, with the
    launcher's values and the backend asked for."""
    script = tmp_path / "env_child.py"
    script.write_text("import json, os\nprint('ENV ' + json.dumps({k: v for k, v in os.environ.items() if k.isupper()}))\n")
    monkeypatch.setenv("RANK", "77")
    r = rank_worker.run_ranks(str(script), 2, backend="gloo", launch_timeout=60, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("ENV ")]
    assert len(lines) == 1
    env = json.loads(lines[0][4:])
    assert (env["WORLD_SIZE"], env["RANK"], env["LOCAL_RANK"], env["DSX_DIST_BACKEND"]) == ("2", "0", "0", "gloo")
