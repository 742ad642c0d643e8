"""``_batches`` + ``store_kept``: every batch of a shard has one size (one executor), the short last one is moved back over
the batch before it, and the kept tail of every batch fills the resident buffer slot by slot, each slot once."""
import math

import pytest
import torch

from diffsplitting_amd.data.tiled_predict import _batches, store_kept

CASES = [(total, world, rank, batch) for total in range(1, 14) for world in range(1, 4) for rank in range(world)
         for batch in range(1, 7) if len(range(rank, total, world))]


def test_the_cases_are_all_of_them():
    assert len(CASES) == 444


@pytest.mark.parametrize("as_list", (False, True), ids=("range", "list"))
def test_every_slot_holds_its_tile_and_is_written_once(as_list):
    for total, world, rank, batch in CASES:
        shard = range(rank, total, world)
        ids = list(shard) if as_list else shard
        buf = torch.full((len(shard),), math.nan)
        writes = torch.zeros(len(shard), dtype=torch.int64)
        sizes = set()
        for chunk, keep in _batches(ids, batch):
            sizes.add(len(chunk))
            one = torch.full_like(buf, math.nan)                      # what this batch alone writes
            store_kept(one, torch.tensor(list(chunk), dtype=torch.float32), chunk, keep, world)
            writes += ~one.isnan()
            store_kept(buf, torch.tensor(list(chunk), dtype=torch.float32), chunk, keep, world)
        case = (total, world, rank, batch)
        assert buf.tolist() == [float(k) for k in shard], case
        assert writes.tolist() == [1] * len(shard), case
        assert len(sizes) == 1, case
