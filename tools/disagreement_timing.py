"""Timing of dsx_tileplan_disagreement for DESIGN.md (seeded inputs, no files needed; it is not bench.py):

    python tools/disagreement_timing.py [repeats]

One process.  The shape is k_blend's of DESIGN item 42: (10, 2048, 2048) frames, patch 512, grid 256 -- 490 whole tiles
of C = 2, 1.03 GB -- under the triangle window.  Three calls are timed with device events, after three warm-up rounds,
`repeats` rounds (default 20) in which the three alternate, every measurement a window of INNER back-to-back calls:

    blend              dsx_tileplan_blend on the same tiles: the kernel with the same reads and a canvas of the map's size
    disagreement+map   dsx_tileplan_disagreement with the map
    disagreement       the same without the map: the rows alone

straight through the library calls on preallocated outputs (no allocation in the window).  The HBM floor at 6.3 TB/s,
the rate MI355X_MICROARCH calls achievable, is (tiles + map) bytes / 6.3e12.  One JSON line: medians, min / max, the
floors, and the ratio of each form to the blend measured in the same run."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FRAMES, PATCH, GRID, C, BAND = (10, 2048, 2048), 512, 256, 2, 8
HBM, INNER = 6.3e12, 5


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def main(argv):
    from diffsplitting_amd import _lib
    from diffsplitting_amd._lib import check, lib
    from diffsplitting_amd.data.tiling import TilePlan
    _lib.require_gpu()
    torch.set_grad_enabled(False)
    repeats = int(argv[0]) if argv else 20
    plan = TilePlan(FRAMES, (1, GRID, GRID), (1, PATCH, PATCH))
    assert plan.total == 490
    plan.set_window("triangle")
    g = torch.Generator(device="cuda").manual_seed(0)
    tiles = torch.randn(plan.total, C, PATCH, PATCH, generator=g, device="cuda")
    canvas = torch.empty(FRAMES + (C,), device="cuda")
    smap = torch.empty(FRAMES + (C,), device="cuda")
    part = torch.empty((FRAMES[0], plan.blend_blocks(), C, 8), dtype=torch.float64, device="cuda")
    h = plan.handle
    runs = {"blend": lambda: check(lib.dsx_tileplan_blend(h, tiles, C, 1, 0, canvas, None, None, None)),
            "disagreement+map": lambda: check(lib.dsx_tileplan_disagreement(h, tiles, C, 1, 0, BAND, smap, part, None)),
            "disagreement": lambda: check(lib.dsx_tileplan_disagreement(h, tiles, C, 1, 0, BAND, None, part, None))}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            ms[k].append(device_ms(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    tile_bytes, map_bytes = tiles.numel() * 4, smap.numel() * 4
    floor = {"blend": (tile_bytes + map_bytes) / HBM * 1e3, "disagreement+map": (tile_bytes + map_bytes) / HBM * 1e3,
             "disagreement": tile_bytes / HBM * 1e3}
    scores = plan.disagreement(tiles, band=BAND, want_map=False)
    row = {"what": "disagreement timing", "frames": FRAMES, "patch": PATCH, "grid": GRID, "C": C, "tiles": plan.total,
           "tile_bytes": tile_bytes, "map_bytes": map_bytes, "repeats": repeats, "calls_per_window": INNER,
           **{f"{k}_us": round(med[k] * 1e3, 1) for k in runs},
           **{f"{k}_us_min_max": [round(min(ms[k]) * 1e3, 1), round(max(ms[k]) * 1e3, 1)] for k in runs},
           **{f"{k}_floor_us": round(floor[k] * 1e3, 1) for k in runs},
           **{f"{k}_over_floor": round(med[k] / floor[k], 2) for k in runs},
           "map_over_blend": round(med["disagreement+map"] / med["blend"], 3),
           "sums_over_blend": round(med["disagreement"] / med["blend"], 3),
           "rms_pair_overlap": [round(float(v), 6) for v in scores["rms_pair"][0, :, 0].cpu()],
           "hbm_bytes_per_s": HBM}
    print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
