"""Timing of dsx_sample_quantiles for DESIGN.md (seeded inputs, no files needed; it is not bench.py):

    python tools/quantiles_timing.py [repeats]

One process.  The stack is a batch of tiles as the tiled path produces it, 8 x 2 x 512 x 512 elements per sample, with
n = 4, 8, 16, 32, 64 samples.  At every n three things are timed with device events, after three warm-up rounds,
`repeats` rounds (default 20) in which the three alternate:

    quantiles        engine.sample_quantiles(stack, (0.05, 0.5, 0.95))            nq = 3, no ranks
    quantiles+rank   the same with a target                                        nq = 3 and ranks
    torch.sort       torch.sort(stack, dim=0) alone: the cheapest thing a user has without the kernel; any
                     torch.quantile costs more

against the HBM floor (n + nq [+ 2]) * count * 4 bytes at 6.3 TB/s, the rate MI355X_MICROARCH calls achievable.  The
gate is that the kernel beats torch.sort at every n; the ratio to the floor is reported.  q = 0 and q = 1 of the kernel
are compared with the first and last row of torch.sort on the way (bit for bit).  One JSON line per n, then a summary."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPE, NS, Q = (8, 2, 512, 512), (4, 8, 16, 32, 64), (0.05, 0.5, 0.95)
HBM = 6.3e12


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv):
    from diffsplitting_amd import _lib, engine
    _lib.require_gpu()
    torch.set_grad_enabled(False)
    repeats = int(argv[0]) if argv else 20
    count = int(np.prod(SHAPE))
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.randn(*SHAPE, generator=g, device="cuda")
    rows, gate = [], True
    for n in NS:
        stack = torch.randn(n, *SHAPE, generator=g, device="cuda")
        runs = {"quantiles": lambda: engine.sample_quantiles(stack, Q),
                "quantiles+rank": lambda: engine.sample_quantiles(stack, Q, target),
                "torch.sort": lambda: torch.sort(stack, dim=0)}
        for _ in range(3):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        ends, _ = engine.sample_quantiles(stack, (0.0, 1.0))
        ordered = torch.sort(stack, dim=0).values
        same = bool(torch.equal(ends[0].view(torch.int32), ordered[0].view(torch.int32)) and
                    torch.equal(ends[1].view(torch.int32), ordered[-1].view(torch.int32)))
        del ends, ordered
        ms = {k: [] for k in runs}
        for _ in range(repeats):
            for k, fn in runs.items():
                ms[k].append(device_ms(fn))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        floor = {"quantiles": (n + len(Q)) * count * 4 / HBM * 1e3, "quantiles+rank": (n + len(Q) + 2) * count * 4 / HBM * 1e3}
        row = {"n": n, "count": count, "repeats": repeats, "extremes_equal_torch_sort": same,
               **{f"{k}_ms": round(med[k], 4) for k in runs},
               **{f"{k}_ms_min_max": [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in runs},
               **{f"{k}_floor_ms": round(floor[k], 4) for k in floor},
               **{f"{k}_over_floor": round(med[k] / floor[k], 2) for k in floor},
               "sort_over_quantiles": round(med["torch.sort"] / med["quantiles"], 2),
               "sort_over_quantiles+rank": round(med["torch.sort"] / med["quantiles+rank"], 2)}
        gate = gate and same and med["quantiles"] < med["torch.sort"] and med["quantiles+rank"] < med["torch.sort"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del stack
        torch.cuda.empty_cache()
    print(json.dumps({"what": "quantiles timing", "faster_than_torch_sort_at_every_n": gate, "hbm_bytes_per_s": HBM}))
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
