"""Measurements of the mixing-time scan for DESIGN.md (seeded inputs, no files needed):

    python tools/refine_measure.py kernel {tiles|canvas} [calls]   dsx_comoments alone, `calls` times (default 20) after
                                                                   two warm-up calls: run it under
                                                                   `rocprofv3 --kernel-trace --stats -- python ...` and read
                                                                   k_comoments_partial / k_comoments_finish from the stats
    python tools/refine_measure.py e2e [repeats]                   both shapes: the scoring of estimate_time_from_estimates
                                                                   (one pass + closed-form curve) against the 20-point
                                                                   torch loop of estimate_time_using_PSNR on the same
                                                                   tensors, alternating in one process after warm-up,
                                                                   device-synchronised; one JSON line per shape

Shapes: `tiles` = 16 contiguous planes of 512 x 512; `canvas` = channel 0 of a channel-last 10 x 2048 x 2048 x 2 canvas
against the two channels of another (pixel stride 2: every 64-byte line read is half used).  HBM floor: 3 * 4 * n bytes
per plane for the one pass of the shifted-data centring (the canvas shape moves twice that through the memory system)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
T_LIST = np.arange(0, 1.0, 0.05)


def inputs(shape):
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    if shape == "tiles":
        p1, p2 = 2 * rn(16, 512, 512) + 1, 0.7 * rn(16, 512, 512) - 3
        return 3 * (0.3 * p1 + 0.7 * p2 + 0.05 * rn(16, 512, 512)) + 5, p1, p2
    pred = rn(10, 2048, 2048, 2)
    pred[..., 0] = 2 * pred[..., 0] + 1
    pred[..., 1] = 0.7 * pred[..., 1] - 3
    inp = rn(10, 2048, 2048, 2)
    inp[..., 0] = 3 * (0.3 * pred[..., 0] + 0.7 * pred[..., 1] + 0.05 * inp[..., 0]) + 5
    return inp[..., 0], pred[..., 0], pred[..., 1]


def torch_loop(g, p1, p2):
    from diffsplitting_amd.core.psnr import RangeInvariantPsnr
    rows = [RangeInvariantPsnr(g, p1 * float(t) + p2 * float(1 - t)) for t in T_LIST]
    m = torch.stack(rows).cpu()
    return T_LIST[m.argmax(dim=0).numpy()], T_LIST[int(m.mean(dim=1).argmax())]


def fused(g, p1, p2):
    from diffsplitting_amd.core.psnr_based_t_refinement import estimate_time_from_estimates
    return estimate_time_from_estimates(g, p1, p2, T_LIST)[:2]


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv):
    torch.set_grad_enabled(False)
    if argv[0] == "kernel":
        from diffsplitting_amd.core.psnr import comoments
        g, p1, p2 = inputs(argv[1])
        for _ in range(2 + (int(argv[2]) if len(argv) > 2 else 20)):
            m = comoments(g, p1, p2)
        torch.cuda.synchronize()
        n = g[0].numel()
        print(json.dumps({"what": "comoments", "shape": argv[1], "planes": g.shape[0], "n": n,
                          "floor_bytes_one_pass": 12 * n * g.shape[0], "mean_Cgg": float(m[:, 6].mean())}))
        return
    repeats = int(argv[1]) if len(argv) > 1 else 7
    for shape in ("tiles", "canvas"):
        g, p1, p2 = inputs(shape)
        for _ in range(2):
            a, b = torch_loop(g, p1, p2), fused(g, p1, p2)
        tl, tf = [], []
        for _ in range(repeats):
            tl.append(timed(torch_loop, g, p1, p2)[0])
            tf.append(timed(fused, g, p1, p2)[0])
        print(json.dumps({"what": "scan_e2e", "shape": shape, "planes": g.shape[0], "n": g[0].numel(), "repeats": repeats,
                          "loop_ms": [round(1e3 * v, 3) for v in (min(tl), float(np.median(tl)), max(tl))],
                          "fused_ms": [round(1e3 * v, 3) for v in (min(tf), float(np.median(tf)), max(tf))],
                          "same_argmax": bool(np.array_equal(a[0], b[0]) and a[1] == b[1])}))


if __name__ == "__main__":
    main(sys.argv[1:])
