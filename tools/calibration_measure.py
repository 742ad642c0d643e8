"""Measurements of the spread calibration for DESIGN.md (seeded inputs, no files needed):

    python tools/calibration_measure.py kernel [calls]    dsx_calibration alone, `calls` times (default 20) after two
                                                          warm-up calls: run it under
                                                          `rocprofv3 --kernel-trace --stats -- python ...` and read
                                                          k_calib_partial / k_calib_finish from the stats
    python tools/calibration_measure.py e2e [repeats]     the two-launch call against the torch sequence that computes
                                                          the same numbers on the same tensors (bucketize, a count and
                                                          two weighted bincounts, the comparisons), alternating in one
                                                          process after warm-up, device-synchronised; one JSON line

Shape: 10 x 2048 x 2048 x 2 channel-last canvases, 30 equal-count bins, z = (1, 2, 3); `smooth` as a third argument of
e2e draws a spatially smooth spread (few bins per wave) instead of white noise.  HBM floor: 3 * n * C * 4 bytes."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPE, BINS, Z = (10, 2048, 2048, 2), 30, (1.0, 2.0, 3.0)


def inputs(smooth=False):
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda: torch.randn(*SHAPE, generator=g, device="cuda")
    mean = rn()
    if smooth:
        ramp = torch.linspace(0.05, 1.0, SHAPE[2], device="cuda").view(1, 1, -1, 1)
        std = (ramp * (1 + 0.01 * rn().abs())).contiguous()
    else:
        std = rn().abs() * 0.5 + 0.01
    return mean, std, mean + 1.3 * std * rn()


def torch_sequence(mean, std, target, edges, z):
    """(C, 3 * nbins + nz) float64, the layout of dsx_calibration's output"""
    nbins = edges.shape[1] + 1
    rows = []
    for c in range(mean.shape[-1]):
        s = std[..., c].reshape(-1).double()
        e = target[..., c].reshape(-1).double() - mean[..., c].reshape(-1).double()
        b = torch.bucketize(s, edges[c], right=True)
        cnt = torch.bincount(b, minlength=nbins).double()
        sv = torch.bincount(b, weights=s * s, minlength=nbins)
        se = torch.bincount(b, weights=e * e, minlength=nbins)
        cov = torch.stack([((s >= 0) & (e.abs() <= zk * s)).sum() for zk in z]).double()
        rows.append(torch.cat([torch.stack([cnt, sv, se], dim=1).reshape(-1), cov]))
    return torch.stack(rows)


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_bytes(fn, *a):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*a)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main(argv):
    from diffsplitting_amd.core.calibration import bin_edges, calibration_sums
    torch.set_grad_enabled(False)
    mode = argv[0] if argv else "e2e"
    mean, std, target = inputs(smooth=len(argv) > 2 and argv[2] == "smooth")
    n, C = mean.numel() // SHAPE[-1], SHAPE[-1]
    t_edges, edges = timed(bin_edges, std, BINS)
    if mode == "kernel":
        for _ in range(2 + (int(argv[1]) if len(argv) > 1 else 20)):
            out = calibration_sums(mean, std, target, edges, Z)
        torch.cuda.synchronize()
        print(json.dumps({"what": "calibration", "n": n, "C": C, "floor_bytes": 12 * n * C, "count0": float(out[0, 0])}))
        return
    repeats = int(argv[1]) if len(argv) > 1 else 7
    edges_dev = torch.from_numpy(edges).cuda()
    fused = lambda: calibration_sums(mean, std, target, edges, Z)
    loop = lambda: torch_sequence(mean, std, target, edges_dev, Z)
    for _ in range(2):
        a, b = fused(), loop()
    tf, tl = [], []
    for _ in range(repeats):
        t, a2 = timed(fused)
        tf.append(t)
        t, b2 = timed(loop)
        tl.append(t)
    ints = torch.zeros(3 * BINS + len(Z), dtype=torch.bool, device="cuda")
    ints[0:3 * BINS:3] = True
    ints[3 * BINS:] = True
    rel = ((a - b).abs() / b.abs().clamp_min(1e-300))[:, ~ints].max().item()
    floor = 12 * n * C / 8e12
    med = lambda v: float(np.median(v))
    print(json.dumps({
        "what": "calibration e2e", "n": n, "C": C, "bins": BINS, "z": Z, "repeats": repeats,
        "kernel_call_ms": round(med(tf) * 1e3, 4), "kernel_call_ms_min_max": [round(min(tf) * 1e3, 4), round(max(tf) * 1e3, 4)],
        "torch_sequence_ms": round(med(tl) * 1e3, 4), "torch_ms_min_max": [round(min(tl) * 1e3, 4), round(max(tl) * 1e3, 4)],
        "torch_over_kernel": round(med(tl) / med(tf), 2), "hbm_floor_ms_at_8TBps": round(floor * 1e3, 4),
        "kernel_over_floor": round(med(tf) / floor, 2), "bin_edges_ms": round(t_edges * 1e3, 3),
        "kernel_temporaries_bytes": peak_bytes(fused), "torch_temporaries_bytes": peak_bytes(loop),
        "same_bits_run_to_run": bool(torch.equal(a.view(torch.int64), a2.view(torch.int64))),
        "torch_same_bits_run_to_run": bool(torch.equal(b.view(torch.int64), b2.view(torch.int64))),
        "integers_equal_torch": bool(torch.equal(a[:, ints], b[:, ints])), "sums_max_rel_diff_to_torch": rel}))


if __name__ == "__main__":
    main(sys.argv[1:])
