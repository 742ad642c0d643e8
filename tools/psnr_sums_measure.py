"""Times the four callers of the RangeInvariantPsnr sums (csrc/dsx_reduce.h: PsnrSums, RedRow), seeded inputs, no files:

    python tools/psnr_sums_measure.py run [label] [windows]    one JSON line: per workload the median over `windows`
                                                               (default 15) windows of 50 calls, device events, after a
                                                               warm-up window; DSX_LIB_PATH chooses the library
    python tools/psnr_sums_measure.py compare FILE             FILE holds such lines labelled "parent" and "branch" from
                                                               alternating fresh processes: prints every median, the
                                                               spread of the parent against itself (max - min of its
                                                               medians) and whether the branch's median stays within it

Workloads: `blend` = plan.blend(gt=..) and `stitch` = plan.stitch_with_psnr on frames (10, 2048, 2048), patch 512, grid
256, C = 2; `msssim` = msssim(range_invariant=True) on 20 planes of 2048 x 2048; `comoments` on 16 planes of 512 x 512."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS = 50
WORKLOADS = ("blend", "stitch", "msssim", "comoments")


def window_us(fn):
    """device time per call over one window of CALLS calls"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / CALLS


def workloads():
    from diffsplitting_amd.core.metrics import msssim
    from diffsplitting_amd.core.psnr import comoments
    from diffsplitting_amd.data.tiling import TilePlan
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    plan = TilePlan((10, 2048, 2048), (1, 256, 256), (1, 512, 512))
    plan.set_window("hann")
    tiles, gt = rn(plan.total, 2, 512, 512), rn(10, 2048, 2048, 2) * 1.5 + 0.25
    canvas = torch.empty((10, 2048, 2048, 2), device="cuda")
    yield "blend", lambda: plan.blend(tiles, gt=gt, canvas=canvas)
    yield "stitch", lambda: plan.stitch_with_psnr(tiles, gt)
    del tiles, canvas
    target = gt.permute(0, 3, 1, 2).contiguous()
    pred = 0.7 * target + 0.3 * rn(10, 2, 2048, 2048) + 0.4
    yield "msssim", lambda: msssim(pred, target, range_invariant=True)
    del pred, target, gt
    planes = [rn(16, 512, 512) for _ in range(3)]
    yield "comoments", lambda: comoments(*planes)


def run(label="", windows=15):
    torch.set_grad_enabled(False)
    out = {"label": label, "lib": os.environ.get("DSX_LIB_PATH", "in-tree"), "calls": CALLS, "windows": int(windows)}
    for name, fn in workloads():
        window_us(fn)
        out[name + "_us"] = round(float(np.median([window_us(fn) for _ in range(int(windows))])), 3)
    print(json.dumps(out), flush=True)


def compare(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    ok = True
    for name in WORKLOADS:
        med = {lab: [r[name + "_us"] for r in rows if r["label"] == lab] for lab in ("parent", "branch")}
        assert len(med["parent"]) >= 3 and len(med["branch"]) >= 3, "at least three processes of each library"
        spread = max(med["parent"]) - min(med["parent"])
        p, b = float(np.median(med["parent"])), float(np.median(med["branch"]))
        within = b <= p + spread
        ok &= within
        print(f"{name}: parent {med['parent']} us, median {p:.3f}; branch {med['branch']} us, median {b:.3f}; "
              f"parent spread {spread:.3f}; branch - parent = {b - p:+.3f} us: "
              f"{'within' if within else 'EXCEEDS'} the spread")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2]) if sys.argv[1] == "compare" else run(*sys.argv[2:]))
