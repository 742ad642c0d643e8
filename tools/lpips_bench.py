"""Times core.metrics.calculate_lpips on a synthetic C3-sized evaluation: target and prediction 10 x 2048^2 x 2
(20 image pairs through the AlexNet trunk, ~4.8 TFLOP).

    python tools/lpips_bench.py [--frames 10 --size 2048 --repeats 5 --warmup 2 --no-cpu]
        warm-up, then `repeats` evaluations inside one process, each between two events; prints the median / min / max
        and one JSON line.  The CPU comparison is the float64-checked restatement (tests/lpips_ref.py) in torch CPU
        float32 on the box's threads, on one pair, scaled to the 20 pairs.
    rocprofv3 --kernel-trace --stats -d DIR -o lpips --output-format csv -- python tools/lpips_bench.py --repeats 1 --warmup 1 --no-cpu
    python tools/lpips_bench.py --kernel-trace DIR
        no GPU needed: reads the kernel trace and prints time and TF/s per kernel against the 157.3 TF fp32 MFMA peak
        (the three 3 x 3 convs share one kernel: their dispatches are told apart by their order).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3


def stage_sizes(n):
    c1 = (n + 4 - 11) // 4 + 1
    p1 = (c1 - 3) // 2 + 1
    p2 = (p1 - 3) // 2 + 1
    return c1, p1, p2


def conv_flops(H, W):
    """2 * MAC of the five convs for one image."""
    (h1, w1), (hp1, wp1), (hp2, wp2) = zip(stage_sizes(H), stage_sizes(W))
    return {"conv1": 2.0 * 363 * 64 * h1 * w1, "conv2": 2.0 * 1600 * 192 * hp1 * wp1,
            "conv3": 2.0 * 1728 * 384 * hp2 * wp2, "conv4": 2.0 * 3456 * 256 * hp2 * wp2,
            "conv5": 2.0 * 2304 * 256 * hp2 * wp2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--evaluations", type=int, default=None, help="evaluations the trace holds (--kernel-trace)")
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_table_ev(a.kernel_trace, a.frames, a.size, a.evaluations or 1)

    import torch
    from diffsplitting_amd.core.lpips import LPIPS
    from diffsplitting_amd.core.metrics import calculate_lpips
    from tests import lpips_ref as R
    torch.set_grad_enabled(False)
    sd = R.synth_state_dict()
    model = LPIPS(net='alex', state_dict=sd).cuda()
    g = torch.Generator().manual_seed(0)
    target = torch.rand((a.frames, a.size, a.size, 2), generator=g)
    pred = (target + 0.05 * torch.randn(target.shape, generator=g)).cuda()
    target = target.cuda()
    for _ in range(a.warmup):
        calculate_lpips(target, pred, model)
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = calculate_lpips(target, pred, model)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    pairs = 2 * a.frames
    flops = sum(conv_flops(a.size, a.size).values()) * 2 * pairs
    med = statistics.median(times)
    res = {"workload": f"calculate_lpips {a.frames} x {a.size}^2 x 2 ({pairs} pairs)", "ms_median": round(med, 2),
           "ms_min": round(min(times), 2), "ms_max": round(max(times), 2), "repeats": a.repeats, "warmup": a.warmup,
           "conv_tflop": round(flops / 1e12, 3), "tf_per_s": round(flops / (med * 1e-3) / 1e12, 1),
           "of_fp32_mfma_peak": round(flops / (med * 1e-3) / 1e12 / PEAK_TF, 3),
           "lpips_ch0_mean": sum(out[0]) / len(out[0])}
    if not a.no_cpu:
        tar, prd = R.frames_prepare(target[:1].cpu().numpy(), pred[:1].cpu().numpy(), 0)
        tar, prd = torch.from_numpy(tar), torch.from_numpy(prd)
        R.lpips_ref(sd, tar[:, :, :256, :256], prd[:, :, :256, :256], torch.float32)     # warm ATen up
        t0 = time.perf_counter()
        R.lpips_ref(sd, tar, prd, torch.float32)
        one = time.perf_counter() - t0
        res["cpu_baseline"] = {"what": f"restatement, torch CPU float32, {torch.get_num_threads()} threads, one pair "
                                       f"x {pairs}", "ms": round(one * 1e3 * pairs, 1),
                               "speedup": round(one * 1e3 * pairs / med, 1)}
    print(f"calculate_lpips: median {med:.1f} ms (min {min(times):.1f}, max {max(times):.1f}) over {a.repeats} repeats")
    print(json.dumps(res))


def kernel_table_ev(directory, frames, size, evaluations):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per, n3 = {}, 0
    for r in rows:
        name = r["Kernel_Name"]
        if "k_lpips_" not in name:
            continue
        if "k_lpips_conv1" in name:
            key = "conv1"
        elif "k_lpips_conv<5>" in name or "k_lpips_convILi5" in name:
            key = "conv2"
        elif "k_lpips_conv<3>" in name or "k_lpips_convILi3" in name:
            key = ("conv3", "conv4", "conv5")[n3 % 3]
            n3 += 1
        else:
            key = "k_lpips_" + name.split("k_lpips_")[1].split("(")[0].split("<")[0]
        d = per.setdefault(key, [0, 0.0])
        d[0] += 1
        d[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    fl = conv_flops(size, size)
    images = 2 * frames * 2 * evaluations
    total = sum(v[1] for v in per.values())
    print(f"{evaluations} evaluation(s) of {frames} x {size}^2 x 2 in the trace; fp32 MFMA peak {PEAK_TF} TF")
    print(f"{'kernel':24s} {'launches':>8s} {'ms':>10s} {'share':>7s} {'TF/s':>8s} {'of peak':>8s}")
    for key, (n, ms) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        line = f"{key:24s} {n:8d} {ms:10.2f} {100 * ms / total:6.1f}%"
        if key in fl:
            tf = fl[key] * images / (ms * 1e-3) / 1e12
            line += f" {tf:8.1f} {100 * tf / PEAK_TF:7.1f}%"
        print(line)
    print(f"{'all LPIPS kernels':24s} {sum(v[0] for v in per.values()):8d} {total:10.2f}")


if __name__ == "__main__":
    main()
