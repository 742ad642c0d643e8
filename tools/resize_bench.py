"""Times data.prepare_data.resize_multiple (lr, hr and sr of a batch) on device-resident uint8 input, and PIL doing the
same on the host.

    python tools/resize_bench.py [--batch 64 --repeats 20 --warmup 5 --inner 10 --threads 16 --no-cpu]

Two workloads: 1024^2 -> 64 / 512 and 256^2 -> 16 / 128, bicubic, B images.  Device: warm-up calls, then `repeats`
intervals of `inner` back-to-back calls between two events (a call is three resizes of a few tens of microseconds, so
one call is too short for the event clock); median / min / max of the per-call time.  Host: the same three
``Image.resize`` calls per image in a pool of `threads` threads (PIL releases the GIL while it resamples), best of three
passes.  Prints a table and one JSON line.  There is no earlier device path to compare with: host PIL is the only
yardstick.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image
    from diffsplitting_amd.data import prepare_data as P
    rng = np.random.default_rng(0)
    results = []
    for side, sizes in ((1024, (64, 512)), (256, (16, 128))):
        host = rng.integers(0, 256, (a.batch, side, side, 3), dtype=np.uint8)
        dev = torch.from_numpy(host).cuda()
        for _ in range(a.warmup):
            P.resize_multiple(dev, sizes, P.BICUBIC)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                P.resize_multiple(dev, sizes, P.BICUBIC)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / a.inner)
        med = statistics.median(times)
        res = {"workload": f"resize_multiple {a.batch} x {side}^2 -> {sizes[0]} / {sizes[1]} bicubic",
               "device_ms_median": round(med, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
               "device_images_per_s": round(a.batch / (med * 1e-3), 1), "repeats": a.repeats, "inner": a.inner,
               "warmup": a.warmup}
        if not a.no_cpu:
            images = [Image.fromarray(h) for h in host]

            def one(img):
                lr = img.resize((sizes[0], sizes[0]), Image.BICUBIC)
                return lr, img.resize((sizes[1], sizes[1]), Image.BICUBIC), lr.resize((sizes[1], sizes[1]), Image.BICUBIC)

            with ThreadPoolExecutor(a.threads) as pool:
                list(pool.map(one, images))                                   # warm
                best = float("inf")
                for _ in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(one, images))
                    best = min(best, time.perf_counter() - t0)
            res.update({"pil_threads": a.threads, "pil_ms_best_of_3": round(best * 1e3, 3),
                        "pil_images_per_s": round(a.batch / best, 1), "device_over_pil": round(best * 1e3 / med, 2)})
        results.append(res)
        line = f"{res['workload']}: device {med:.3f} ms ({res['device_images_per_s']:.0f} images/s)"
        if not a.no_cpu:
            line += f", PIL x{a.threads} threads {res['pil_ms_best_of_3']:.2f} ms ({res['pil_images_per_s']:.0f} images/s), ratio {res['device_over_pil']}"
        print(line)
    print(json.dumps({"resize_bench": results}))


if __name__ == "__main__":
    main()
