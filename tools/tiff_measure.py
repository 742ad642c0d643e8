"""Measurements of the .tif ingestion path, one process:

    python tools/tiff_measure.py [scratch directory]

  * compute_normalization_dict through dsx_order_stats (radix select) and through the quantile_device sort, on
    10 x 2048^2 frames per channel (BASELINE C3's stack) and on 80 x 2048^2 (a training-sized stack: the 10 frames
    repeated 8 times on the device): wall time after a warm call, median of 5, and the peak device memory above the
    resident frames (torch.cuda.max_memory_allocated);
  * the C3 stack from a uint16 .tif: read, then upload + dsx_frames_to_f32 against host clip + astype(float32) + upload.
One JSON line per figure."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_grad_enabled(False)
Q, W = 0.98, [1, 1]


def timed(fn, reps=5):
    fn()                                                            # warm
    ts, peak = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return out, float(np.median(ts)), int(peak)


def main():
    from diffsplitting_amd.data import split_dataset as SD
    from diffsplitting_amd.data.tiff import imread, imwrite
    scratch = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
    os.makedirs(scratch, exist_ok=True)
    rng = np.random.default_rng(1)
    raw = [rng.gamma(2.0, 400.0, size=(10, 2048, 2048)).astype(np.uint16), rng.gamma(3.0, 200.0, size=(10, 2048, 2048)).astype(np.uint16)]
    print(json.dumps({"what": "stack", "above_clip": [float((r > 1993).mean()) for r in raw]}), flush=True)

    # ---- file -> device
    paths = [os.path.join(scratch, f"c3_ch{c}.tif") for c in (0, 1)]
    for p, r in zip(paths, raw):
        imwrite(p, r)
    dev = torch.device("cuda")
    for rep in range(3):
        t = time.perf_counter(); got = [imread(p) for p in paths]; t_read = time.perf_counter() - t
        torch.cuda.synchronize()
        t = time.perf_counter(); d = [SD.frames_to_device(g, dev, SD.UPPER_CLIP) for g in got]; torch.cuda.synchronize()
        t_dev = time.perf_counter() - t
        t = time.perf_counter()
        h = [torch.as_tensor(np.minimum(g, 1993).astype(np.float32)).to(dev) for g in got]; torch.cuda.synchronize()
        t_host = time.perf_counter() - t
        same = all(torch.equal(a, b) for a, b in zip(d, h))
        print(json.dumps({"what": "c3_two_channels_from_tif", "rep": rep, "read_s": t_read, "upload_u16_widen_s": t_dev,
                          "host_clip_astype_upload_f32_s": t_host, "bit_equal": same}), flush=True)
        del h
    for p in paths:
        os.remove(p)

    # ---- statistics
    for frames in (10, 80):
        t0, t1 = (x.repeat(frames // 10, 1, 1).contiguous() for x in d)
        data = {0: t0, 1: t1}

        def by_sort():
            a, b = t0.reshape(-1), t1.reshape(-1)
            s0, s1 = SD.quantile_device(a, Q), SD.quantile_device(b, Q)
            return s0, s1, SD.quantile_device(a.to(torch.float64) * W[0] + b.to(torch.float64) * W[1], Q)
        try:
            nd, t_sel, m_sel = timed(lambda: SD.compute_normalization_dict(data, W, q_val=Q))
            print(json.dumps({"what": "normalization_dict_select", "frames": frames, "seconds_median": t_sel,
                              "peak_bytes": m_sel, "input_max": float(nd["input_max"])}), flush=True)
            old, t_sort, m_sort = timed(by_sort)
            print(json.dumps({"what": "normalization_dict_sort", "frames": frames, "seconds_median": t_sort,
                              "peak_bytes": m_sort, "equal": bool(old[0] == nd["target0_max"] and old[1] == nd["target1_max"]
                                                                  and old[2] == nd["input_max"])}), flush=True)
        except torch.OutOfMemoryError as e:
            print(json.dumps({"what": "out_of_memory", "frames": frames, "message": str(e)[:200]}), flush=True)
        del t0, t1, data
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
