"""Times ``validation_report`` on the device next to the same arithmetic in numpy on the host:

    python tools/validation_measure.py [B C H W]        (default 8 2 512 512, Cin = 1)

Prints the two launches alone (device events around ``dsx_val_report``), the whole call (with its allocations, the
statistics' copy and, with visuals, the three images formed on the host) and the host's numpy time.  A measurement,
no threshold."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsplitting_amd._lib import check, lib  # noqa: E402
from diffsplitting_amd.core.validation import VAL_CHUNK, validation_report  # noqa: E402


def numpy_block(inp, tar, pred, nd):
    """The block per item, as the reference writes it."""
    out = []
    for b in range(tar.shape[0]):
        i_img = ((inp[b] * nd["std_input"] + nd["mean_input"]) / 2).astype(np.uint16)
        t_img = (tar[b] * nd["std_target"] + nd["mean_target"]).astype(np.uint16)
        p_img = np.clip(pred[b] * nd["std_target"] + nd["mean_target"], 0, 65535).astype(np.uint16)
        t32, p32 = t_img.reshape(len(t_img), -1).astype(np.float32), p_img.reshape(len(p_img), -1).astype(np.float32)
        psnr = 20 * np.log10((t32.max(1) - t32.min(1)) / np.sqrt(((t32 - p32) ** 2).mean(1)))
        minv = t_img.reshape(len(t_img), -1).min(axis=1).reshape(-1, 1, 1)
        t_img = t_img - minv
        maxv = t_img.reshape(len(t_img), -1).max(axis=1).reshape(-1, 1, 1)
        i_img = i_img - i_img.min()
        out.append((psnr, t_img / maxv, i_img / i_img.reshape(len(i_img), -1).max(axis=1).reshape(-1, 1, 1),
                    np.clip((p_img - minv) / maxv, 0, 1)))
    return out


def main(B=8, Cn=2, H=512, W=512, Cin=1, reps=50):
    rng = np.random.default_rng(0)
    nd = {"mean_input": np.float64(1246.59), "std_input": np.float64(1246.59),
          "mean_target": np.resize([759.685, 486.905], Cn).reshape(-1, 1, 1),
          "std_target": np.resize([759.685, 486.905], Cn).reshape(-1, 1, 1)}
    tar = rng.uniform(-0.9, 1.5, size=(B, Cn, H, W)).astype(np.float32)
    pred = (tar + rng.normal(0, 0.2, size=tar.shape)).astype(np.float32)
    inp = rng.uniform(-0.9, 1.5, size=(B, Cin, H, W)).astype(np.float32)
    t0 = time.perf_counter()
    for _ in range(3):
        numpy_block(inp, tar, pred, nd)
    host = (time.perf_counter() - t0) / 3
    di, dt, dp = (torch.from_numpy(a).cuda() for a in (inp, tar, pred))
    for visuals in (False, True):
        for _ in range(3):
            validation_report(di, dt, dp, nd, visuals=visuals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            validation_report(di, dt, dp, nd, visuals=visuals)
        torch.cuda.synchronize()
        print(f"validation_report(visuals={visuals}): {(time.perf_counter() - t0) / reps * 1e3:.3f} ms per call")
    # the two launches alone
    u16 = lambda like: torch.empty(like.shape, dtype=torch.uint16, device="cuda")
    q = [u16(di), u16(dt), u16(dp)]
    n = [u16(di), u16(dt), u16(dp)]
    nblk = (H * W + VAL_CHUNK - 1) // VAL_CHUNK
    part = torch.empty(B * (Cn + Cin) * nblk * 4, dtype=torch.int64, device="cuda")
    stats = torch.empty(1 + B * (3 * Cn + 2 * Cin), dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    pd = C.POINTER(C.c_double)
    mt, st = (np.ascontiguousarray(nd[k].reshape(-1)) for k in ("mean_target", "std_target"))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(with_n):
        nn = [p(t) for t in n] if with_n else [None, None, None]
        check(lib.dsx_val_report(p(di), p(dt), p(dp), B, Cin, Cn, H, W, float(nd["mean_input"]), float(nd["std_input"]),
                                 mt.ctypes.data_as(pd), st.ctypes.data_as(pd), p(q[0]), p(q[1]), p(q[2]), *nn, p(part),
                                 p(stats), stream))
    for with_n in (False, True):
        for _ in range(5):
            launch(with_n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch(with_n)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 200 * 1e3
        px = B * Cn * H * W
        moved = px * (8 + 4) + B * Cin * H * W * (4 + 2) + (px * 8 + B * Cin * H * W * 4 if with_n else 0)
        print(f"dsx_val_report(numerators={with_n}): {us:.1f} us per call, {moved / us / 1e6:.2f} TB/s of "
              f"{moved / 1e6:.1f} MB moved")
    print(f"numpy on the host, the same block per item: {host * 1e3:.1f} ms  (B={B}, C={Cn}, Cin={Cin}, {H}x{W})")


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:5]])
