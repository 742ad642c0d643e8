"""Measurements of the mixed-input evaluation at BASELINE C5's size.

    python tools/mixed_measure.py range [n ...]     dsx_mix_range on 10 x 2048^2 frames per channel (wall, 5 calls each);
                                                    run it under `rocprofv3 --kernel-trace --stats` for the kernel time
    python tools/mixed_measure.py numpy [n ...]     the float64 numpy restatement of the same table, on this host
    python tools/mixed_measure.py drivers           evaluate_time_predictor (21 ratios x 490 tiles of 512^2, batches of 8) and
                                                    predict_tiled_mixed (490 tiles, n = 1 and 3), fp16 and fp32,
                                                    synthesised weights of the C5 networks' shapes (this mode has not
                                                    produced a recorded figure yet: DESIGN.md item 24)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_grad_enabled(False)


def frames():
    rng = np.random.default_rng(1)
    return (np.minimum(rng.gamma(2.0, 150.0, size=(10, 2048, 2048)), 1993).astype(np.uint16),
            np.minimum(rng.gamma(3.0, 70.0, size=(10, 2048, 2048)), 1993).astype(np.uint16))


def norm(ch0, ch1):
    m = np.array([np.quantile(ch0[0], 0.98) / 2, np.quantile(ch1[0], 0.98) / 2])
    return m, m


def main():
    what, ns = sys.argv[1], [int(v) for v in sys.argv[2:]] or [100, 20]
    ch0, ch1 = frames()
    mean, std = norm(ch0, ch1)
    if what == "numpy":
        from tests import mixed_ref as MR
        for n in ns:
            t = time.perf_counter()
            tab = MR.range_table(ch0, ch1, n, mean, std)
            print(json.dumps({"what": "numpy_range_table", "n": n, "seconds": time.perf_counter() - t,
                              "threads": os.environ.get("OMP_NUM_THREADS"), "row0": tab[0].tolist()}), flush=True)
        return
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    if what == "range":
        dev = {0: torch.from_numpy(ch0.astype(np.float32)).cuda(), 1: torch.from_numpy(ch1.astype(np.float32)).cuda()}
        for n in ns:
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t = time.perf_counter()
                tab = compute_input_normalization_dict(dev, n, mean, std)
                ts.append(time.perf_counter() - t)
            print(json.dumps({"what": "dsx_mix_range_wall", "n": n, "seconds_median": float(np.median(ts)),
                              "seconds_first": ts[0], "row0": [float(v) for v in tab[0]]}), flush=True)
        return
    # drivers: the C5 networks' shapes with synthesised weights (timing only)
    from diffsplitting_amd.data.tiled_predict import evaluate_time_predictor, predict_tiled_mixed
    from diffsplitting_amd.model.ddpm_modules.time_predictor import TimePredictor
    from diffsplitting_amd.model.ddpm_modules.unet import UNet
    from diffsplitting_amd.model.samplers import InDISampler
    import types
    ds = SplitDatasetTiledPred("Hagen", DataLocation(arrays=(ch0, ch1)), 512, grid_size=256, max_qval=0.98,
                               normalization_dict={"mean_input": mean.sum(), "std_input": std.sum(),
                                                   "mean_target": mean, "std_target": std})
    unet_kw = dict(in_channel=1, out_channel=1, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 4, 8, 8),
                   attn_res=(16,), res_blocks=2, image_size=512)

    def synth(mod, seed, dtype):
        g = torch.Generator().manual_seed(seed)
        for name, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05 + (1.0 if name.endswith("norm.weight") else 0.0))
        for m in mod.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = dtype
        return mod

    for dtype in ("f16", "f32"):
        tp = synth(TimePredictor(**unet_kw), 0, dtype).cuda()
        t = time.perf_counter()
        all_pred, rmse = evaluate_time_predictor(ds, tp, num_timesteps=20, batch_tiles=8)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        print(json.dumps({"what": "evaluate_time_predictor", "dtype": dtype, "tiles": len(ds), "ratios": 21, "seconds": dt,
                          "tiles_per_s": 21 * len(ds) / dt}), flush=True)
        i1 = synth(InDISampler(UNet(with_time_emb=True, **unet_kw), 512, channels=1, out_channel=1, conditional=False), 1, dtype).cuda()
        i2 = synth(InDISampler(UNet(with_time_emb=True, **unet_kw), 512, channels=1, out_channel=1, conditional=False), 2, dtype).cuda()
        netG = types.SimpleNamespace(indi1=i1, indi2=i2, noise_source=None)
        for n in (1, 3):
            t = time.perf_counter()
            for smp in (i1, i2):
                smp.set_new_noise_schedule({"n_timestep": n}, "cuda")
            (canvas, psnr), pred_t = predict_tiled_mixed(netG, tp, ds, 0.5, num_timesteps=n, batch_tiles=8)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            print(json.dumps({"what": "predict_tiled_mixed", "dtype": dtype, "n": n, "tiles": len(ds), "seconds": dt,
                              "tiles_per_s": len(ds) / dt}), flush=True)


if __name__ == "__main__":
    main()
