"""Measurements of the objective's forward evaluation on one MI355X (nothing here is asserted; DESIGN.md quotes it):

    python tools/objective_measure.py

  dtype : the loss of the four reference fixtures (tests/golden/objective_*.npz, the fixture's t and noise injected)
          with bf16 MFMA operands, relative to the fp32 engine's loss;
  time  : p_losses(...).item() -- what DDPM.eval_loss() runs -- at the size of config/sr_sr3_16_128.json (B = 16, 128^2,
          fp32 and bf16, device noise), and one UNet forward of the same engine: two separately timed wall-clock
          medians over 10 synchronised calls after 2 warm-up calls.
One JSON line per figure.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle import cases  # noqa: E402
from tests.util import golden_state_dict  # noqa: E402
from diffsplitting_amd.model.ddpm_modules.unet import UNet as UNetDdpm  # noqa: E402
from diffsplitting_amd.model.samplers import GaussianSampler, GaussianSamplerDdpm, InDISampler, JointIndiSampler  # noqa: E402
from diffsplitting_amd.model.sr3_modules.unet import UNet as UNetSr3  # noqa: E402

torch.set_grad_enabled(False)
N_INDI = 20


def unet(cls, cfg):
    return cls(**{k: cfg[k] for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "channel_mults",
                                      "attn_res", "res_blocks", "image_size")})


def set_dtype(smp, dtype):
    for m in smp.modules():
        if hasattr(m, "compute_dtype"):
            m.compute_dtype = dtype


def fixtures():
    """name -> (sampler, callable returning the loss with the fixture's draws injected)"""
    cu = lambda g, k: torch.from_numpy(g[k]).cuda()
    sd, g = golden_state_dict("objective_sr3")
    s = GaussianSampler(unet(UNetSr3, cases.UNET_CASES["sr3_tiny"]["cfg"]), 32, channels=3, loss_type="l1").cuda()
    s.set_new_noise_schedule(cases.SCHEDULES["lin_25"], "cuda")
    s.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()}, strict=False)
    yield "sr3", s, lambda s=s, g=g: s({"target": cu(g, "target"), "input": cu(g, "input")}, cu(g, "noise"),
                                      continuous_sqrt_alpha_cumprod=torch.from_numpy(g["continuous_sqrt_alpha_cumprod"]))
    sd, g = golden_state_dict("objective_ddpm")
    s = GaussianSamplerDdpm(unet(UNetDdpm, cases.UNET_CASES["ddpm_tiny"]["cfg"]), 32, channels=1, loss_type="l2",
                            lr_reduction="mean").cuda()
    s.set_new_noise_schedule(cases.SCHEDULES["lin_8"], "cuda")
    s.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()}, strict=False)
    yield "ddpm", s, lambda s=s, g=g: s({"target": cu(g, "target"), "input": cu(g, "input")}, cu(g, "noise"),
                                       t=torch.from_numpy(g["t"]))
    sd, g = golden_state_dict("objective_indi")
    s = InDISampler(unet(UNetDdpm, cases.UNET_CASES["ddpm_tiny"]["cfg"]), 32, channels=2, loss_type="l1", out_channel=2,
                    conditional=False, val_schedule_opt={"n_timestep": N_INDI}).cuda()
    s.set_new_noise_schedule({"n_timestep": N_INDI}, "cuda")
    s.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()}, strict=True)
    yield "indi", s, lambda s=s, g=g: s({"target": cu(g, "target"), "input": cu(g, "input")}, cu(g, "noise"),
                                       t=torch.from_numpy(g["t"]))
    sd, g = golden_state_dict("objective_joint")
    cfg = cases.UNET_CASES["joint_32"]["cfg"]
    for tag, full in (("custom", False), ("full", True)):
        s = JointIndiSampler(None, 32, channels=1, loss_type="l1", out_channel=1, denoise_fn_ch1=unet(UNetDdpm, cfg),
                             denoise_fn_ch2=unet(UNetDdpm, cfg), conditional=False,
                             val_schedule_opt={"n_timestep": N_INDI}, allow_full_translation=full).cuda()
        s.set_new_noise_schedule({"n_timestep": N_INDI}, "cuda")
        s.load_state_dict(sd, strict=True)

        def run(s=s, g=g, tag=tag):
            draws = [torch.from_numpy(g[f"{tag}_noise{i}"]) for i in (1, 2)]
            s.noise_source = lambda shape: draws.pop(0)
            return s({"target": cu(g, "target")}, t=(torch.from_numpy(g[f"{tag}_t1"]), torch.from_numpy(g[f"{tag}_t2"])))
        yield "joint_" + tag, s, run


def wall(fn, n=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    for name, smp, run in fixtures():
        smp.set_loss("cuda")
        vals = {}
        for dtype in ("f32", "bf16"):
            set_dtype(smp, dtype)
            vals[dtype] = float(run())
        print(json.dumps({"what": "loss_dtype", "case": name, "f32": vals["f32"], "bf16": vals["bf16"],
                          "rel_dev": abs(vals["bf16"] - vals["f32"]) / abs(vals["f32"])}), flush=True)
        del smp
    net = unet(UNetSr3, bench.UNET)
    smp = GaussianSampler(net, 128, channels=3, loss_type="l1", conditional=True).cuda()
    smp.set_new_noise_schedule(dict(schedule="linear", n_timestep=2000, linear_start=1e-6, linear_end=1e-2), "cuda")
    smp.set_loss("cuda")
    x_in = {"target": torch.randn(16, 3, 128, 128, device="cuda"), "input": torch.randn(16, 3, 128, 128, device="cuda")}
    x, t = torch.randn(16, 6, 128, 128, device="cuda"), torch.rand(16, 1, device="cuda")
    for dtype in ("f32", "bf16"):
        set_dtype(smp, dtype)
        fwd = wall(lambda: net(x, t))
        obj = wall(lambda: smp(x_in).item())
        print(json.dumps({"what": "eval_time", "dtype": dtype, "B": 16, "size": 128, "unet_forward_ms": fwd,
                          "p_losses_item_ms": obj}), flush=True)


if __name__ == "__main__":
    main()
