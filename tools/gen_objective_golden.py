"""Writes tests/golden/objective_{sr3,ddpm,indi,joint}.npz with the REFERENCE's own code: one seeded CPU run of
``p_losses(x_in)`` per sampler family on the tiny UNet cases of oracle/cases.py with ``synth_state_dict`` weights.

    python tools/gen_objective_golden.py /path/to/reference/checkout

The modules are in ``.eval()`` (dropout is identity, as in the engine), ``set_loss('cpu')`` is called, ``torch`` and
``numpy`` are seeded, and ``p_losses`` runs with ``noise=None`` so every draw is the reference's own, in its order.
A wrapper around each sampler's ``q_sample`` and a forward hook on each ``denoise_fn`` record the intermediate values;
``np.random.randint`` is wrapped to record SR3's integer t.  Only inputs and outputs are stored; nothing of the
reference is copied.  Each file holds the seeds, ``input`` / ``target``, the drawn ``t`` (and SR3's
``continuous_sqrt_alpha_cumprod``), ``noise``, ``x_noisy``, ``x_recon``, the reference's fp32 ``loss`` and the UNet's
state-dict key list (``keys``, as the other fixtures).
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from oracle.weights import synth_state_dict  # noqa: E402

SEED_TORCH, SEED_NUMPY = 20250917, 917
N_INDI = 20


def key_shapes(module):
    return [(k, list(v.shape)) for k, v in module.state_dict().items()]


def load_synth(module):
    ks = key_shapes(module)
    missing, unexpected = module.load_state_dict(synth_state_dict(ks), strict=False)
    assert not unexpected, unexpected
    return ks


def data(name, shape):
    g = torch.Generator().manual_seed(zlib.crc32(("objective_" + name).encode()) & 0x7FFFFFFF)
    return torch.randn(shape, generator=g)


def record(sampler, net):
    """q_sample's keyword arguments and result, the UNet's time argument and output, into one dict."""
    rec = {}
    inner = sampler.q_sample

    def q_sample(*args, **kwargs):
        assert not args
        out = inner(**kwargs)
        rec.update({k: v.detach().clone() for k, v in kwargs.items() if torch.is_tensor(v)})
        rec["x_noisy"] = out.detach().clone()
        return out

    sampler.q_sample = q_sample
    net.register_forward_hook(lambda m, inp, out: rec.update(time=inp[1].detach().clone(), x_recon=out.detach().clone()))
    return rec


def seeded(fn):
    torch.manual_seed(SEED_TORCH)
    np.random.seed(SEED_NUMPY)
    return fn()


def save(name, **arrs):
    arrs.update(seed_torch=np.int64(SEED_TORCH), seed_numpy=np.int64(SEED_NUMPY), torch_version=np.array(torch.__version__),
                numpy_version=np.array(np.__version__))
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def jstr(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def main(ref):
    sys.path.insert(0, ref)
    from model.sr3_modules.unet import UNet as UNetSr3
    from model.sr3_modules.diffusion import GaussianDiffusion as GDSr3
    from model.ddpm_modules.unet import UNet as UNetDdpm
    from model.ddpm_modules.diffusion import GaussianDiffusion as GDDdpm
    from model.ddpm_modules.indi import InDI
    from model.ddpm_modules.joint_indi import JointIndi
    torch.set_grad_enabled(False)

    # ---- SR3: conditional, l1 (always 'sum'), lin_25
    case = cases.UNET_CASES["sr3_tiny"]
    B, H, W = case["B"], case["H"], case["W"]
    net = UNetSr3(**case["cfg"]).eval()
    ks = load_synth(net)
    gd = GDSr3(net, 32, channels=3, loss_type="l1", conditional=True).eval()
    gd.set_new_noise_schedule(cases.SCHEDULES["lin_25"], "cpu")
    gd.set_loss("cpu")
    x_in = {"target": data("sr3_target", (B, 3, H, W)), "input": data("sr3_input", (B, 3, H, W))}
    rec = record(gd, net)
    randint, drawn = np.random.randint, []
    np.random.randint = lambda *a, **k: drawn.append(randint(*a, **k)) or drawn[-1]
    try:
        loss = seeded(lambda: gd.p_losses(x_in))
    finally:
        np.random.randint = randint
    save("objective_sr3", keys=jstr(ks), input=x_in["input"], target=x_in["target"], t=np.int64(drawn[0]),
         continuous_sqrt_alpha_cumprod=rec["continuous_sqrt_alpha_cumprod"].reshape(-1), noise=rec["noise"],
         x_noisy=rec["x_noisy"], x_recon=rec["x_recon"], loss=loss.numpy())

    # ---- DDPM: channels = 1, conditional, l2, 'mean', lin_8 (the 2-channel UNet output broadcasts against the noise)
    case = cases.UNET_CASES["ddpm_tiny"]
    B, H, W = case["B"], case["H"], case["W"]
    net = UNetDdpm(**case["cfg"]).eval()
    ks = load_synth(net)
    gd = GDDdpm(net, 32, channels=1, loss_type="l2", lr_reduction="mean", conditional=True).eval()
    gd.set_new_noise_schedule(cases.SCHEDULES["lin_8"], "cpu")
    gd.set_loss("cpu")
    x_in = {"target": data("ddpm_target", (B, 1, H, W)), "input": data("ddpm_input", (B, 1, H, W))}
    rec = record(gd, net)
    loss = seeded(lambda: gd.p_losses(x_in))
    save("objective_ddpm", keys=jstr(ks), input=x_in["input"], target=x_in["target"], t=rec["t"], noise=rec["noise"],
         x_noisy=rec["x_noisy"], x_recon=rec["x_recon"], loss=loss.numpy())

    # ---- InDI: out_channel = 2, unconditional, l1 ('sum'), n = 20
    net = UNetDdpm(**case["cfg"]).eval()
    ks = load_synth(net)
    indi = InDI(net, 32, channels=2, loss_type="l1", out_channel=2, conditional=False,
                val_schedule_opt={"n_timestep": N_INDI}).eval()
    indi.set_new_noise_schedule({"n_timestep": N_INDI}, "cpu")
    indi.set_loss("cpu")
    x_in = {"target": data("indi_target", (B, 2, H, W)), "input": data("indi_input", (B, 1, H, W))}
    rec = record(indi, net)
    loss = seeded(lambda: indi.p_losses(x_in))
    save("objective_indi", keys=jstr(ks), input=x_in["input"], target=x_in["target"], t=rec["t"].reshape(-1),
         noise=rec["noise"], x_noisy=rec["x_noisy"], x_recon=rec["x_recon"], loss=loss.numpy(), n_timestep=np.int64(N_INDI))

    # ---- JointIndi: two 1 -> 1 UNets, l1, n = 20; allow_full_translation false ("custom") and true ("full")
    case = cases.UNET_CASES["joint_32"]
    B, H, W = case["B"], case["H"], case["W"]
    target = data("joint_target", (B, 2, H, W))
    out = {"target": target, "n_timestep": np.int64(N_INDI)}
    for tag, full in (("custom", False), ("full", True)):
        n1, n2 = UNetDdpm(**case["cfg"]).eval(), UNetDdpm(**case["cfg"]).eval()
        joint = JointIndi(None, 32, channels=1, loss_type="l1", out_channel=1, denoise_fn_ch1=n1, denoise_fn_ch2=n2,
                          conditional=False, val_schedule_opt={"n_timestep": N_INDI}, allow_full_translation=full).eval()
        ks = load_synth(joint)
        joint.set_new_noise_schedule({"n_timestep": N_INDI}, "cpu")
        joint.set_loss("cpu")
        r1, r2 = record(joint.indi1, n1), record(joint.indi2, n2)
        loss = seeded(lambda: joint.p_losses({"target": target}))
        out["keys"] = jstr(ks)
        for i, r in ((1, r1), (2, r2)):
            out[f"{tag}_t{i}"] = r["t"].reshape(-1)
            for k in ("noise", "x_noisy", "x_recon"):
                out[f"{tag}_{k}{i}"] = r[k]
        out[f"{tag}_loss"] = loss.numpy()
        log = joint.get_current_log()
        out[f"{tag}_log"] = np.array([log["loss_splitting"], log["alpha"], log["offset"], log["scale"]], dtype=np.float64)
    save("objective_joint", **out)


if __name__ == "__main__":
    main(sys.argv[1])
