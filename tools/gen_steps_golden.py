"""Writes tests/golden/steps_{sr3,ddpm,indi}.npz and interpolate_ddpm.npz with the REFERENCE's own code: seeded CPU
runs of the single reverse steps (``p_sample`` / ``p_mean_variance``, ``inference_one_step``) and of ``interpolate`` on
the tiny UNet cases of oracle/cases.py with ``synth_state_dict`` weights and the ``lin_8`` schedule, B = 2 at 32 x 32.

    python tools/gen_steps_golden.py /path/to/reference/checkout

The modules are in ``.eval()``.  ``torch.randn_like`` and the DDPM module's ``noise_like`` are wrapped to record every
draw in draw order, a forward hook on each ``denoise_fn`` records the UNet's time argument and output, and wrappers
around ``predict_start_from_noise`` / ``q_posterior`` / ``q_sample`` / ``p_sample`` record the intermediate values.
Only inputs and outputs are stored; nothing of the reference is copied.  Keys carry the case as a suffix
(``_t7_clip1`` ...); ``keys`` is the UNet's state-dict key list, as in the other fixtures.
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

SEED_TORCH = 20251017
B, H, W = 2, 32, 32
SR3_T, DDPM_CASES = (7, 3, 0), (("mixed", (5, 0), False), ("repeat", (7, 7), True))
INDI_CASES = (("a", 0.25, 1.0), ("b", 0.1, 0.1))
INTERP_CASES = (("a", 0.3, 5), ("b", 0.5, None))


def key_shapes(module):
    return [(k, list(v.shape)) for k, v in module.state_dict().items()]


def load_synth(module):
    ks = key_shapes(module)
    missing, unexpected = module.load_state_dict(synth_state_dict(ks), strict=False)
    assert not unexpected, unexpected
    return ks


def data(name, shape):
    g = torch.Generator().manual_seed(zlib.crc32(("steps_" + name).encode()) & 0x7FFFFFFF)
    return torch.randn(shape, generator=g)


def jstr(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def save(name, **arrs):
    arrs.update(seed_torch=np.int64(SEED_TORCH), torch_version=np.array(torch.__version__))
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


class Recorder:
    """Lists of clones, by name, in call order."""

    def __init__(self):
        self.log = {}

    def add(self, name, t):
        self.log.setdefault(name, []).append(t.detach().clone())
        return t

    def wrap(self, obj, attr, name, arg=None):
        """Record the result of ``obj.attr(...)`` (and the keyword / positional argument ``arg``) at every call."""
        inner = getattr(obj, attr)

        def fn(*args, **kwargs):
            if arg is not None:
                self.add(name + "_" + str(arg), kwargs[arg] if isinstance(arg, str) else args[arg])
            out = inner(*args, **kwargs)
            self.add(name, out[0] if isinstance(out, tuple) else out)
            return out

        setattr(obj, attr, fn)

    def hook(self, net):
        net.register_forward_hook(lambda m, inp, out: (self.add("time", inp[1]), self.add("net", out)) and None)

    def pop(self):
        log, self.log = self.log, {}
        return log


def seeded(fn):
    torch.manual_seed(SEED_TORCH)
    return fn()


def main(ref):
    sys.path.insert(0, ref)
    from model.sr3_modules.unet import UNet as UNetSr3
    from model.sr3_modules.diffusion import GaussianDiffusion as GDSr3
    from model.ddpm_modules.unet import UNet as UNetDdpm
    import model.ddpm_modules.diffusion as ddpm_diffusion
    from model.ddpm_modules.indi import InDI
    torch.set_grad_enabled(False)
    rec = Recorder()
    rec.wrap(torch, "randn_like", "randn_like")
    rec.wrap(ddpm_diffusion, "noise_like", "noise_like")
    sched = cases.SCHEDULES["lin_8"]

    # ---- SR3: conditional, one x and one condition for every case (the UNet output depends on t alone)
    net = UNetSr3(**cases.UNET_CASES["sr3_tiny"]["cfg"]).eval()
    ks = load_synth(net)
    gd = GDSr3(net, 32, channels=3, conditional=True).eval()
    gd.set_new_noise_schedule(sched, "cpu")
    rec.hook(net)
    rec.wrap(gd, "predict_start_from_noise", "x_recon_raw")
    rec.wrap(gd, "q_posterior", "model_mean", arg="x_start")
    x, cond = data("sr3_x", (B, 3, H, W)), data("sr3_cond", (B, 3, H, W))
    out = dict(keys=jstr(ks), x=x, condition=cond, t=np.asarray(SR3_T, dtype=np.int64))
    for t in SR3_T:
        for clip in (1, 0):
            sample = seeded(lambda: gd.p_sample(x.clone(), t, clip_denoised=bool(clip), condition_x=cond))
            log = rec.pop()
            mean, logvar = gd.p_mean_variance(x=x.clone(), t=t, clip_denoised=bool(clip), condition_x=cond)
            again = rec.pop()
            assert torch.equal(mean, log["model_mean"][0]) and torch.equal(again["net"][0], log["net"][0])
            tag = f"_t{t}_clip{clip}"
            out["net" + f"_t{t}"] = log["net"][0]
            out["time" + f"_t{t}"] = log["time"][0]
            out["noise" + f"_t{t}"] = log["randn_like"][0] if t > 0 else torch.zeros_like(x)
            assert len(log.get("randn_like", [])) == (1 if t > 0 else 0)
            out["x_recon" + tag] = log["model_mean_x_start"][0]          # what q_posterior received: after the clamp
            out["model_mean" + tag] = mean
            out["log_variance" + f"_t{t}"] = logvar
            out["sample" + tag] = sample
            if not clip:
                assert torch.equal(log["x_recon_raw"][0], log["model_mean_x_start"][0])
    save("steps_sr3", **out)

    # ---- DDPM: conditional, channels = 1; per-sample t, repeat_noise
    case = cases.DDPM_COND_CASE
    net = UNetDdpm(**case["cfg"]).eval()
    ks = load_synth(net)
    gd = ddpm_diffusion.GaussianDiffusion(net, 32, channels=1, conditional=True).eval()
    gd.set_new_noise_schedule(sched, "cpu")
    rec.hook(net)
    rec.wrap(gd, "predict_start_from_noise", "x_recon_raw")
    rec.wrap(gd, "q_posterior", "model_mean", arg="x_start")
    x, cond = data("ddpm_x", (B, 1, H, W)), data("ddpm_cond", (B, 1, H, W))
    out = dict(keys=jstr(ks), x=x, condition=cond)
    for tag, t, repeat in DDPM_CASES:
        t = torch.tensor(t, dtype=torch.long)
        sample = seeded(lambda: gd.p_sample(x.clone(), t, clip_denoised=True, repeat_noise=repeat, condition_x=cond))
        log = rec.pop()
        mean, var, logvar = gd.p_mean_variance(x=x.clone(), t=t, clip_denoised=True, condition_x=cond)
        rec.pop()
        assert torch.equal(mean, log["model_mean"][0]) and len(log["noise_like"]) == 1
        out.update({"t_" + tag: t, "net_" + tag: log["net"][0], "time_" + tag: log["time"][0],
                    "x_recon_" + tag: log["model_mean_x_start"][0], "model_mean_" + tag: mean,
                    "variance_" + tag: var, "log_variance_" + tag: logvar,
                    "noise_" + tag: log["noise_like"][0][:1] if repeat else log["noise_like"][0],
                    "sample_" + tag: sample})
        if repeat:
            assert torch.equal(log["noise_like"][0][0], log["noise_like"][0][1])
    save("steps_ddpm", **out)

    # ---- InDI: out_channel = 2, unconditional
    net = UNetDdpm(**cases.UNET_CASES["ddpm_tiny"]["cfg"]).eval()
    ks = load_synth(net)
    indi = InDI(net, 32, channels=2, out_channel=2, conditional=False, val_schedule_opt={"n_timestep": 4}).eval()
    indi.set_new_noise_schedule({"n_timestep": 4}, "cpu")
    rec.hook(net)
    x = data("indi_x", (B, 2, H, W))
    out = dict(keys=jstr(ks), x=x, e=np.float64(indi.e))
    for tag, delta, t_cur in INDI_CASES:
        sample = seeded(lambda: indi.inference_one_step(x.clone(), delta, t_cur))
        log = rec.pop()
        assert len(log["randn_like"]) == 1
        out.update({"delta_" + tag: np.float64(delta), "t_cur_" + tag: np.float64(t_cur), "net_" + tag: log["net"][0],
                    "time_" + tag: log["time"][0], "noise_" + tag: log["randn_like"][0], "sample_" + tag: sample})
    save("steps_indi", **out)

    # ---- interpolate: unconditional DDPM, channels = 2
    net = UNetDdpm(**cases.UNET_CASES["ddpm_tiny"]["cfg"]).eval()
    ks = load_synth(net)
    gd = ddpm_diffusion.GaussianDiffusion(net, 32, channels=2, conditional=False).eval()
    gd.set_new_noise_schedule(sched, "cpu")
    rec.wrap(gd, "q_sample", "x_noisy")
    rec.wrap(gd, "p_sample", "p_sample", arg=0)
    x1, x2 = data("interp_x1", (B, 2, H, W)), data("interp_x2", (B, 2, H, W))
    out = dict(keys=jstr(ks), x1=x1, x2=x2)
    for tag, lam, t in INTERP_CASES:
        result = seeded(lambda: gd.interpolate(x1, x2, t=t, lam=lam))
        log = rec.pop()
        steps = gd.num_timesteps - 1 if t is None else t
        assert len(log["randn_like"]) == 2 and len(log["noise_like"]) == steps and len(log["x_noisy"]) == 2
        out.update({"lam_" + tag: np.float64(lam), "t_" + tag: np.int64(steps),
                    "noise1_" + tag: log["randn_like"][0], "noise2_" + tag: log["randn_like"][1],
                    "xt1_" + tag: log["x_noisy"][0], "xt2_" + tag: log["x_noisy"][1],
                    "start_" + tag: log["p_sample_0"][0],           # the first step's input: (1 - lam) xt1 + lam xt2
                    "step_noise_" + tag: torch.stack(log["noise_like"]), "result_" + tag: result})
    save("interpolate_ddpm", **out)


if __name__ == "__main__":
    main(sys.argv[1])
