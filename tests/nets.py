"""Tiny networks, config sections and small inputs shared by the tests.  Nothing here is cached and importing this module
sets nothing global: a test module that shares an object caches it itself."""
import ctypes as C
import json

import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def i64(*v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def dbl(*v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def rand(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- options and config files
def opt(model_section, **extra):
    from diffsplitting_amd.core.logger import dict_to_nonedict
    d = {"model": json.loads(json.dumps(model_section)), "phase": "val", "gpu_ids": [0], "distributed": False,
         "path": {"resume_state": None}}
    d.update(extra)
    return dict_to_nonedict(d)


def tiny_indi_section(in_ch=2, out_ch=2, which="indi"):
    return {"which_model_G": which, "loss_type": "l1", "lr_reduction": "mean", "finetune_norm": False,
            "w_input_loss": 0.0,
            "unet": {"in_channel": in_ch, "out_channel": out_ch, "inner_channel": 16, "norm_groups": 16,
                     "channel_multiplier": [1, 2, 4] if which == "indi" else [1, 2, 4, 8], "attn_res": [],
                     "res_blocks": 1, "dropout": 0},
            "beta_schedule": {"train": {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-6, "linear_end": 1e-2},
                              "val": {"schedule": "linear", "n_timestep": 3, "linear_start": 1e-6, "linear_end": 1e-2}},
            "diffusion": {"image_size": 32, "channels": out_ch, "conditional": False}}


def hagen64_section():
    """The tiny InDI section with the four levels of the golden ``unet_hagen_64`` weights."""
    sec = tiny_indi_section()
    sec["unet"]["channel_multiplier"] = [1, 2, 4, 8]
    return sec


def write_config(tmp_path, which, loss_type="l2", **ds):
    """The smallest config file ``split`` and ``time_prediction`` read their flags against; ``ds`` goes into "datasets"."""
    cfg = {"name": "tiny", "phase": "val", "gpu_ids": [0], "path": {"resume_state": None},
           "datasets": dict({"patch_size": 32, "max_qval": 0.98, "train": {"name": "Hagen", "batch_size": 3},
                             "val": {"name": "Hagen"}}, **ds),
           "model": {"which_model_G": which, "loss_type": loss_type}}
    p = tmp_path / f"{which}{len(ds) or ''}.json"
    p.write_text(json.dumps(cfg))
    return str(p)


# ----------------------------------------------------------------------------- networks and weights
def unet(flavour, cfg):
    from diffsplitting_amd.model.ddpm_modules.unet import UNet as UNetDdpm
    from diffsplitting_amd.model.sr3_modules.unet import UNet as UNetSr3
    cls = UNetSr3 if flavour == "sr3" else UNetDdpm
    return cls(in_channel=cfg["in_channel"], out_channel=cfg["out_channel"], inner_channel=cfg["inner_channel"],
               norm_groups=cfg["norm_groups"], channel_mults=cfg["channel_mults"], attn_res=cfg["attn_res"],
               res_blocks=cfg["res_blocks"], image_size=cfg["image_size"])


def load(smp, sd, prefix="denoise_fn."):
    missing, unexpected = smp.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(not k.startswith("denoise_fn") and ".denoise_fn" not in k for k in missing), missing


def engine_state_dict(case, seed):
    """synthetic weights for the engine's own parameter table (no fixture: the engine names its parameters)"""
    from diffsplitting_amd import engine
    from oracle.weights import synth_state_dict
    cfg = case["cfg"]
    eng = engine.UNetEngine(engine.make_cfg(case["flavour"], cfg["in_channel"], cfg["out_channel"],
                                            cfg["inner_channel"], cfg["norm_groups"], cfg["channel_mults"],
                                            cfg["attn_res"], cfg["res_blocks"], cfg["image_size"]), case["flavour"])
    return synth_state_dict(zip(eng.param_names, eng.param_shapes), seed=seed)
