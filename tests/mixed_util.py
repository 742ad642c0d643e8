"""Helpers of the mixed-input, TimePredictor and refinement tests on the MI355X and of their rank workers: synthetic
frames, the tiny InDI pair with its TimePredictor, the tiled dataset, and the config files of the command-line tests."""
import json

import numpy as np
import torch

from oracle import cases
from oracle.weights import synth_state_dict
from tests import nets
from tests.util import load_golden


def frames(shape, seed):
    rng = np.random.default_rng(seed)
    return (np.minimum(rng.gamma(2.0, 150.0, size=shape), 4000).astype(np.uint16),
            np.minimum(rng.gamma(3.0, 70.0, size=shape), 4000).astype(np.uint16))


def networks(nsteps):
    from diffsplitting_amd.model.ddpm_modules.time_predictor import TimePredictor
    from diffsplitting_amd.model.ddpm_modules.unet import UNet
    from diffsplitting_amd.model.samplers import InDISampler
    g = load_golden("refine_n1")
    keys = {k: [(a, tuple(s)) for a, s in json.loads(bytes(g[k]).decode())] for k in ("keys1", "keys2", "keys_tp")}
    c = cases.UNET_CASES["joint_32"]["cfg"]
    sds = {"keys1": synth_state_dict(keys["keys1"], 1), "keys2": synth_state_dict(keys["keys2"], 2),
           "keys_tp": synth_state_dict(keys["keys_tp"], 0)}

    def sampler(sd):
        net = UNet(in_channel=1, out_channel=1, inner_channel=c["inner_channel"], norm_groups=c["norm_groups"],
                   channel_mults=c["channel_mults"], attn_res=c["attn_res"], res_blocks=c["res_blocks"], image_size=32)
        s = InDISampler(net, 32, channels=1, out_channel=1, conditional=False, val_schedule_opt={"n_timestep": nsteps}).cuda()
        s.load_state_dict(sd, strict=True)
        s.set_new_noise_schedule({"n_timestep": nsteps}, "cuda")
        return s

    tp = TimePredictor(**cases.TIME_PRED_CFG).cuda()
    tp.load_state_dict(sds["keys_tp"], strict=True)
    return sampler(sds["keys1"]), sampler(sds["keys2"]), tp, sds, c


def dataset(shape, seed, patch=32, grid=16):
    from diffsplitting_amd.data.split_dataset import DataLocation, SplitDatasetTiledPred
    ch0, ch1 = frames(shape, seed)
    ds = SplitDatasetTiledPred("Hagen", DataLocation(arrays=(ch0, ch1)), patch, grid_size=grid, max_qval=0.98)
    return ds, ch0, ch1


_TP = {}


def time_predictor():
    """The synthetic TimePredictor of ``networks`` and its state dict, built once per process."""
    if not _TP:
        from diffsplitting_amd.model.ddpm_modules.time_predictor import TimePredictor
        g = load_golden("refine_n1")
        keys = [(a, tuple(s)) for a, s in json.loads(bytes(g["keys_tp"]).decode())]
        sd = synth_state_dict(keys, 0)
        tp = TimePredictor(**cases.TIME_PRED_CFG).cuda()
        tp.load_state_dict(sd, strict=True)
        _TP.update(tp=tp, sd=sd)
    return _TP["tp"], _TP["sd"]


def write_configs(tmp_path):
    from diffsplitting_amd.data.tiff import imwrite
    rng = np.random.default_rng(9)
    paths = []
    for ch, (shape, scale) in enumerate(((2.0, 150.0), (3.0, 70.0))):
        p = str(tmp_path / f"val_ch{ch}.tif")
        imwrite(p, np.minimum(rng.gamma(shape, scale, size=(1, 64, 64)), 1900).astype(np.uint16))
        paths.append(p)
    part = lambda extra: dict({"name": "Hagen", "datapath": {"ch0": paths[0], "ch1": paths[1]}}, **extra)
    datasets = {"patch_size": 32, "max_qval": 0.98, "upper_clip": False, "channel_weights": [1, 1],
                "train": part({"batch_size": 3, "uncorrelated_channels": False, "gaussian_noise_std_factor": 0.02}),
                "val": part({})}
    path = {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None}
    c = cases.TIME_PRED_CFG
    tp_cfg = {"name": "tiny_tp", "phase": "train", "gpu_ids": [0], "path": path, "datasets": datasets,
              "model": {"loss_type": "l2", "which_model_G": "UnetClassifier",
                        "unet": {"in_channel": c["in_channel"], "out_channel": c["out_channel"],
                                 "inner_channel": c["inner_channel"], "norm_groups": c["norm_groups"],
                                 "channel_multiplier": list(c["channel_mults"]), "attn_res": list(c["attn_res"]),
                                 "res_blocks": c["res_blocks"], "dropout": 0.2}}}
    joint_cfg = {"name": "tiny_joint", "phase": "val", "gpu_ids": [0], "path": path, "datasets": datasets,
                 "model": nets.tiny_indi_section(1, 1, "joint_indi")}
    out = {}
    for name, cfg in (("tp", tp_cfg), ("joint", joint_cfg)):
        p = tmp_path / f"{name}.json"
        p.write_text(json.dumps(cfg, indent=2))
        out[name] = (cfg, str(p))
    _, sd = time_predictor()
    pth = str(tmp_path / "best_time_predictor.pth")
    torch.save({k: v.clone() for k, v in sd.items()}, pth)
    return out, pth
