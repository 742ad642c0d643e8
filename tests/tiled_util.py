"""Helpers of the tiled-prediction tests on the MI355X (field noise, blended stitching, step fusion, frame diffusion) and of
their rank workers: the tiny samplers and stacks, the restatements through ``noise_source`` and on the host, the seam
measure, and the ``split`` runs.  The cached builders return objects that the tests of a process share."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import torch

from tests import blend_ref, nets
from tests.blend_step_ref import blend_step_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240
TINY = dict(in_channel=3, out_channel=2, inner_channel=16, norm_groups=16, channel_mults=(1, 2), attn_res=(), res_blocks=1,
            image_size=32)
SCHED = dict(schedule="linear", n_timestep=12, linear_start=1e-3, linear_end=0.3)
SOLVERS = {"dpmpp2m": dict(solver="dpmpp2m", steps=4, eta=0.0, spacing=None),
           "ddim": dict(solver="ddim", steps=4, eta=0.5, spacing=None), "ancestral": None}
BATCH = 4
# (frames, patch, grid): 56 tiles with odd W and a shifted last row and column; pw % 4 = 2 twice; 12 contributors; one tile
BLEND_PLANS = [((2, 40, 57), 16, 8), ((2, 40, 57), 6, 4), ((2, 40, 57), 10, 6), ((1, 37, 50), 24, 8), ((1, 32, 32), 32, 32)]


def crops(plan, ids, Cn, seed, draw, id_base=0):
    """The definition: tile i, cut at (n, y0, x0), holds that crop of the (C, H, W) tensor of the sample stream
    (seed, id_base + n, draw) -- drawn with the generator that was there before the field."""
    from diffsplitting_amd import engine
    N, H, W = plan.data_shape
    p = plan.patch_shape[1]
    frames, out = {}, []
    for i in ids:
        n, y, x = (int(v) for v in plan.patch_start[int(i)])
        if n not in frames:
            frames[n] = engine.randn_samples((1, Cn, H, W), seed, [id_base + n], draw)[0]
        out.append(frames[n][:, y:y + p, x:x + p])
    return torch.stack(out).contiguous()


@functools.lru_cache(maxsize=None)
def plan_of(shape, patch, grid):
    from diffsplitting_amd.data.tiling import TilePlan
    return TilePlan(shape, (1, grid, grid), (1, patch, patch))


def random_tiles(plan, Cn, seed=11):
    return np.random.default_rng(seed).standard_normal((plan.total, Cn) + plan.patch_shape[1:]).astype(np.float32)


# ----------------------------------------------------------------------------- samplers and stacks
def randomise(module, seed):
    """Seeded random weights (oracle/weights.py: GroupNorm gammas around 1, biases off zero) in every UNet of ``module``."""
    from diffsplitting_amd.model.engine_unet import EngineUNet
    from oracle import weights
    sds = []
    for k, m in enumerate(u for u in module.modules() if isinstance(u, EngineUNet)):
        sd = weights.synth_state_dict([(key, tuple(v.shape)) for key, v in m.state_dict().items()], seed=seed + k)
        m.load_state_dict(sd)
        sds.append(sd)
    return sds


@functools.lru_cache(maxsize=None)
def sr3():
    """The tiny conditional sr3 sampler: UNet 3 -> 2 (one condition channel + two noisy target channels)"""
    from diffsplitting_amd.model.samplers import GaussianSampler
    from diffsplitting_amd.model.sr3_modules.unet import UNet
    smp = GaussianSampler(UNet(**TINY), 32, channels=2, conditional=True).cuda()
    smp.set_new_noise_schedule(SCHED, "cuda")
    smp.weights = randomise(smp, 41)[0]
    return smp


@functools.lru_cache(maxsize=None)
def indi():
    from diffsplitting_amd.model import networks
    netG = networks.define_G(nets.opt(nets.tiny_indi_section())).cuda()
    netG.set_new_noise_schedule({"n_timestep": 3}, "cuda")
    randomise(netG, 51)
    assert netG.e == 0.01
    return netG


@functools.lru_cache(maxsize=None)
def joint():
    from diffsplitting_amd.model import networks
    netG = networks.define_G(nets.opt(nets.tiny_indi_section(1, 1, "joint_indi"))).cuda()
    netG.set_new_noise_schedule({"n_timestep": 3}, "cuda")
    randomise(netG, 61)
    assert netG.indi1.e == 0.01 and netG.indi2.e == 0.01
    return netG


def smooth(shape, seed=0):
    N, H, W = shape
    n, y, x = np.mgrid[0:N, 0:H, 0:W].astype(np.float64)
    f = np.sin((x + 3 * n + seed) / 11.0) * np.cos(y / 7.0) + 0.5 * np.sin((x + y + 5 * n) / 17.0)
    return ((f - f.mean()) / f.std()).astype(np.float32)


def stack(shape, patch, grid, seed=0):
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    nd = dict(mean_input=0.0, std_input=1.0, mean_target=np.zeros(2), std_target=np.ones(2))
    return InputStackTiledPred(smooth(shape, seed), patch, nd, grid_size=grid)


@functools.lru_cache(maxsize=None)
def stack32():
    s = stack((2, 40, 57), 32, 16)
    assert s.plan.total == 12
    return s


def run(smp, x, solver, **kw):
    if solver:
        smp.solver_sample_loop(x, **solver, **kw)
    else:
        smp.super_resolution(x, **kw)
    return smp.last_full_batch.clone()


class Source:
    """A noise_source that hands out the given draws in order."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __call__(self, shape):
        z = self.draws.pop(0)
        assert tuple(z.shape) == tuple(shape)
        return z


def stochastic_steps(smp, solver):
    """The steps s of one loop that add noise (each takes draw s + 1)."""
    if solver:
        sigma = smp.solver_table(**solver).sigma
        return [s for s in range(len(sigma)) if sigma[s] != 0]
    return list(range(smp.num_timesteps - 1))                          # sr3: none at the last step


def restated_field(smp, stack, solver, batch, id_base=0, C_state=2, reverse=True):
    """The prediction tile by tile with ``noise_source`` set to the crops of the field: draw 0 for the initial state,
    draw s + 1 for every step s that adds noise; the batches from the last to the first."""
    plan = stack.plan
    steps = stochastic_steps(smp, solver)
    starts = list(range(0, plan.total, batch))
    tiles = {}
    try:
        for i in (reversed(starts) if reverse else starts):
            chunk = list(range(i, i + batch))
            smp.noise_source = Source([crops(plan, chunk, C_state, SEED, d, id_base) for d in [0] + [s + 1 for s in steps]])
            tiles[i] = run(smp, stack.tiles(chunk)["input"], solver)
            assert not smp.noise_source.draws                          # every draw was asked for, in this order
    finally:
        smp.noise_source = None
    return torch.cat([tiles[i] for i in starts])


def numpy_item(ch0, ch1, loc, p, nd, w, from_norm_target):
    """SplitDataset.__getitem__ (data/split_dataset.py:237-278) restated with numpy for one patch at ``loc`` = (frame, y,
    x); ``p``: the patch side, or (ph, pw)."""
    n, y, x = loc
    ph, pw = (p, p) if np.isscalar(p) else p
    patch1 = ch0[n, y:y + ph, x:x + pw].astype(np.float32)[None]
    patch2 = ch1[n, y:y + ph, x:x + pw].astype(np.float32)[None]
    target = np.concatenate([patch1, patch2], axis=0)
    target = ((target - nd["mean_target"].reshape(-1, 1, 1)) / nd["std_target"].reshape(-1, 1, 1)).astype(np.float32)
    if from_norm_target:
        inp = np.float32(w[0]) * target[0:1] + np.float32(w[1]) * target[1:2]
    else:
        inp = np.float32(w[0]) * patch1 + np.float32(w[1]) * patch2
        assert inp.dtype == np.float32
        inp = ((inp.astype(np.float64) - np.float64(nd["mean_input"])) / np.float64(nd["std_input"])).astype(np.float32)
    return {"input": inp, "target": target}


def welford(xs):
    """include/dsx.h, dsx_moments_update / dsx_moments_finish restated in float64, one rounded operation at a time"""
    mean, m2 = xs[0].astype(np.float64), np.zeros(xs[0].shape)
    for r in range(1, len(xs)):
        x = xs[r].astype(np.float64)
        d = x - mean
        mean = mean + d / (r + 1)
        m2 = m2 + d * (x - mean)
    return mean.astype(np.float32), np.sqrt(m2 / (len(xs) - 1)).astype(np.float32)


def seam_rms(plan, tiles):
    """RMS difference of every horizontally adjacent pair of UNCROPPED tiles over the strip of 8 pixels on either side of
    their crop line (where the stitched frame changes from one tile to the other)."""
    N, H, W = plan.data_shape
    d = []
    for i in range(plan.total - 1):
        (n0, y0, x0), (n1, y1, x1) = (tuple(int(v) for v in plan.patch_start[k]) for k in (i, i + 1))
        if (n0, y0) != (n1, y1):
            continue                                                  # the last tile of a row of tiles
        line = int(plan.grid_start[i + 1][2])
        a, b = line - x0, line - x1
        d.append(tiles[i][:, :, a - 8:a + 8] - tiles[i + 1][:, :, b - 8:b + 8])
    d = np.stack(d).astype(np.float64)
    assert d.shape[1:] == (2, plan.patch_shape[1], 16)
    return float(np.sqrt((d ** 2).mean())), len(d)


# ----------------------------------------------------------------------------- frame diffusion, restated on the host
def frame_field(plan, Cn, seed, draw, id_base=0):
    """the noise fields of the plan's frames in the state's layout (N, H, W, C), from the sample streams"""
    from diffsplitting_amd import engine
    N, H, W = plan.data_shape
    z = engine.randn_samples((N, Cn, H, W), seed, [id_base + n for n in range(N)], draw)
    return np.ascontiguousarray(z.permute(0, 2, 3, 1).cpu().numpy())


def children(netG):
    if hasattr(netG, "indi1"):
        return [(netG.indi1, 0.5, 0), (netG.indi2, 1 - 0.5, netG.STREAM2_BIT)]
    return [(netG, 1.0, 0)]


def input_frames(stack):
    """the crop-paste of the stack's own input tiles, with numpy"""
    plan = stack.plan
    tiles = stack.tiles(list(range(plan.total)))["input"].cpu().numpy()
    out = np.full(plan.data_shape + (tiles.shape[1],), np.nan, dtype=np.float32)
    for t, (n, y, x, h, w, ry, rx, _) in enumerate(plan.regions):
        out[n, y:y + h, x:x + w] = tiles[t][:, ry:ry + h, rx:rx + w].transpose(1, 2, 0)
    assert np.isfinite(out).all()
    return out


def restated_child(child, stack, x_in, n, t0, batches, id_base, window, keep_rows=None):
    """One child's frame state row by row: the state on the host, tiles cut with numpy, one UNet forward per batch (the
    batches from the last to the first; ``batches`` = (ids, entries kept from the end)), the row's blend and step on the
    host by tests/blend_step_ref.py with the noise from the sample streams."""
    from diffsplitting_amd import engine
    plan = stack.plan
    copies = child.out_channel // x_in.shape[-1]
    X = np.concatenate([x_in] * copies, axis=-1)
    Cn = X.shape[-1]
    scale = child.e * torch.Tensor([t0])                                # InDISampler._start
    X = (torch.from_numpy(X) + torch.from_numpy(frame_field(plan, Cn, SEED, 0, id_base)) * scale).numpy()
    table = engine.indi_step_table(n, t0, child.e)
    win = blend_ref.window_pair(plan, window)
    for s in range(n):
        cut = blend_ref.cut_tiles(plan, X)
        x0t = np.full((plan.total, Cn) + plan.patch_shape[1:], np.nan, dtype=np.float32)
        for chunk, keep in reversed(batches):
            x0 = child.denoise_fn(torch.from_numpy(cut[chunk]).cuda(), torch.Tensor([float(table.tcond[s])]).cuda())
            x0t[chunk[-keep:]] = x0.cpu().numpy()[-keep:]
        if keep_rows is not None:
            keep_rows.append(x0t)
        sg = float(table.sigma[s])
        Z = frame_field(plan, Cn, SEED, s + 1, id_base) if sg != 0 else None
        X = blend_step_ref(plan, x0t, *win, X, float(table.c1[s]), float(table.c2[s]), sg, Z)
    return X


def restated_frames(netG, stack, n, batches, r=0, window="triangle"):
    x_in = input_frames(stack)
    N = stack.plan.data_shape[0]
    return np.concatenate([restated_child(child, stack, x_in, n, t0, batches, r * N + bit, window)
                           for child, t0, bit in children(netG)], axis=-1)


# ----------------------------------------------------------------------------- split, end to end
def split_runs(tmp_path, runs, extra=()):
    """fresh `split` processes at once on the tiny sr3 config (TINY, SCHED) -> the bytes of every --out"""
    cfg = {"name": "tiny_sr3", "phase": "val", "gpu_ids": [0],
           "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
           "datasets": {"patch_size": 32, "max_qval": 0.98, "upper_clip": False, "train": {"name": "Hagen"},
                        "val": {"name": "Hagen"}},
           "model": {"which_model_G": "sr3", "loss_type": "l1", "finetune_norm": False,
                     "unet": {"in_channel": 3, "out_channel": 2, "inner_channel": 16, "norm_groups": 16,
                              "channel_multiplier": [1, 2], "attn_res": [], "res_blocks": 1, "dropout": 0},
                     "beta_schedule": {"train": SCHED, "val": SCHED},
                     "diffusion": {"image_size": 32, "channels": 2, "conditional": True}}}
    cfg_path = str(tmp_path / "tiny_sr3.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "diffsplitting_amd.split", "-c", cfg_path, "-p", "val", "-gpu", "0", "--synthetic", "1,64,64",
            "--solver", "dpmpp2m", "--solver-steps", "4", "--sample-seed", "3", "--batch-tiles", "3"] + list(extra)
    procs = {}
    for name, flags in runs.items():
        root = tmp_path / name
        root.mkdir()
        procs[name] = subprocess.Popen(base + flags + ["-rootdir", str(root), "--out", str(root / "pred.npy")], env=env,
                                       cwd=str(root), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for name, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-3000:])
    pred = np.load(tmp_path / next(iter(runs)) / "pred.npy")
    assert pred.shape == (1, 64, 64, 2) and pred.dtype == np.float32 and np.isfinite(pred).all()
    return {name: open(tmp_path / name / "pred.npy", "rb").read() for name in runs}
