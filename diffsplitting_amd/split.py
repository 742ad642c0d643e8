#!/usr/bin/env python3
"""``split.py`` — the reference's entry point (split.py:75-85 flags) for the
validation / tiled-prediction path on MI355X:

    python -m diffsplitting_amd.split -c config/splitting_hagen_indi.json -p val -gpu 0
    torchrun --nproc-per-node 8 -m diffsplitting_amd.split -c <config> -p val -gpu 0,1,2,3,4,5,6,7

The config file is consumed unchanged (JSON with // comments).  Frames come
from the config's own ``datasets.{train,val}.datapath`` stacks with
``--datapath`` (``get_datasets``: the validation set normalised with the
training stack's statistics, ``--norm-from val`` for users who hold no training
data), from ``--frames <file.npy|.tif>`` ((N,H,W,2) raw channels), or are
synthesised.  ``--out FILE`` (.npy / .tif) writes the stitched prediction in raw
counts.  ``-p train`` is refused: the engine is inference-only.  ``--validate [--results DIR]`` runs the training
loop's validation report instead (core/validation.py): ``# Validation # PSNR``
of the first 19 non-tiled items (``--items N`` for another count), and with ``--results`` the three images per item.

A ``cifar10`` config with ``--datapath`` reads the pickle batches of its ``datapath`` directories (data/cifar10.py).
Colour items are not tiled: the run IS the validation report, over the whole validation set unless ``--items`` says
otherwise, ``--batch-tiles`` items at a time; ``--results DIR`` writes the RGB triples and ``--out FILE.npy`` the
predictions (N, 2 Cc, p, p) float32 in raw counts.

A ``joint_indi`` config with ``--mix-t T`` runs the mixed-input prediction instead (``predict_tiled_mixed``, BASELINE
C5): the two channels of every tile mixed at ``T``, ``indi1`` / ``indi2`` started at the time the TimePredictor of
``--time-predictor CONFIG [--time-predictor-checkpoint PTH]`` estimates per tile (``--t-from given``: at ``T`` itself,
no classifier), ``--mmse N`` repeats averaged.  Frames, ranks and ``--out`` as for the plain prediction.
``--t-from refined [--refine-rounds R] [--refine-scope tile|frame|set] [--refine-step S]`` re-estimates the start times
from the split's own channel estimates (``predict_tiled_refined``: the scan of core/psnr_based_t_refinement.py, which
needs no ground truth) and splits again, R times (default 1); round 0 starts at the TimePredictor's estimate when
``--time-predictor`` is given, else at 0.5.  Rank 0 logs what every round chose.

``--sample-seed S`` draws every tile's noise from its own stream (seed S, sample id = tile id; MMSE repeat ``r`` of the
mixed-input prediction: tile id + r * tiles): the noise does not depend on ``--batch-tiles`` or ``--gpus``, and neither
does the prediction for an equal batch size.  Off by default.

``--input FILE`` splits a stack that has no ground truth: a ``.tif`` / ``.npy`` (N,H,W) acquisition in which the two
structures are already superimposed (``data/input_stack.py``; uint8 / uint16 stacks stay on the device in their file
width).  Its normalisation comes from ``--norm FILE``, written by ``--save-norm FILE`` of a run that had the channels
(``--datapath``: the training stack's statistics; ``--frames``): ``data/normalization.py``.  ``--input-clip V`` clips the
counts of the sum first.  ``--samples N`` draws N posterior samples per tile and writes their mean to ``--out``;
``--std-out FILE`` the per-pixel spread in raw counts (``std * std_target``).  Both also apply to the plain two-channel
prediction, where the PSNR of the mean shows what averaging buys.  Repeat ``r`` of tile ``k`` draws from sample id
``k + r * tiles`` under ``--sample-seed``.

An ``sr3`` / ``ddpm`` config (the reference's ``config/splitting.json``) runs its full ancestral loop per batch of tiles;
``--solver {ddim,dpmpp2m} --solver-steps K [--eta E] [--spacing uniform|logsnr]`` samples with a few-step solver over
the trained schedule instead (``model/solvers.py``).  ``--noise-field`` (needs ``--sample-seed S``) cuts every tile's noise
from one field per frame -- a draw is a function of (seed, frame, draw ordinal, channel, y, x) -- so that overlapping
tiles share the noise of their overlap; posterior sample ``r`` draws from the fields ``r * frames + frame``.

``--stitch blend [--window triangle|hann]`` overlap-adds the whole predicted tiles under a separable window instead of
pasting every tile's inner region (``--stitch crop``, the default); it works for every sampler.  ``--fuse-steps`` (with
``--solver``, ``--sample-seed S`` and ``--noise-field``, one rank) diffuses every frame as one state: after every solver
row the tiles are blended on a frame canvas and cut out again.

``--frame-steps`` (an ``indi`` / ``joint_indi`` config with ``--sample-seed S``; any number of ranks) is frame diffusion
for the InDI family (``predict_stack_frames``): every frame is one state, and a step of it is one kernel that blends
the tiles' UNet outputs and applies the InDI update with the frame's noise field.  ``--samples``, ``--std-out``,
``--window`` and ``--out`` work as with ``--stitch blend``.

``--ms-ssim`` also scores the stitched prediction with the range-invariant multi-scale SSIM
(``core.metrics.calculate_msssim``, five scales): rank 0 logs mean +- standard error over the frames per channel.  It
needs a ground truth (not with ``--input``, ``--validate`` or colour items) and frames of 176 x 176 or more.

``--calibration FILE [--calibration-bins K]`` (with ``--samples N``, N >= 2, and a ground truth) asks whether the spread
tracks the real error (``core/calibration.py``): rank 0 bins the pixels of the stitched canvases by predicted std, logs
per channel the scale, the line ``rmse ~ a rmv + c`` and the coverage at z = 1, 2, 3, and writes curve and fit to FILE.
``--apply-calibration FILE`` (with ``--std-out``) writes ``a std + c`` (clamped at 0) instead of the raw spread, for a
stack without ground truth (``--input``); the file must hold the prediction's channel count and ``--samples``.

``--quantiles Q1,Q2,.. --quantile-out FILE`` (with ``--samples N``, 2 <= N <= 64) writes the per-pixel quantiles of the N
posterior samples (``predict_stack(quantiles=)``: the median, a credible band) in raw counts, (Q,N,H,W,C) as .npy or
Q * N * C pages as .tif; with ``--stitch blend`` outside the frame-state paths a map is a blend of per-tile quantiles.
``--rank-histogram FILE.json`` (with a ground truth) counts per channel the rank of the ground truth among the samples of
every pixel (``core.calibration.rank_histogram``): uniform counts mean calibrated bands, whatever the posterior's shape;
rank 0 logs the observed against the nominal coverage of the widest central band and of the one nearest 50 %.

``--seam-report FILE.json [--seam-map FILE.npy|.tif] [--seam-band B]`` measures how far the predicted tiles disagree where
they overlap (``predict_stack(disagreement=)``, ``TilePlan.disagreement``; no ground truth needed): per channel the RMS
pairwise difference over every overlap and over the band of B pixels (default 8) around the crop lines, and the largest
per-pixel spread, in normalised units and in raw counts; ``--seam-map`` writes the per-pixel spread among the tiles in raw
counts, laid out as ``--std-out``.  It measures the per-tile means of the ``--samples``, or with ``--fuse-steps`` /
``--frame-steps`` the x0 tiles of the last row (``--seam-map`` then needs ``--samples 1``).

``--consistency-report FILE.json [--consistency-map FILE.npy|.tif] [--project] [--consistency-noise RHO]
[--channel-weights W0,W1]`` (all need ``--input``) ask whether the split adds back up to the acquisition
(``core/consistency.py``): the residual ``r = x - sum_c w_c p_c`` in raw counts, with the weights of the norm file's
``channel_weights`` (else ones).  Rank 0 logs rms, bias, relative residual and saturated share, with ``--samples N >= 2``
also the ``chi2`` of the spread, and writes them per frame and in total to FILE; ``--consistency-map`` writes r (N,H,W),
laid out as ``--seam-map``.  ``--project`` conditions the posterior on the observation (noise ``RHO`` counts): ``--out``
and ``--std-out`` then hold the conditioned mean and spread; with ``--samples 1`` the projection is orthogonal
(``--std-out`` stays refused).  Order: the spread is first recalibrated by ``--apply-calibration`` where given, THEN it
weights the projection and the ``chi2``; ``--std-out`` writes the conditioned, recalibrated spread.  The report always
describes the prediction before the projection.  Quantile maps are not projected: ``--project`` with ``--quantile-out`` is
refused.
"""
import argparse
import functools
import logging
import os
import sys
import time

import numpy as np
import torch

from . import parallel
from .core import logger as Logger
from ._lib import DsxError
from .data.split_dataset import DataLocation, SplitDataset, SplitDatasetTiledPred
from .data.tiled_predict import TileExchange
from .model import create_model


def get_datasets(opt, tiled_pred=False, norm_from="train", device="cuda"):
    """The reference's ``get_datasets(opt, tiled_pred)`` (split.py:30-71) -> (train_set, val_set): locations from
    ``datasets.{train,val}.datapath.{ch0,ch1}``; ``patch_size``, ``max_qval``, ``upper_clip``, ``channel_weights``,
    ``target_channel_idx`` and ``uncorrelated_channels`` read as there; the validation set normalised with the
    TRAINING stack's statistics.  The training set is built with ``enable_transforms=False`` and without random
    patching: this engine does not train, the set is there for its statistics only.  ``tiled_pred`` gives
    ``SplitDatasetTiledPred`` with grid = patch // 2 over the validation stack's actual shape (the reference
    hard-codes (10, 2048, 2048)).  ``norm_from="val"`` takes the statistics from the validation stack itself;
    ``train_set`` is then None."""
    ds = opt["datasets"]
    patch_size = ds["patch_size"]
    target_channel_idx = ds.get("target_channel_idx", None)
    upper_clip = ds.get("upper_clip", None)
    max_qval = ds["max_qval"]
    channel_weights = ds.get("channel_weights", None)
    data_type = _data_type(ds, norm_from)
    assert data_type in ["cifar10", "Hagen"]
    if norm_from not in ("train", "val"):
        raise DsxError(f"norm_from = {norm_from!r}: 'train' or 'val'")
    if data_type == "cifar10":
        loc = lambda part: _cifar_location(ds, part, norm_from)
    else:
        loc = lambda part: DataLocation(channelwise_fpath=(ds[part]["datapath"]["ch0"], ds[part]["datapath"]["ch1"]))
    common = dict(target_channel_idx=target_channel_idx, max_qval=max_qval, upper_clip=bool(upper_clip),
                  channel_weights=channel_weights, enable_transforms=False, random_patching=False,
                  input_from_normalized_target=opt["model"]["which_model_G"] == "joint_indi", device=device)
    train_set, nd = None, None
    if norm_from == "train":
        train_set = SplitDataset(data_type, loc("train"), patch_size, normalization_dict=None,
                                 uncorrelated_channels=bool(ds["train"].get("uncorrelated_channels")), **common)
        nd = train_set.get_normalization_dict()
    if tiled_pred:
        val_set = SplitDatasetTiledPred(data_type, loc("val"), patch_size, grid_size=patch_size // 2,
                                        normalization_dict=nd, **common)
    else:
        val_set = SplitDataset(data_type, loc("val"), patch_size, normalization_dict=nd, **common)
    return train_set, val_set


def _data_type(ds, norm_from="train"):
    return ((ds.get("train") if norm_from == "train" else ds.get("train") or ds.get("val")) or {}).get("name")


def _config_once(path):
    """-> ``config()``: (``model.which_model_G``, the ``datasets`` dict) of the configuration file, for the flag checks.
    The file is read at the first call and only then: a run whose flags ask nothing of it does not open it here."""
    @functools.lru_cache(maxsize=None)
    def config():
        cfg = Logger.load_json(path)
        return (cfg.get("model") or {}).get("which_model_G"), cfg.get("datasets") or {}
    return config


def _cifar_location(ds, part, norm_from):
    """``datasets.<part>.datapath`` of a cifar10 config: a directory of pickle batches (split.py:37-38, 53-54)."""
    path = (ds[part] or {}).get("datapath")
    if not isinstance(path, str) or not path:
        raise DsxError(f"data_type 'cifar10': datasets.{part}.datapath must name a directory of CIFAR-10 batch files, "
                       f"got {path!r}")
    if not os.path.isdir(path):
        hint = ""
        if part == "train" and norm_from == "train":
            hint = ("; the statistics of uint8 data depend on the plane count and the channel weights only, so "
                    "--norm-from val (norm_from='val') gives the same numbers without the training directory")
        raise DsxError(f"data_type 'cifar10': datasets.{part}.datapath = {path} is not a directory{hint}")
    return DataLocation(directory=path)


def _read_frames(path):
    """--frames: (N,H,W,2) raw channels from .npy or .tif, as fp32."""
    if str(path).endswith((".tif", ".tiff")):
        from .data.tiff import imread
        frames = imread(path)
        if frames.ndim != 4 or frames.shape[-1] != 2:
            raise DsxError(f"--frames {path}: (N,H,W,2) expected, the file holds {frames.shape}")
        return frames.astype(np.float32)
    return np.load(path, allow_pickle=False).astype(np.float32)


def _target_stats(val_set, channels):
    """(mean_target, std_target), float64, of the ``channels`` channels a prediction of ``val_set`` holds."""
    nd = val_set.get_normalization_dict()
    idx = val_set._target_channel_idx
    mean, std = (np.asarray(nd[k], dtype=np.float64).reshape(-1) for k in ("mean_target", "std_target"))
    if idx is not None:
        mean, std = mean[idx:idx + 1], std[idx:idx + 1]
    if mean.size != channels:
        raise DsxError(f"--out: the prediction has {channels} channels, the dataset normalises {mean.size}")
    return mean, std


def _write_prediction(path, pred, val_set, spread=False):
    """--out: the stitched prediction (N,H,W,C), un-normalised to raw counts with the dataset's mean_target /
    std_target, as .npy (N,H,W,C) float32 or as a .tif hyperstack of N * C float32 pages (frame-major).  ``spread``
    (--std-out): a per-pixel standard deviation, scaled by std_target with no mean added."""
    C_out = pred.shape[-1]
    mean, std = _target_stats(val_set, C_out)
    mean_t = torch.as_tensor(mean, dtype=torch.float32, device=pred.device)
    std_t = torch.as_tensor(std, dtype=torch.float32, device=pred.device)
    raw = ((pred * std_t) if spread else (pred * std_t + mean_t)).cpu().numpy()
    if str(path).endswith(".npy"):
        np.save(path, raw)
    elif str(path).endswith((".tif", ".tiff")):
        from .data.tiff import imwrite
        N, H, W, _ = raw.shape
        desc = (f"ImageJ=1.11a\nimages={N * C_out}\nchannels={C_out}\nframes={N}\nhyperstack=true\nmode=grayscale\n")
        imwrite(path, np.ascontiguousarray(raw.transpose(0, 3, 1, 2)).reshape(N * C_out, H, W), description=desc)
    else:
        raise DsxError(f"--out {path}: .npy or .tif")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True, help="JSON file for configuration")
    ap.add_argument("-p", "--phase", type=str, choices=["train", "val"], default="val")
    ap.add_argument("-gpu", "--gpu_ids", type=str, default="0")
    ap.add_argument("-debug", "-d", action="store_true")
    ap.add_argument("-enable_wandb", action="store_true")
    ap.add_argument("-rootdir", type=str, default=".")
    ap.add_argument("--frames", type=str, default=None, help=".npy or .tif with (N,H,W,2) raw channel frames")
    ap.add_argument("--datapath", action="store_true",
                    help="read the frames from the config's datasets.{train,val}.datapath stacks (get_datasets)")
    ap.add_argument("--norm-from", type=str, choices=["train", "val"], default="train",
                    help="with --datapath: the stack whose statistics normalise the validation set")
    ap.add_argument("--out", type=str, default=None, help="write the stitched prediction in raw counts (.npy / .tif)")
    ap.add_argument("--synthetic", type=str, default="2,512,512", help="N,H,W of synthetic frames")
    ap.add_argument("--steps", type=int, default=None, help="override beta_schedule.val.n_timestep")
    ap.add_argument("--batch-tiles", type=int, default=8)
    ap.add_argument("--dtype", type=str, default=None, choices=["f32", "bf16", "f16"])
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks to run (one process per GPU); default: the number of ids in -gpu.  Without a "
                         "launcher (torchrun) the ranks are started here")
    ap.add_argument("--validate", action="store_true",
                    help="the training loop's validation report (split.py:163-257) instead of the tiled prediction")
    ap.add_argument("--results", type=str, default=None, help="with --validate: directory for the image triples")
    ap.add_argument("--items", type=int, default=None,
                    help="items the validation report scores: default 19 with --validate, the whole validation set "
                         "for a cifar10 config with --datapath")
    ap.add_argument("--mix-t", type=float, default=None,
                    help="joint_indi only: the mixed-input prediction (predict_tiled_mixed) at this mixing weight")
    ap.add_argument("--time-predictor", type=str, default=None, help="with --mix-t: the TimePredictor's JSON configuration")
    ap.add_argument("--time-predictor-checkpoint", type=str, default=None, help="its state_dict file")
    ap.add_argument("--mmse", type=int, default=None, help="with --mix-t: repeats averaged per tile (default 1)")
    ap.add_argument("--t-from", type=str, choices=["classifier", "given", "refined"], default=None,
                    help="with --mix-t: start times from the TimePredictor (default), --mix-t itself, or re-estimated "
                         "from the split's own channel estimates (predict_tiled_refined; --time-predictor optional)")
    ap.add_argument("--refine-rounds", type=int, default=None,
                    help="with --t-from refined: how often the start times are re-estimated and the tiles split again "
                         "(default 1; 0 scores the first split only)")
    ap.add_argument("--refine-scope", type=str, choices=["tile", "frame", "set"], default=None,
                    help="with --t-from refined: the tiles whose curves are averaged before the argmax (default frame)")
    ap.add_argument("--refine-step", type=float, default=None,
                    help="with --t-from refined: spacing of the scanned mixing times np.arange(0, 1, S) (default 0.05)")
    ap.add_argument("--sample-seed", type=int, default=None,
                    help="per-sample noise streams: every tile draws from the stream (seed, tile id), whatever batch "
                         "or rank predicts it (default: off, one stream per step over the batch)")
    ap.add_argument("--input", type=str, default=None,
                    help=".tif or .npy with one (N,H,W) stack in which the two structures are already superimposed "
                         "(no ground truth); needs --norm")
    ap.add_argument("--norm", type=str, default=None, help="with --input: the normalisation file (--save-norm)")
    ap.add_argument("--input-clip", type=float, default=None, help="with --input: clip the counts at this value first")
    ap.add_argument("--save-norm", type=str, default=None,
                    help="with --datapath or --frames: write the normalisation the validation set uses to this file")
    ap.add_argument("--samples", type=int, default=None,
                    help="posterior samples per tile of the tiled prediction; --out holds their mean (default 1)")
    ap.add_argument("--std-out", type=str, default=None,
                    help="write the per-pixel spread over --samples >= 2 samples in raw counts (.npy / .tif)")
    ap.add_argument("--solver", type=str, default=None, choices=["ddim", "dpmpp2m"],
                    help="sr3 / ddpm configs: sample every batch of tiles with this few-step solver over "
                         "--solver-steps timesteps of the trained schedule (default: the full ancestral loop)")
    ap.add_argument("--solver-steps", type=int, default=None, help="with --solver: how many timesteps")
    ap.add_argument("--eta", type=float, default=None, help="with --solver ddim: stochasticity in [0, 1] (default 0)")
    ap.add_argument("--spacing", type=str, default=None, choices=["uniform", "logsnr"],
                    help="with --solver: how the timesteps are spaced (default: logsnr for dpmpp2m, uniform for ddim)")
    ap.add_argument("--noise-field", action="store_true",
                    help="with --sample-seed: cut every tile's noise from one field per frame (seed, frame, draw, "
                         "channel, y, x), so that overlapping tiles share the noise of their overlap")
    ap.add_argument("--stitch", type=str, default=None, choices=["crop", "blend"],
                    help="how the predicted tiles become a frame: paste every tile's inner region (crop, the default) "
                         "or overlap-add whole tiles under --window (blend)")
    ap.add_argument("--window", type=str, default=None, choices=["triangle", "hann"],
                    help="with --stitch blend: the separable blend window (default triangle)")
    ap.add_argument("--fuse-steps", action="store_true",
                    help="with --solver, --sample-seed and --noise-field: diffuse every frame as one state -- after every "
                         "solver row the tiles are blended on a frame canvas and cut out again (implies --stitch blend)")
    ap.add_argument("--frame-steps", action="store_true",
                    help="indi / joint_indi configs with --sample-seed: diffuse every frame as one state -- per step the "
                         "tiles' UNet outputs are blended and the InDI update runs on the frame canvas, with the frame's "
                         "noise field (implies --stitch blend; any number of ranks)")
    ap.add_argument("--ms-ssim", action="store_true",
                    help="also score the stitched prediction with the range-invariant multi-scale SSIM "
                         "(core.metrics.calculate_msssim: five scales, frames of 176 x 176 or more)")
    ap.add_argument("--calibration", type=str, default=None,
                    help="with --samples N >= 2 and ground truth: score the spread against the real error "
                         "(core.calibration: RMV-RMSE bins, line fit, coverage) and write the calibration to this JSON file")
    ap.add_argument("--calibration-bins", type=int, default=None, help="with --calibration: equal-count bins (default 30)")
    ap.add_argument("--apply-calibration", type=str, default=None,
                    help="with --std-out: write the spread recalibrated by this file (a std + c per channel)")
    ap.add_argument("--quantiles", type=str, default=None,
                    help="with --samples N >= 2 and --quantile-out: 1 to 8 quantiles in [0, 1] of the posterior samples per "
                         "pixel, comma-separated (0.05,0.5,0.95)")
    ap.add_argument("--quantile-out", type=str, default=None,
                    help="with --quantiles: write the quantile maps in raw counts, (Q,N,H,W,C) .npy or a .tif of "
                         "Q * N * C pages (quantile-major)")
    ap.add_argument("--rank-histogram", type=str, default=None,
                    help="with --samples N >= 2 and ground truth: count the rank of the ground truth among the samples per "
                         "pixel (core.calibration.rank_histogram) and write histogram and band coverage to this .json file")
    ap.add_argument("--seam-report", type=str, default=None,
                    help="measure how far the predicted tiles disagree where they overlap (TilePlan.disagreement; needs no "
                         "ground truth) and write the scores to this .json file")
    ap.add_argument("--seam-map", type=str, default=None,
                    help="with --seam-report: write the per-pixel disagreement s in raw counts (.npy / .tif), laid out as "
                         "--std-out")
    ap.add_argument("--seam-band", type=int, default=None,
                    help="with --seam-report: half-width in pixels of the band around the crop lines (default 8)")
    ap.add_argument("--consistency-report", type=str, default=None,
                    help="with --input: how far the split is from adding back up to the acquisition "
                         "(core.consistency: rms, bias, relative residual, chi2 of the spread) to this .json file")
    ap.add_argument("--consistency-map", type=str, default=None,
                    help="with --input: write the residual x - sum_c w_c p_c (N,H,W) in raw counts (.npy / .tif)")
    ap.add_argument("--project", action="store_true",
                    help="with --input: condition mean and spread on the acquisition; --out / --std-out hold the result")
    ap.add_argument("--consistency-noise", type=float, default=None,
                    help="with --consistency-report / --project: the noise rho of the observation in raw counts (default 0)")
    ap.add_argument("--channel-weights", type=str, default=None,
                    help="with --consistency-report / --project: W0,W1 of x = W0 ch0 + W1 ch1 (default: the norm file's "
                         "channel_weights, else ones)")
    args = ap.parse_args(argv)
    config = _config_once(args.config)
    _check_consistency_args(args, config)
    _check_seam_args(args, config)
    _check_msssim_args(args, config)
    _check_calibration_args(args, config)
    _check_quantile_args(args, config)
    _check_solver_args(args, config)
    _check_stitch_args(args, len(str(args.gpu_ids).split(",")) if args.gpus is None else args.gpus)
    _check_frame_args(args, config)
    if args.sample_seed is not None and args.validate:
        raise SystemExit("--sample-seed names the tiles of a tiled prediction: not with --validate")
    if args.phase == "train":
        raise SystemExit("training is out of scope of the MI355X sampling engine; use -p val")
    if args.datapath and args.frames:
        raise SystemExit("--datapath and --frames both name the frames: give one")
    if args.out and not args.out.endswith((".npy", ".tif", ".tiff")):
        raise SystemExit("--out: a .npy or .tif file")
    if args.out and args.validate:
        raise SystemExit("--out writes the tiled prediction: not with --validate")
    _check_input_args(args, config)
    _check_mixed_args(args, config)
    n_ranks = args.gpus if args.gpus is not None else len(str(args.gpu_ids).split(","))
    if argv is None and parallel.needs_self_launch(n_ranks):
        # fresh child processes, started before anything here touches the GPU (never an exec after HIP init)
        raise SystemExit(parallel.self_launch(n_ranks, ["-m", "diffsplitting_amd.split"] + sys.argv[1:]))

    rank, world = parallel.init()
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING, format="%(asctime)s %(message)s")
    log = logging.getLogger("base")
    opt = Logger.parse(args)
    if args.dtype:
        opt["model"]["compute_dtype"] = args.dtype
    # colour items (cifar10) are not tiled: with --datapath the run is the validation report over the whole set
    colour = bool(args.datapath) and _data_type(opt["datasets"], args.norm_from) == "cifar10"
    if colour and args.out and not args.out.endswith(".npy"):
        raise SystemExit("--out: colour items are written as (N, 2 Cc, p, p) .npy; a .tif hyperstack holds grey frames")
    if args.items is not None and args.items < 1:
        raise SystemExit("--items: a positive count")
    if colour and args.sample_seed is not None:
        raise SystemExit("--sample-seed names the tiles of a tiled prediction: colour items are not tiled")
    if colour and args.mix_t is not None:
        raise SystemExit("--mix-t: the mixed-input prediction takes two grey channels, not a cifar10 config")
    # -gpu selects the device(s): rank r of a torchrun launch drives gpu_ids[r] (the reference exports
    # CUDA_VISIBLE_DEVICES=gpu_ids instead, core/logger.py:59-65; mapping the index keeps one process per GPU
    # working without touching the environment after HIP may have been initialised)
    ids = list(opt["gpu_ids"] or [0])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(ids[local % len(ids)])
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.backends.cudnn.benchmark = True

    diffusion = create_model(opt)
    diffusion.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    netG = diffusion.netG
    n_steps = args.steps or opt["model"]["beta_schedule"]["val"]["n_timestep"]

    dsopt = opt["datasets"] or {}
    which = opt["model"]["which_model_G"]
    if args.input:
        from .data.input_stack import InputStackTiledPred, read_stack
        from .data.normalization import load_normalization
        nd, _ = load_normalization(args.norm)
        stack = read_stack(args.input)
        patch = min(_config_patch(dsopt), stack.shape[1], stack.shape[2])
        val_set = InputStackTiledPred(stack, patch, nd, grid_size=patch // 2,
                                      target_channel_idx=dsopt.get("target_channel_idx"), input_clip=args.input_clip,
                                      device=dev)
        return _predict(args, netG, val_set, n_steps, patch, rank, world, dev, log)
    if args.datapath:
        _, val_set = get_datasets(opt, tiled_pred=not (args.validate or colour), norm_from=args.norm_from, device=dev)
        _save_norm(args, val_set, dsopt, _data_type(dsopt, args.norm_from), rank, log)
        if args.validate or colour:
            return _run_validate(args, opt, diffusion, val_set, log, whole_set=colour)
        if args.mix_t is not None:
            return _predict_mixed(args, netG, val_set, n_steps, int(dsopt["patch_size"]), rank, world, log)
        return _predict(args, netG, val_set, n_steps, int(dsopt["patch_size"]), rank, world, dev, log)
    if args.frames:
        frames = _read_frames(args.frames)
    else:
        n, h, w = (int(v) for v in args.synthetic.split(","))
        rng = np.random.default_rng(0)
        frames = (rng.random((n, h, w, 2), dtype=np.float32) * 1000.0).astype(np.float32)    # raw detector counts
        log.info("no --frames given: using synthetic frames %s", frames.shape)
    # the validation dataset of split.get_datasets(opt, tiled_pred=True) (reference split.py:30-71) with the frames
    # resident on the GPU: quantile normalisation (compute_normalization_dict), ShiftBoundary tiling, normalised
    # tile batches cut by one HIP launch
    patch = min(_config_patch(dsopt), frames.shape[1], frames.shape[2])
    common = dict(target_channel_idx=dsopt.get("target_channel_idx"), max_qval=dsopt.get("max_qval") or 0.98,
                  upper_clip=bool(dsopt.get("upper_clip")), channel_weights=dsopt.get("channel_weights"),
                  enable_transforms=False, random_patching=False, input_from_normalized_target=(which == "joint_indi"),
                  device=dev)
    location = DataLocation(arrays=(frames[..., 0], frames[..., 1]))
    val_set = SplitDatasetTiledPred("Hagen", location, patch, grid_size=patch // 2, **common)
    if args.frames:
        _save_norm(args, val_set, dsopt, "Hagen", rank, log)
    if args.validate:
        # the non-tiled dataset of the same frames with the same normalisation (split.get_datasets without tiled_pred)
        items = SplitDataset("Hagen", location, patch, normalization_dict=val_set.get_normalization_dict(), **common)
        return _run_validate(args, opt, diffusion, items, log)
    if args.mix_t is not None:
        return _predict_mixed(args, netG, val_set, n_steps, patch, rank, world, log)
    return _predict(args, netG, val_set, n_steps, patch, rank, world, dev, log)


def _config_patch(dsopt):
    """The patch size of the config: ``datasets.val.patch_size``, else ``datasets.patch_size``, else 512."""
    patch = (dsopt["val"] or {}).get("patch_size") if dsopt.get("val") else None
    return int(patch or dsopt.get("patch_size") or 512)


def _save_norm(args, val_set, dsopt, data_type, rank, log):
    """``--save-norm``: rank 0 writes the dict ``val_set`` is normalised with (data/normalization.py)."""
    if not args.save_norm or rank != 0:
        return
    from .data.normalization import save_normalization
    save_normalization(args.save_norm, val_set.get_normalization_dict(), data_type=data_type,
                       channel_weights=dsopt.get("channel_weights"), max_qval=dsopt.get("max_qval") or 0.98,
                       upper_clip=bool(dsopt.get("upper_clip")), target_channel_idx=dsopt.get("target_channel_idx"))
    log.info("normalisation written to %s", args.save_norm)


def _predict(args, netG, val_set, n_steps, patch, rank, world, dev, log):
    """The tiled prediction of ``val_set`` (two channels, or an input-only stack) over the ranks, ``--samples`` posterior
    samples per tile; rank 0 writes the mean to ``--out`` and the spread to ``--std-out``.  Returns the stitched mean."""
    from .data.tiled_predict import predict_stack
    samples = args.samples or 1
    solver = _solver_of(args)
    if args.ms_ssim:
        _msssim_size_or_exit(*val_set._data_shape[-2:])              # before any tile is predicted
    if hasattr(netG, "solver_sample_loop"):
        # a Gaussian sampler runs its trained schedule: --steps does not shorten it, --solver does
        n_steps = solver["steps"] if solver else netG.num_timesteps
        if rank == 0 and solver:
            log.info("sr3 / ddpm: %s over %d of the %d trained timesteps per batch of tiles", solver["solver"], n_steps,
                     netG.num_timesteps)
        elif rank == 0:
            log.info("sr3 / ddpm without --solver: the full ancestral loop, %d steps per batch of tiles", n_steps)
    cons = _consistency_wanted(args)
    want_std = bool(args.std_out or args.calibration or (cons and samples > 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # every rank holds the frames: the ground truth needs no tiles and no collective; the metric is accumulated while
    # pasting, and the path's only collectives are the cropped tiles of each output canvas
    if args.frame_steps:
        from .data.tiled_predict import predict_stack_frames
        out, plan = predict_stack_frames(netG, val_set, batch_tiles=args.batch_tiles, num_timesteps=n_steps,
                                         samples=samples, return_std=want_std,
                                         seed=args.sample_seed, window=args.window or "triangle", **_quantile_kwargs(args),
                                         **_seam_kwargs(args))
    else:
        out, plan = predict_stack(netG, val_set, batch_tiles=args.batch_tiles, num_timesteps=n_steps, samples=samples,
                                  return_std=want_std, seed=args.sample_seed, solver=solver,
                                  noise="field" if args.noise_field else "samples", stitch=args.stitch,
                                  window=args.window or "triangle", fuse=args.fuse_steps, **_quantile_kwargs(args),
                                  **_seam_kwargs(args))
    pred, ps = out["mean"], out.get("psnr")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rank == 0:
        log.info("tiled prediction: %d tiles of %d^2, %d steps, %d GPU(s): %.3f s (%.1f tiles/s)",
                 plan.total, patch, n_steps, world, dt, plan.total / dt)
        if samples > 1:
            log.info("mean over %d posterior samples per tile", samples)
        if ps is not None:
            for c in range(ps.shape[1]):
                log.info("channel %d: RangeInvariantPsnr %.2f +- %.2f dB (random-init weights unless a checkpoint "
                         "was given in path.resume_state)", c, ps[:, c].mean().item(),
                         ps[:, c].std().item() if ps.shape[0] > 1 else 0.0)
        _log_msssim(args, val_set, pred, ps, log)
        _log_calibration(args, val_set, pred, out.get("std"), ps, samples, log)
        spread = out.get("std")
        if args.apply_calibration:
            from .core.calibration import Calibration
            spread = Calibration.load(args.apply_calibration).apply(spread)
            log.info("spread recalibrated by %s", args.apply_calibration)
        if cons:
            # the recalibrated spread, where there is one, weights the projection and the chi2
            pred, spread = _run_consistency(args, val_set, pred, spread if samples > 1 else None, log)
        if args.out:
            _write_prediction(args.out, pred, val_set)
            log.info("prediction written to %s", args.out)
        if args.std_out:
            _write_prediction(args.std_out, spread, val_set, spread=True)
            log.info("spread over %d samples written to %s", samples, args.std_out)
        if args.quantile_out:
            _write_quantiles(args.quantile_out, out["quantiles"], _parse_quantiles(args.quantiles), val_set)
            log.info("quantiles %s over %d samples written to %s", args.quantiles, samples, args.quantile_out)
        _log_rank_histogram(args, out.get("rank"), samples, log)
        _write_seam_report(args, out.get("disagreement"), val_set, plan, patch, samples, log)
    return pred


# ---- --consistency-report / --project: does the split add back up to the acquisition ------------------------------
def _consistency_wanted(args):
    return bool(args.consistency_report or args.consistency_map or args.project)


def _parse_weights(text):
    try:
        w = [float(v) for v in text.split(",")]
    except ValueError:
        raise SystemExit(f"--channel-weights {text}: W0,W1, two numbers")
    return w


def _check_consistency_args(args, config):
    """``--consistency-report`` / ``--consistency-map`` / ``--project`` / ``--consistency-noise`` / ``--channel-weights``,
    checked on the command line, the config and the norm file alone (nothing touches the GPU, no rank is started).
    Without them: nothing."""
    given = [flag for flag, value in (("--consistency-report", args.consistency_report),
                                      ("--consistency-map", args.consistency_map), ("--project", args.project),
                                      ("--consistency-noise", args.consistency_noise is not None),
                                      ("--channel-weights", args.channel_weights)) if value]
    if not given:
        return
    if not args.input:
        other = next((f for f, v in (("--datapath", args.datapath), ("--frames", args.frames)) if v), "synthetic frames")
        raise SystemExit(f"{given[0]}: only with --input FILE; the check compares a split with the acquisition it was "
                         f"made from, and {other} are two ground-truth channels, not an acquisition")
    if not _consistency_wanted(args):
        raise SystemExit(f"{given[0]}: only with --consistency-report, --consistency-map or --project")
    if args.consistency_report and not args.consistency_report.endswith(".json"):
        raise SystemExit(f"--consistency-report {args.consistency_report}: a .json file")
    if args.consistency_map and not args.consistency_map.endswith((".npy", ".tif", ".tiff")):
        raise SystemExit(f"--consistency-map {args.consistency_map}: a .npy or .tif file")
    rho = args.consistency_noise
    if rho is not None and not (np.isfinite(rho) and rho >= 0):
        raise SystemExit(f"--consistency-noise {rho}: rho in raw counts, finite and not negative")
    if args.project and args.quantile_out:
        raise SystemExit("--project with --quantile-out: quantile maps are not projected; write them in a run of their own")
    idx = config()[1].get("target_channel_idx")
    if idx is not None:
        raise SystemExit(f"{given[0]}: the config predicts one channel (target_channel_idx = {idx}); the sum "
                         "sum_c w_c p_c needs every summand")
    if args.channel_weights is not None:
        w = _parse_weights(args.channel_weights)
        if len(w) != 2:
            raise SystemExit(f"--channel-weights {args.channel_weights}: {len(w)} weights, the split has two channels: W0,W1")
        if not np.isfinite(w).all() or not any(w):
            raise SystemExit(f"--channel-weights {args.channel_weights}: finite, and not both zero")


def _consistency_weights(args):
    """--channel-weights, else the norm file's channel_weights, else None (ones)."""
    if args.channel_weights is not None:
        return _parse_weights(args.channel_weights)
    from .data.normalization import load_normalization
    return load_normalization(args.norm)[1].get("channel_weights")


def _run_consistency(args, val_set, pred, spread, log):
    """Rank 0, on the stitched canvases: report, map and, with ``--project``, the conditioned (mean, spread)."""
    import json
    from .core.consistency import consistency, json_report
    stack, pix, _, clip = val_set.acquisition()
    rep = consistency(pred, stack, val_set.get_normalization_dict(), weights=_consistency_weights(args), std=spread,
                      clip=clip, noise=args.consistency_noise or 0.0, project=args.project,
                      want_map=bool(args.consistency_map), pix=pix)
    tot = rep["total"]
    n_all = tot["pixels"] + tot["saturated"]
    fmt = lambda v: "n/a" if v is None else "%.6g" % v
    log.info("weights %s: residual x - sum w p: rms %s, bias %s counts, relative %s, saturated %.4f %% of %d pixels",
             rep["weights"], fmt(tot["rms"]), fmt(tot["bias"]), fmt(tot["relative"]), 100.0 * tot["saturated"] / n_all, n_all)
    if spread is not None:
        log.info("weights %s: chi2 %s over %d pixels (near 1: the spread of the sum is honest; well above: over-confident, "
                 "or the channels' errors are correlated; well below: the opposite)", rep["weights"], fmt(tot["chi2"]),
                 tot["chi2_pixels"])
    if args.consistency_report:
        doc = json_report(rep)
        doc["projected"] = bool(args.project)
        doc["spread"] = None if spread is None else ("recalibrated" if args.apply_calibration else "samples")
        with open(args.consistency_report, "w") as f:
            json.dump(doc, f, indent=1)
        log.info("consistency report written to %s", args.consistency_report)
    if args.consistency_map:
        _write_frames(args.consistency_map, rep["map"].cpu().numpy())
        log.info("residual map written to %s", args.consistency_map)
    if args.project:
        log.info("--out%s: conditioned on the acquisition (%s)", " / --std-out" if spread is not None else "",
                 "orthogonal projection" if spread is None and not args.consistency_noise else "Gaussian posterior")
        return rep["mean"], rep.get("std", spread)
    return pred, spread


def _write_frames(path, frames):
    """(N,H,W) float32 frames in raw counts as .npy or as a .tif of N pages."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    if str(path).endswith(".npy"):
        np.save(path, frames)
    else:
        from .data.tiff import imwrite
        imwrite(path, frames)


# ---- --seam-report: how far the predicted tiles disagree where they overlap ---------------------------------------
def _check_seam_args(args, config):
    """``--seam-report`` / ``--seam-map`` / ``--seam-band``, checked on the command line and the config alone (nothing
    touches the GPU, no rank is started).  Without them: nothing."""
    if not args.seam_report:
        for flag, value in (("--seam-map", args.seam_map), ("--seam-band", args.seam_band)):
            if value is not None:
                raise SystemExit(f"{flag}: only with --seam-report FILE.json")
        return
    if not args.seam_report.endswith(".json"):
        raise SystemExit(f"--seam-report {args.seam_report}: a .json file")
    if args.seam_map and not args.seam_map.endswith((".npy", ".tif", ".tiff")):
        raise SystemExit(f"--seam-map {args.seam_map}: a .npy or .tif file")
    if args.seam_band is not None and not 1 <= args.seam_band <= 65535:
        raise SystemExit(f"--seam-band {args.seam_band}: 1..65535 pixels")
    if args.validate:
        raise SystemExit("--seam-report measures the tiles of a tiled prediction: not with --validate")
    if args.mix_t is not None:
        raise SystemExit("--seam-report: not with --mix-t; the measure is not built for the mixed-input prediction")
    if args.datapath and _data_type(config()[1], args.norm_from) == "cifar10":
        raise SystemExit("--seam-report measures the tiles of a tiled prediction: the colour items of a cifar10 config are "
                         "not tiled")
    if args.seam_map and (args.fuse_steps or args.frame_steps) and (args.samples or 1) > 1:
        raise SystemExit(f"--seam-map with {'--fuse-steps' if args.fuse_steps else '--frame-steps'} and --samples "
                         f"{args.samples}: the x0 tiles of every posterior sample have a map of their own; give --samples 1 "
                         "or leave --seam-map out")


def _seam_kwargs(args):
    """What ``--seam-report`` adds to the driver's call: nothing without it."""
    if not args.seam_report:
        return {}
    return dict(disagreement=True if args.seam_map else "sums", seam_band=args.seam_band or 8)


def _write_seam_report(args, dis, val_set, plan, patch, samples, log):
    """``--seam-report``: the scores per channel over all frames, each once in normalised units and once in raw counts
    (scaled by std_target, as --std-out scales its spread; a variance by its square); zero counts give null.
    ``--seam-map``: s in raw counts."""
    if not args.seam_report:
        return
    import json
    count = dis["count"].sum(dim=0).cpu().numpy()                       # (C, 2): over all frames
    sum_var = dis["sum_var"].sum(dim=0).cpu().numpy()
    max_var = dis["max_var"].amax(dim=0).cpu().numpy()
    C_out = count.shape[0]
    _, std = _target_stats(val_set, C_out)
    frame_state = bool(args.fuse_steps or args.frame_steps)
    both = lambda v, scale: None if v is None else {"normalised": float(v), "raw": float(v * scale)}
    rms = lambda c, j: float(np.sqrt(2.0 * sum_var[c, j] / count[c, j])) if count[c, j] > 0 else None
    channels = []
    for c in range(C_out):
        largest = float(np.float32(np.sqrt(max_var[c]))) if count[c, 0] > 0 else None
        channels.append({"channel": c, "overlap_pixels": int(count[c, 0]), "band_pixels": int(count[c, 1]),
                         "rms_pair_overlap": both(rms(c, 0), std[c]), "rms_pair_band": both(rms(c, 1), std[c]),
                         "largest_s": both(largest, std[c])})
        log.info("channel %d: tiles disagree by %s RMS over the overlap, %s within %d pixels of a crop line (raw counts)",
                 c, *("%.4g" % (v * std[c]) if v is not None else "n/a" for v in (rms(c, 0), rms(c, 1))),
                 args.seam_band or 8)
    report = {"band": int(args.seam_band or 8),
              "stitch": "blend" if (args.stitch == "blend" or frame_state) else "crop",
              "tiles": int(plan.total), "patch": int(patch), "grid": int(plan.grid_shape[1]), "samples": int(samples),
              "frames": [int(v) for v in plan.data_shape],
              "measured": "x0 tiles of the last row" if frame_state else f"per-tile mean of {samples} samples",
              "rms_pair": "sqrt(2 * mean(var)): the RMS difference over all pairs of tiles that predicted a pixel",
              "channels": channels}
    with open(args.seam_report, "w") as f:
        json.dump(report, f, indent=1)
    log.info("seam report written to %s", args.seam_report)
    if args.seam_map:
        _write_prediction(args.seam_map, dis["map"], val_set, spread=True)
        log.info("disagreement map written to %s", args.seam_map)


def _check_msssim_args(args, config):
    """``--ms-ssim``, checked on the command line and the config file alone (nothing touches the GPU, no rank is
    started): it scores a tiled prediction of two grey channels against their ground truth.  Without it: nothing."""
    if not args.ms_ssim:
        return
    if args.input:
        raise SystemExit("--ms-ssim with --input: an input-only stack has no ground truth to score against")
    if args.validate:
        raise SystemExit("--ms-ssim scores the stitched frames of a tiled prediction: not with --validate")
    if args.datapath and _data_type(config()[1], args.norm_from) == "cifar10":
        raise SystemExit("--ms-ssim scores the stitched frames of a tiled prediction: the colour items of a cifar10 "
                         "config are not tiled (and 32 x 32 items cannot hold five scales)")
    if not (args.datapath or args.frames):
        try:
            _, h, w = (int(v) for v in args.synthetic.split(","))
        except ValueError:
            raise SystemExit(f"--synthetic {args.synthetic}: N,H,W")
        _msssim_size_or_exit(h, w)


def _msssim_size_or_exit(h, w):
    from .core.metrics import MSSSIM_WEIGHTS, check_msssim_size
    try:
        check_msssim_size(h, w, len(MSSSIM_WEIGHTS))
    except ValueError as e:
        raise SystemExit(f"--ms-ssim: {e}")


def _log_msssim(args, val_set, pred, ps, log):
    """``--ms-ssim`` on rank 0, after the stitched prediction has been scored with RangeInvariantPsnr: one line per
    channel, the mean and the standard error of the mean over the frames."""
    if not args.ms_ssim:
        return
    if ps is None:
        raise DsxError("--ms-ssim: the dataset holds no target with the prediction's channels to score against")
    from .core.metrics import calculate_msssim
    for c, vals in calculate_msssim(val_set.normalized_target_frames(), pred).items():
        v = np.asarray(vals, np.float64)
        sem = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else 0.0
        log.info("channel %d: MS-SSIM (range-invariant) %.6f +- %.6f over %d frames", c, float(v.mean()), sem, v.size)


def _check_calibration_args(args, config):
    """``--calibration`` / ``--apply-calibration``, checked on the command line, the config and the calibration file alone
    (nothing touches the GPU, no rank is started).  Without them: nothing."""
    if args.calibration_bins is not None and not args.calibration:
        raise SystemExit("--calibration-bins: only with --calibration FILE")
    if args.calibration:
        if args.input:
            raise SystemExit("--calibration with --input: an input-only stack has no ground truth to score the spread "
                             "against; fit the calibration on a stack with ground truth and use --apply-calibration here")
        if args.validate:
            raise SystemExit("--calibration scores the spread of a tiled prediction: not with --validate")
        if args.mix_t is not None:
            raise SystemExit("--calibration: not with --mix-t; the mixed-input prediction has no posterior spread")
        if (args.samples or 1) < 2:
            raise SystemExit("--calibration: the spread needs --samples 2 or more (--samples 1 has none)")
        if args.datapath and _data_type(config()[1], args.norm_from) == "cifar10":
            raise SystemExit("--calibration scores the stitched frames of a tiled prediction: the colour items of a "
                             "cifar10 config are not tiled")
        from .core.calibration import MAX_BINS
        if args.calibration_bins is not None and not 2 <= args.calibration_bins <= MAX_BINS:
            raise SystemExit(f"--calibration-bins {args.calibration_bins}: 2..{MAX_BINS} equal-count bins")
    if args.apply_calibration:
        if not args.std_out:
            raise SystemExit("--apply-calibration recalibrates the spread that --std-out writes: give --std-out FILE")
        from .core.calibration import Calibration
        try:
            cal = Calibration.load(args.apply_calibration)
        except (DsxError, OSError) as e:
            raise SystemExit(f"--apply-calibration {args.apply_calibration}: {e}")
        channels = 2 if config()[1].get("target_channel_idx") is None else 1
        if cal.channels != channels:
            raise SystemExit(f"--apply-calibration {args.apply_calibration}: a calibration of {cal.channels} channels, the "
                             f"prediction has {channels}")
        if cal.samples != (args.samples or 1):
            raise SystemExit(f"--apply-calibration {args.apply_calibration}: fitted at --samples {cal.samples}, this run "
                             f"draws {args.samples or 1}; the error of an N-sample mean depends on N")


def _log_calibration(args, val_set, pred, std, ps, samples, log):
    """``--calibration`` on rank 0: the gathered canvases against the normalised ground truth, one line per channel, the
    curve and its fit to the file."""
    if not args.calibration:
        return
    if ps is None:
        raise DsxError("--calibration: the dataset holds no target with the prediction's channels to score against")
    from .core.calibration import Calibration
    from .core.metrics import calculate_calibration
    stats = calculate_calibration(val_set.normalized_target_frames(), pred, std, bins=args.calibration_bins or 30)
    cal = Calibration.from_stats(stats, samples, _target_stats(val_set, pred.shape[-1])[1])
    for c in range(cal.channels):
        log.info("channel %d: calibration scale %.4f, rmse ~ %.4f rmv %+.4g; coverage at z = 1, 2, 3: %.4f %.4f %.4f "
                 "(%d bins, %d pixels)", c, cal.scale[c], cal.a[c], cal.c[c], *stats.coverage[c], stats.count.shape[1],
                 stats.n)
    cal.save(args.calibration)
    log.info("calibration over %d samples written to %s", samples, args.calibration)


def _parse_quantiles(text):
    """``--quantiles``: 1 to 8 comma-separated numbers in [0, 1] -> a tuple of floats (SystemExit otherwise)."""
    try:
        q = tuple(float(v) for v in str(text).split(","))
    except ValueError:
        q = ()
    if not 1 <= len(q) <= 8 or any(not 0.0 <= v <= 1.0 for v in q):
        raise SystemExit(f"--quantiles {text}: 1 to 8 comma-separated numbers in [0, 1], such as 0.05,0.5,0.95")
    return q


def _quantile_kwargs(args):
    """What ``--quantiles`` / ``--rank-histogram`` add to the driver's call: nothing without them."""
    kw = {}
    if args.quantiles:
        kw["quantiles"] = _parse_quantiles(args.quantiles)
    if args.rank_histogram:
        kw["ranks"] = True
    return kw


def _check_quantile_args(args, config):
    """``--quantiles`` / ``--quantile-out`` / ``--rank-histogram``, checked on the command line and the config alone
    (nothing touches the GPU, no rank is started).  Without them: nothing."""
    if bool(args.quantiles) != bool(args.quantile_out):
        if args.quantiles:
            raise SystemExit("--quantiles: give --quantile-out FILE (.npy / .tif) for the maps")
        raise SystemExit("--quantile-out: give --quantiles Q1,Q2,.. to say which maps to write")
    for flag, value, exts in (("--quantile-out", args.quantile_out, (".npy", ".tif", ".tiff")),
                              ("--rank-histogram", args.rank_histogram, (".json",))):
        if not value:
            continue
        if not value.endswith(exts):
            raise SystemExit(f"{flag} {value}: a {' or '.join(exts[:2])} file")
        if args.validate:
            raise SystemExit(f"{flag} is taken over the posterior samples of a tiled prediction: not with --validate")
        if args.mix_t is not None:
            raise SystemExit(f"{flag}: not with --mix-t; the mixed-input prediction has no posterior samples")
        if (args.samples or 1) < 2:
            raise SystemExit(f"{flag}: quantiles and ranks are taken over --samples 2 or more (--samples 1 has none)")
        if args.samples > 64:
            raise SystemExit(f"{flag}: the samples of a pixel are sorted in registers: --samples {args.samples}, at most 64")
        if args.datapath and _data_type(config()[1], args.norm_from) == "cifar10":
            raise SystemExit(f"{flag} is taken over the stitched frames of a tiled prediction: the colour items of a "
                             "cifar10 config are not tiled")
    if args.quantiles:
        _parse_quantiles(args.quantiles)
    if args.rank_histogram:
        if args.input:
            raise SystemExit("--rank-histogram with --input: an input-only stack has no ground truth to rank among the "
                             "samples")
        if args.stitch == "blend" and not (args.fuse_steps or args.frame_steps):
            raise SystemExit("--rank-histogram with --stitch blend: a blend of per-tile ranks is not a rank; use --stitch "
                             "crop, or a frame-state path (--fuse-steps, --frame-steps) where ranks are exact per pixel")


def _write_quantiles(path, quant, q, val_set):
    """--quantile-out: the quantile maps (Q,N,H,W,C), un-normalised to raw counts like --out (q * std_target +
    mean_target), as .npy (Q,N,H,W,C) float32 or as a .tif of Q * N * C float32 pages, quantile-major (page
    (k * N + n) * C + c), the description naming the quantiles and the order."""
    Q, N, H, W, C_out = quant.shape
    mean, std = _target_stats(val_set, C_out)
    raw = (quant * torch.as_tensor(std, dtype=torch.float32, device=quant.device)
           + torch.as_tensor(mean, dtype=torch.float32, device=quant.device)).cpu().numpy()
    if str(path).endswith(".npy"):
        np.save(path, raw)
        return
    from .data.tiff import imwrite
    desc = (f"ImageJ=1.11a\nimages={Q * N * C_out}\nchannels={C_out}\nslices={N}\nframes={Q}\nhyperstack=true\n"
            f"mode=grayscale\norder=quantile,frame,channel\nquantiles={','.join(repr(v) for v in q)}\n")
    imwrite(path, np.ascontiguousarray(raw.transpose(0, 1, 4, 2, 3)).reshape(Q * N * C_out, H, W), description=desc)


def _log_rank_histogram(args, rank, samples, log):
    """``--rank-histogram`` on rank 0: the counts of the rank canvas per channel, the coverage of the widest central band
    and of the one nearest 50 % against their nominal values, histogram and bands to the file."""
    if not args.rank_histogram:
        return
    from .core.calibration import interval_coverage, rank_histogram, save_rank_histogram
    hist = rank_histogram(rank, samples)
    cov = interval_coverage(hist)
    half = int(np.argmin(np.abs(cov.nominal - 0.5)))
    for c in range(hist.shape[0]):
        log.info("channel %d: ground truth between the extreme samples in %.4f of the pixels (nominal %.4f); between the "
                 "%d-th smallest and largest in %.4f (nominal %.4f); %d samples, %d pixels", c, cov.observed[c, 0],
                 cov.nominal[0], int(cov.m[half]), cov.observed[c, half], cov.nominal[half], samples, cov.pixels)
    save_rank_histogram(args.rank_histogram, hist)
    log.info("rank histogram over %d samples written to %s", samples, args.rank_histogram)


def _check_input_args(args, config):
    """The flags of the input-only prediction and of the posterior samples, checked on the command line, the config and
    the normalisation file alone (nothing touches the GPU, no rank is started)."""
    if args.samples is not None:
        if args.samples < 1:
            raise SystemExit(f"--samples {args.samples}: a positive count of posterior samples")
        if args.mix_t is not None:
            raise SystemExit("--samples: not with --mix-t; the repeats of the mixed-input prediction are --mmse N")
        if args.validate:
            raise SystemExit("--samples repeats the tiles of a tiled prediction: not with --validate")
    if args.std_out:
        if not args.std_out.endswith((".npy", ".tif", ".tiff")):
            raise SystemExit("--std-out: a .npy or .tif file")
        if args.validate or args.mix_t is not None:
            raise SystemExit("--std-out writes the spread of a tiled prediction: not with --validate or --mix-t")
        if (args.samples or 1) < 2:
            raise SystemExit("--std-out: the spread needs --samples 2 or more (--samples 1 has none)")
    if args.save_norm and not (args.datapath or args.frames):
        raise SystemExit("--save-norm writes the normalisation of real channels: only with --datapath or --frames")
    if not args.input:
        for flag, value in (("--norm", args.norm), ("--input-clip", args.input_clip)):
            if value is not None:
                raise SystemExit(f"{flag}: only with --input FILE")
        return
    for flag, value in (("--datapath", args.datapath), ("--frames", args.frames), ("--validate", args.validate),
                        ("--mix-t", args.mix_t is not None)):
        if value:
            raise SystemExit(f"--input with {flag}: an input-only stack has no ground-truth channels; it is a tiled "
                             "prediction of its own")
    if not args.norm:
        raise SystemExit("--input needs --norm FILE: the normalisation of the training set, written by --save-norm (an "
                         "input-only stack has no channels to compute it from)")
    if args.input_clip is not None and not (np.isfinite(args.input_clip) and args.input_clip >= 0):
        raise SystemExit(f"--input-clip {args.input_clip}: a finite, non-negative count")
    which, ds = config()
    if which == "joint_indi":
        raise SystemExit("--input with a joint_indi config: its network input is the weighted sum of the NORMALISED "
                         "channels, which is no function of the superimposed counts unless both stds are equal")
    from .data.normalization import load_normalization
    try:
        _, meta = load_normalization(args.norm)
    except (DsxError, OSError) as e:
        raise SystemExit(f"--norm {args.norm}: {e}")
    if meta["data_type"] == "cifar10":
        raise SystemExit(f"--norm {args.norm}: a cifar10 normalisation; --input takes a grey (N,H,W) stack, colour items "
                         "are not tiled")
    idx = ds.get("target_channel_idx")
    if meta["target_channel_idx"] != idx:
        raise SystemExit(f"--norm {args.norm}: written for target_channel_idx = {meta['target_channel_idx']}, the config "
                         f"says {idx}")


def _check_solver_args(args, config):
    """The flags of few-step sampling and of frame-keyed noise, checked on the command line and the config file alone
    (nothing touches the GPU, no rank is started).  Without any of them: nothing."""
    if args.noise_field:
        if args.sample_seed is None:
            raise SystemExit("--noise-field needs --sample-seed S: a noise field is named by (seed, frame, draw)")
        if args.validate or args.mix_t is not None:
            raise SystemExit("--noise-field cuts the noise of a tiled prediction's tiles: not with --validate or --mix-t")
    given = [flag for flag, value in (("--solver-steps", args.solver_steps), ("--eta", args.eta),
                                      ("--spacing", args.spacing)) if value is not None]
    if args.solver is None:
        if given:
            raise SystemExit(f"{', '.join(given)}: only with --solver {{ddim,dpmpp2m}}")
        return
    which = config()[0]
    if which not in ("sr3", "ddpm"):
        raise SystemExit(f"--solver: few-step solvers run a Gaussian sampler (which_model_G sr3 / ddpm); this config "
                         f"builds {which!r}, whose loop already takes --steps")
    if args.solver_steps is None:
        raise SystemExit("--solver needs --solver-steps K: how many timesteps of the trained schedule to run")
    if args.solver_steps < 1:
        raise SystemExit(f"--solver-steps {args.solver_steps}: a positive count")
    if args.validate or args.mix_t is not None:
        raise SystemExit("--solver samples the tiles of a tiled prediction: not with --validate or --mix-t")
    from .model import solvers
    try:
        solvers.check_solver(args.solver, args.eta or 0.0)
    except DsxError as e:
        raise SystemExit(f"--solver {args.solver} --eta {args.eta}: {e}")


def _check_stitch_args(args, n_ranks):
    """The flags of blended stitching and of per-step frame fusion, checked on the command line alone (nothing touches
    the GPU, no rank is started).  Without any of them: nothing."""
    blend = args.stitch == "blend" or args.fuse_steps or args.frame_steps
    if args.window is not None and not blend:
        raise SystemExit("--window: only with --stitch blend (the window weighs the overlap-add of whole tiles)")
    if args.stitch == "blend" and (args.validate or args.mix_t is not None):
        raise SystemExit("--stitch blend stitches the tiles of a tiled prediction: not with --validate or --mix-t")
    if not args.fuse_steps:
        return
    if args.validate or args.mix_t is not None:
        raise SystemExit("--fuse-steps fuses the tiles of a tiled prediction: not with --validate or --mix-t")
    if args.stitch == "crop":
        raise SystemExit("--fuse-steps with --stitch crop: a fused frame is a blend of its tiles; leave --stitch out or give "
                         "--stitch blend")
    if args.solver is None:
        raise SystemExit("--fuse-steps needs --solver {ddim,dpmpp2m}: the rows of a few-step solver are fused; the "
                         "ancestral loop is not")
    if args.sample_seed is None or not args.noise_field:
        raise SystemExit("--fuse-steps needs --sample-seed S and --noise-field: overlapping tiles must receive the same "
                         "noise, or the blend would shrink its variance")
    if n_ranks > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--fuse-steps runs on one rank: a collective after every solver row is not provided")


def _check_frame_args(args, config):
    """``--frame-steps``, checked on the command line and the config file alone (nothing touches the GPU, no rank is
    started).  Without it: nothing."""
    if not args.frame_steps:
        return
    if args.fuse_steps:
        raise SystemExit("--frame-steps together with --fuse-steps: --fuse-steps fuses the rows of a Gaussian solver, "
                         "--frame-steps diffuses the frames of an InDI config; give one")
    if args.solver is not None:
        raise SystemExit("--frame-steps with --solver: frame diffusion runs the InDI loop of an indi / joint_indi config; "
                         "few-step solvers belong to sr3 / ddpm (--fuse-steps)")
    which = config()[0]
    if which not in ("indi", "joint_indi"):
        raise SystemExit(f"--frame-steps diffuses the frames of an InDI sampler (which_model_G indi / joint_indi); this "
                         f"config builds {which!r}: a Gaussian sampler's fusion is --solver with --fuse-steps")
    if args.validate or args.mix_t is not None or args.mmse is not None:
        raise SystemExit("--frame-steps diffuses the frames of a tiled prediction: not with --validate, --mix-t or --mmse")
    if args.stitch == "crop":
        raise SystemExit("--frame-steps with --stitch crop: a frame state is a blend of its tiles; leave --stitch out or "
                         "give --stitch blend")
    if args.sample_seed is None:
        raise SystemExit("--frame-steps needs --sample-seed S: a frame's noise field is named by (seed, frame, draw)")


def _solver_of(args):
    """The dict ``predict_stack(solver=...)`` takes (what ``DDPM.set_solver`` keeps), or None without --solver."""
    if args.solver is None:
        return None
    return dict(solver=args.solver, steps=int(args.solver_steps), eta=float(args.eta or 0.0), spacing=args.spacing)


_MIXED_FLAGS = (("--mix-t", "mix_t"), ("--time-predictor", "time_predictor"),
                ("--time-predictor-checkpoint", "time_predictor_checkpoint"), ("--mmse", "mmse"), ("--t-from", "t_from"),
                ("--refine-rounds", "refine_rounds"), ("--refine-scope", "refine_scope"), ("--refine-step", "refine_step"))
_REFINE_FLAGS = _MIXED_FLAGS[-3:]


def _check_mixed_args(args, config):
    """The flags of the mixed-input prediction, checked on the command line and the config file alone (nothing touches
    the GPU, no rank is started): they need a ``joint_indi`` config and ``--mix-t``.  Without any of them: nothing."""
    given = [flag for flag, name in _MIXED_FLAGS if getattr(args, name) is not None]
    if not given:
        return
    which = config()[0]
    if which != "joint_indi":
        raise SystemExit(f"{', '.join(given)}: the mixed-input prediction runs indi1 and indi2 of a joint_indi config; "
                         f"this config builds {which!r}")
    if args.mix_t is None:
        raise SystemExit(f"{', '.join(given)}: only with --mix-t T (the mixing weight of the mixed-input prediction)")
    if not (np.isfinite(args.mix_t) and 0.0 <= args.mix_t <= 1.0):
        raise SystemExit(f"--mix-t {args.mix_t}: a mixing weight in [0, 1]")
    if args.validate:
        raise SystemExit("--mix-t is a tiled prediction: not with --validate")
    if args.mmse is not None and args.mmse < 1:
        raise SystemExit(f"--mmse {args.mmse}: a positive count of repeats")
    if (args.t_from or "classifier") == "classifier" and not args.time_predictor:
        raise SystemExit("--t-from classifier (the default) needs --time-predictor CONFIG; --t-from given starts both "
                         "samplers at --mix-t")
    if args.time_predictor_checkpoint and not args.time_predictor:
        raise SystemExit("--time-predictor-checkpoint: only with --time-predictor CONFIG")
    refine = [flag for flag, name in _REFINE_FLAGS if getattr(args, name) is not None]
    if refine and args.t_from != "refined":
        raise SystemExit(f"{', '.join(refine)}: only with --t-from refined (the start times re-estimated from the split)")
    if args.refine_rounds is not None and args.refine_rounds < 0:
        raise SystemExit(f"--refine-rounds {args.refine_rounds}: a count of rounds, 0 or more")
    if args.refine_step is not None and not (np.isfinite(args.refine_step) and 0.0 < args.refine_step < 1.0):
        raise SystemExit(f"--refine-step {args.refine_step}: a spacing in (0, 1)")


def _predict_mixed(args, netG, val_set, n_steps, patch, rank, world, log):
    """``--mix-t``: ``predict_tiled_mixed`` of ``val_set`` over the ranks (the TimePredictor of ``--time-predictor``
    chooses every tile's start time unless ``--t-from given``); ``pred_t`` is gathered so that rank 0 holds every
    tile's value; rank 0 logs and writes ``--out``.  ``--t-from refined``: ``predict_tiled_refined`` instead (its table
    is complete on every rank), and a log line per refinement round.  Returns the stitched canvas."""
    from .data.tiled_predict import gather_pred_t, predict_tiled_mixed, predict_tiled_refined
    t_from = args.t_from or "classifier"
    tp = None
    if args.ms_ssim:
        _msssim_size_or_exit(*val_set._data_shape[-2:])              # before any tile is predicted
    if t_from == "classifier" or (t_from == "refined" and args.time_predictor):
        from . import time_prediction
        tp_opt = Logger.dict_to_nonedict(Logger.load_json(args.time_predictor))
        if args.dtype:
            tp_opt["model"]["compute_dtype"] = args.dtype
        tp = time_prediction.build_time_predictor(tp_opt, args.time_predictor_checkpoint)
        if args.time_predictor_checkpoint is None and rank == 0:
            log.info("no --time-predictor-checkpoint given: the TimePredictor keeps its random initial weights")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    report = None
    if t_from == "refined":
        (pred, ps), pred_t, report = predict_tiled_refined(
            netG, tp, val_set, args.mix_t, num_timesteps=n_steps, mmse_count=args.mmse or 1,
            batch_tiles=args.batch_tiles, rounds=1 if args.refine_rounds is None else args.refine_rounds,
            scope=args.refine_scope or "frame", t_list=np.arange(0, 1.0, args.refine_step or 0.05),
            seed=args.sample_seed)
    else:
        (pred, ps), pred_t = predict_tiled_mixed(netG, tp, val_set, args.mix_t, num_timesteps=n_steps,
                                                 mmse_count=args.mmse or 1, batch_tiles=args.batch_tiles, t_from=t_from,
                                                 seed=args.sample_seed)
        pred_t = gather_pred_t(pred_t)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rank == 0:
        total = val_set.plan.total
        for q, rnd in enumerate(report["rounds"] if report else []):
            chosen = rnd["chosen"][~np.isnan(rnd["chosen"])]
            if chosen.size == 0:
                log.info("refinement round %d: every curve is NaN, the start times stay", q)
                continue
            log.info("refinement round %d (scope %s, %d of %d units): chosen time min %.4f mean %.4f max %.4f; peak of the "
                     "mean curve %.2f dB; |chosen - mix_t| mean %.4f max %.4f", q, args.refine_scope or "frame",
                     chosen.size, rnd["chosen"].size, chosen.min(), chosen.mean(), chosen.max(),
                     float(np.nanmax(np.nanmean(rnd["mean_curves"][~np.isnan(rnd["chosen"])], axis=0))),
                     np.abs(chosen - args.mix_t).mean(), np.abs(chosen - args.mix_t).max())
        log.info("mixed-input prediction at t = %g (%s start times): %d tiles of %d^2, %d steps, mmse %d, %d GPU(s): "
                 "%.3f s (%.1f tiles/s)", args.mix_t, t_from, total, patch, n_steps, args.mmse or 1, world, dt, total / dt)
        for c in range(ps.shape[1]):
            log.info("channel %d: RangeInvariantPsnr %.2f +- %.2f dB; predicted start time min %.4f mean %.4f max %.4f",
                     c, ps[:, c].mean().item(), ps[:, c].std().item() if ps.shape[0] > 1 else 0.0,
                     pred_t[:, c].min().item(), pred_t[:, c].mean().item(), pred_t[:, c].max().item())
        _log_msssim(args, val_set, pred, ps, log)
        if args.out:
            _write_prediction(args.out, pred, val_set)
            log.info("prediction written to %s", args.out)
    return pred


def _run_validate(args, opt, diffusion, items, log, whole_set=False):
    """``core.validation.validate`` over the first ``--items`` items (default 19; every item with ``whole_set``), the
    log lines of the training loop, and with ``--out`` the predictions in raw counts.  Returns avg_psnr."""
    from .core.validation import validate
    if args.steps:
        diffusion.netG.set_new_noise_schedule(dict(opt["model"]["beta_schedule"]["val"], n_timestep=args.steps),
                                              diffusion.device)
    n_items = args.items if args.items is not None else (None if whole_set else 19)
    preds = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    avg_psnr, per_channel = validate(diffusion, items, n_items=n_items, batch=args.batch_tiles, result_path=args.results,
                                     on_batch=(lambda i0, pred: preds.append(_raw_counts(pred, items))) if args.out else None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    log.info("# Validation # PSNR: {:.4e}".format(avg_psnr))
    for ch, vals in per_channel.items():
        log.info("channel %d: PSNR %.4e over %d items", ch, float(np.mean(vals)), len(vals))
    if whole_set:
        n = len(next(iter(per_channel.values())))
        log.info("validation: %d items in batches of %d: %.3f s (%.1f items/s)", n, args.batch_tiles, dt, n / dt)
    if args.out:
        np.save(args.out, torch.cat(preds).cpu().numpy())
        log.info("predictions written to %s", args.out)
    return avg_psnr


def _raw_counts(pred, val_set):
    """A normalised prediction (B, C, H, W) in raw counts: x * std_target + mean_target per channel in float64, as the
    validation report un-normalises it, rounded to float32 once."""
    mean, std = _target_stats(val_set, pred.shape[1])
    as_t = lambda v: torch.as_tensor(v, dtype=torch.float64, device=pred.device).reshape(1, -1, 1, 1)
    return (pred.to(torch.float64) * as_t(std) + as_t(mean)).to(torch.float32)


if __name__ == "__main__":
    main()
