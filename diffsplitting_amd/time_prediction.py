#!/usr/bin/env python3
"""``time_prediction_training.py`` of the reference, the parts that do not train: the datasets of a TimePredictor
config (:20-63), the network (:79-89), and the validation loop whose mean selects the checkpoint (:133-152).

    python -m diffsplitting_amd.time_prediction -c config/splitting_hagen_time_predictor.json --datapath \\
        --checkpoint best_time_predictor.pth [--norm-from val] [--seed S] [--batch-size B] [--sweep N] [--dtype f32]

logs ``val_loss`` of the checkpoint on the config's validation stack and, with ``--sweep N``, the RMSE and the mean
prediction per mixing ratio of the classifier sweep (``evaluate_time_predictor``) on the tiled form of the same stack.
Every batch of the loop is one fused gather launch (``TimePredictorDataset.batch``) and one batched forward.
Training is refused: the engine is inference-only.
"""
import argparse
import logging
import time

import numpy as np
import torch

from .core import logger as Logger
from ._lib import DsxError
from .data.split_dataset import DataLocation, SplitDataset, SplitDatasetTiledPred
from .data.tiled_predict import _batches, evaluate_time_predictor, store_kept
from .data.time_predictor_dataset import TimePredictorDataset
from .model.ddpm_modules.time_predictor import TimePredictor

LOSS_TYPES = ("l1", "l2")


def _check_loss_type(loss_type):
    if loss_type not in LOSS_TYPES:
        raise DsxError(f"loss_type = {loss_type!r}: 'l1' (torch.nn.L1Loss) or 'l2' (torch.nn.MSELoss)")


def _locations(opt):
    ds = opt["datasets"]
    return {part: DataLocation(channelwise_fpath=(ds[part]["datapath"]["ch0"], ds[part]["datapath"]["ch1"]))
            for part in ("train", "val") if ds[part]}


def _common(opt, device):
    ds = opt["datasets"]
    return dict(target_channel_idx=ds.get("target_channel_idx", None), max_qval=ds["max_qval"],
                upper_clip=bool(ds.get("upper_clip", None)), channel_weights=ds.get("channel_weights", None),
                enable_transforms=False, random_patching=False, device=device)


def get_datasets(opt, tiled_pred=False, norm_from="train", device="cuda"):
    """time_prediction_training.py:20-63 -> (train_set, val_set) with the conventions of ``split.get_datasets``: the
    training set is built without transforms, random patching or Gaussian noise (``gaussian_noise_std_factor`` is not
    passed on) -- this engine does not train, the set is there for its statistics only, so it is a plain
    ``SplitDataset`` and no range table is computed for it.  The validation set is a ``TimePredictorDataset``
    normalised with the training set's dict.  ``norm_from="val"`` takes the statistics from the validation stack
    itself (``train_set`` is then None)."""
    if tiled_pred:
        raise NotImplementedError("Tiled prediction not implemented yet")          # :54
    if norm_from not in ("train", "val"):
        raise DsxError(f"norm_from = {norm_from!r}: 'train' or 'val'")
    ds = opt["datasets"]
    data_type = (ds["train"] if norm_from == "train" else ds["train"] or ds["val"])["name"]
    if data_type != "Hagen":
        raise DsxError(f"data_type {data_type!r}: the TimePredictor's mixed inputs take two grey channels ('Hagen')")
    loc, common = _locations(opt), _common(opt, device)
    train_set, nd = None, None
    if norm_from == "train":
        train_set = SplitDataset(data_type, loc["train"], ds["patch_size"], normalization_dict=None,
                                 uncorrelated_channels=bool(ds["train"].get("uncorrelated_channels")), **common)
        nd = train_set.get_normalization_dict()
    val_set = TimePredictorDataset(data_type, loc["val"], ds["patch_size"], normalization_dict=nd, **common)
    return train_set, val_set


def tiled_val_set(opt, val_set, device="cuda"):
    """The ``SplitDatasetTiledPred`` (grid = patch // 2) of the validation stack ``val_set`` was read from, with
    ``val_set``'s normalisation: what the classifier sweep runs on."""
    ds = opt["datasets"]
    return SplitDatasetTiledPred("Hagen", _locations(opt)["val"], ds["patch_size"], grid_size=ds["patch_size"] // 2,
                                 normalization_dict=val_set.get_normalization_dict(), **_common(opt, device))


def build_time_predictor(opt, checkpoint=None):
    """:79-89: ``TimePredictor`` from ``model.unet`` with ``image_size = datasets.patch_size``, on the device;
    ``checkpoint``: a plain ``state_dict`` file (what :151 saves), loaded with ``strict=True``.  ``model.compute_dtype``
    selects the MFMA operand type as in ``define_G``."""
    u = opt["model"]["unet"]
    model = TimePredictor(in_channel=u["in_channel"], out_channel=u["out_channel"], norm_groups=u["norm_groups"],
                          inner_channel=u["inner_channel"], channel_mults=u["channel_multiplier"],
                          attn_res=u["attn_res"], res_blocks=u["res_blocks"], dropout=u["dropout"],
                          image_size=opt["datasets"]["patch_size"])
    dtype = opt["model"].get("compute_dtype") or "f32"
    for m in model.modules():
        if hasattr(m, "compute_dtype"):
            m.compute_dtype = dtype
    model = model.cuda()
    if checkpoint is not None:
        model.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True), strict=True)
    return model.eval()


def batch_losses(pred, t, batch_size, loss_type):
    """The arithmetic of :135-140 and :144 from the predictions: items in index order in batches of ``batch_size``,
    per batch the mean of ``|pred - y|`` ('l1') or ``(pred - y)**2`` ('l2') with ``y = float32(t)`` (``y.type(
    torch.float32)``), ``val_loss`` the mean over the batches -- a short last batch weighs as much as a full one.
    ``pred`` is taken as float32; the means are float64 (the reference sums in float32 on the GPU: a few ulps).
    -> (val_loss, per_batch_losses (n_batches,) float64)."""
    _check_loss_type(loss_type)
    pred = np.asarray(pred, dtype=np.float32).reshape(-1)
    y = np.asarray(t, dtype=np.float64).reshape(-1).astype(np.float32)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise DsxError(f"batch_size = {batch_size}: a positive count")
    if pred.size != y.size or pred.size == 0:
        raise DsxError(f"{pred.size} predictions for {y.size} values of t (at least one item)")
    d = pred.astype(np.float64) - y.astype(np.float64)
    d = np.abs(d) if loss_type == "l1" else d * d
    per_batch = np.array([d[i:i + batch_size].mean() for i in range(0, d.size, batch_size)], dtype=np.float64)
    return float(per_batch.mean()), per_batch


@torch.no_grad()
def validation_loss(model, val_set, batch_size, loss_type):
    """:133-140 on the device: every item of ``val_set`` (a ``TimePredictorDataset``) in index order, its t drawn
    exactly once by ``val_set.sample_t()`` in that order (``np.random``: seed it for a repeatable value); one gather
    launch and one batched forward per batch.  A short last batch is moved back to overlap the batch before it
    (``_batches``: one executor) with the overlapped items keeping the t they drew; only its own entries are kept.
    The predictions come back once, at the end; ``batch_losses`` takes the means.
    -> (val_loss, per_batch_losses, pred (N,) float32 numpy, t (N,) float64 numpy)."""
    _check_loss_type(loss_type)
    if getattr(val_set, "_random_patching", False):
        raise DsxError("validation_loss: random_patching draws the locations too; the validation set has fixed patches")
    n, batch_size = len(val_set), int(batch_size)
    if n < 1 or batch_size < 1:
        raise DsxError(f"validation_loss: {n} items in batches of {batch_size}: both must be positive")
    pred = torch.empty(n, dtype=torch.float32, device=val_set._dev[0].device)
    t_ints, t_all = [0] * n, np.empty(n, dtype=np.float64)
    for chunk, keep in _batches(range(n), batch_size):
        for i in chunk[len(chunk) - keep:]:
            t_ints[i] = val_set.sample_t()[1]
        inp, t = val_set.batch(chunk, t_ints=[t_ints[i] for i in chunk])
        store_kept(pred, model(inp), chunk, keep)
        store_kept(t_all, t, chunk, keep)
    pred = pred.cpu().numpy()
    val_loss, per_batch = batch_losses(pred, t_all, batch_size, loss_type)
    return val_loss, per_batch, pred, t_all


def main(argv=None):
    ap = argparse.ArgumentParser(description="val_loss and classifier sweep of a TimePredictor checkpoint")
    ap.add_argument("-c", "--config", type=str, required=True, help="the TimePredictor's JSON configuration")
    ap.add_argument("-p", "--phase", type=str, choices=["train", "val"], default="val")
    ap.add_argument("-gpu", "--gpu_ids", type=str, default="0")
    ap.add_argument("--datapath", action="store_true",
                    help="read the frames from the config's datasets.{train,val}.datapath stacks (required)")
    ap.add_argument("--checkpoint", type=str, default=None, help="state_dict file (best_time_predictor.pth)")
    ap.add_argument("--norm-from", type=str, choices=["train", "val"], default="train",
                    help="the stack whose statistics normalise the validation set")
    ap.add_argument("--seed", type=int, default=None, help="seeds np.random before the draws of t")
    ap.add_argument("--batch-size", type=int, default=None, help="default: datasets.train.batch_size")
    ap.add_argument("--sweep", type=int, default=None, help="also the classifier sweep over N + 1 mixing ratios")
    ap.add_argument("--dtype", type=str, default=None, choices=["f32", "bf16", "f16"])
    args = ap.parse_args(argv)
    if args.phase == "train":
        raise SystemExit("training is out of scope of the MI355X engine: there is no -p train")
    if not args.datapath:
        raise SystemExit("--datapath: the frames come from the config's datasets.{train,val}.datapath stacks")
    if args.sweep is not None and not 1 <= args.sweep <= 1024:
        raise SystemExit(f"--sweep {args.sweep}: the number of mixing steps, 1..1024")
    if args.batch_size is not None and args.batch_size < 1:
        raise SystemExit(f"--batch-size {args.batch_size}: a positive count")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    log = logging.getLogger("base")
    opt = Logger.parse(args)
    if args.dtype:
        opt["model"]["compute_dtype"] = args.dtype
    loss_type = opt["model"]["loss_type"]
    _check_loss_type(loss_type)
    batch_size = args.batch_size or int(opt["datasets"]["train"]["batch_size"])
    ids = list(opt["gpu_ids"] or [0])
    torch.cuda.set_device(ids[0])
    dev = torch.device("cuda", torch.cuda.current_device())

    model = build_time_predictor(opt, args.checkpoint)
    if args.checkpoint is None:
        log.info("no --checkpoint given: the TimePredictor keeps its random initial weights")
    _, val_set = get_datasets(opt, norm_from=args.norm_from, device=dev)
    if args.seed is not None:
        np.random.seed(args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    val_loss, per_batch, pred, t = validation_loss(model, val_set, batch_size, loss_type)
    dt = time.perf_counter() - t0
    log.info("val_loss: {:.4e}".format(val_loss))
    log.info("validation: %d items in %d batches of %d, loss %s: %.3f s (%.1f items/s)", len(pred), len(per_batch),
             batch_size, loss_type, dt, len(pred) / dt)
    result = {"val_loss": val_loss, "per_batch": per_batch, "pred": pred, "t": t}
    if args.sweep is not None:
        tiled = tiled_val_set(opt, val_set, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        all_pred, rmse = evaluate_time_predictor(tiled, model, num_timesteps=args.sweep, batch_tiles=batch_size)
        dt = time.perf_counter() - t0
        log.info("sweep RMSE: {:.4e}".format(rmse))
        for k, row in enumerate(all_pred):
            log.info("ratio %.4f: mean prediction %.4f", k / args.sweep, float(row.mean()))
        log.info("sweep: %d ratios x %d tiles: %.3f s (%.1f items/s)", all_pred.shape[0], all_pred.shape[1], dt,
                 all_pred.size / dt)
        result.update(rmse=rmse, all_pred=all_pred)
    return result


if __name__ == "__main__":
    main()
