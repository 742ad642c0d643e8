"""Does the predicted spread mean anything?  The calibration of a per-pixel standard deviation against the real error.

``predict_stack(..., samples=N, return_std=True)`` returns a mean and a spread per pixel.  With ground truth at hand the
pixels of every channel are binned by their predicted std (equal-count bins: the edges are exact quantiles,
``bin_edges``), and per bin the root mean variance ``rmv = sqrt(mean std^2)`` stands beside the root mean squared error
``rmse = sqrt(mean (target - mean)^2)``: a calibrated spread has ``rmse == rmv`` in every bin.  ``calibration_stats``
computes the bins and the interval coverage (the share of pixels with ``|error| <= z std``) in ONE HIP pass over the
three canvases (``dsx_calibration``: exact counts, bounded sums, equal bits run to run); ``fit`` draws the weighted line
``rmse ~ a rmv + c`` through the curve; ``Calibration`` keeps curve and fit as a JSON file and applies the line to a
spread predicted where no ground truth exists (``split --calibration FILE`` / ``--apply-calibration FILE``).

Everything after the kernel runs in float64 on the host: a curve is a few hundred numbers."""
import json
import math
import types

import numpy as np
import torch

from .._lib import DsxError

FORMAT = "diffsplitting_amd.calibration"
VERSION = 1
MAX_BINS, MAX_Z, MAX_C = 64, 8, 4


def _canvas(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() < 1:
        got = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise DsxError(f"calibration: {name} must be a CUDA float32 tensor (..., C), got {got}")
    if not 1 <= t.shape[-1] <= MAX_C:
        raise DsxError(f"calibration: {name} has {t.shape[-1]} channels (the last dimension), must be in 1..{MAX_C}")
    if t.numel() == 0:
        raise DsxError(f"calibration: {name} of shape {tuple(t.shape)} holds no pixel")
    return t.contiguous()


def quantile_ranks(n, bins):
    """What ``np.quantile(x, j / bins)`` (x of n values, j = 1 .. bins - 1) needs of sorted x: (ranks, lo, hi, frac) with
    the two neighbouring order statistics of edge j at ranks[lo[j]] and ranks[hi[j]] and the interpolation weight."""
    pos = (n - 1) * (np.arange(1, bins, dtype=np.float64) / bins)
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    ranks, inverse = np.unique(np.concatenate([lo, hi]), return_inverse=True)
    return ranks, inverse[:bins - 1], inverse[bins - 1:], pos - lo


def edges_from_order_stats(stats, lo, hi, frac):
    """The edges from the order statistics of ``quantile_ranks``: the interpolation expression of ``quantile_select``."""
    return np.array([np.quantile(np.array([stats[l], stats[h]]), f) for l, h, f in zip(lo, hi, frac)], dtype=np.float64)


def bin_edges(std, bins):
    """The ``bins - 1`` inner edges of equal-count bins per channel of a (..., C) CUDA fp32 spread -> (C, bins - 1)
    float64, bit-equal to ``np.quantile(std[..., c].astype(np.float64), j / bins)``: one radix select per channel
    (``order_stats_device``) for all the ranks it needs, no sort."""
    from ..data.split_dataset import order_stats_device
    std = _canvas(std, "std")
    bins = _check_bins(bins)
    C = std.shape[-1]
    flat = std.reshape(-1, C)
    ranks, lo, hi, frac = quantile_ranks(flat.shape[0], bins)
    out = np.empty((C, bins - 1), dtype=np.float64)
    for c in range(C):
        if bins > 1:
            out[c] = edges_from_order_stats(order_stats_device(flat[:, c].contiguous(), None, 1.0, 0.0, ranks), lo, hi, frac)
    return out


def _check_bins(bins):
    if int(bins) != bins or not 1 <= bins <= MAX_BINS:
        raise DsxError(f"calibration: bins = {bins!r}, must be an integer in 1..{MAX_BINS}")
    return int(bins)


def calibration_sums(mean, std, target, edges, z):
    """``dsx_calibration`` on three (..., C) CUDA fp32 canvases of one shape -> (C, 3 * nbins + nz) float64 on the device:
    per channel {count, Sv, Se} of every bin, then the coverage counts.  Two launches, nothing synchronised."""
    from .. import _lib
    mean, std, target = _canvas(mean, "mean"), _canvas(std, "std"), _canvas(target, "target")
    if not (mean.shape == std.shape == target.shape):
        raise DsxError(f"calibration: mean, std and target must be of one shape, got {tuple(mean.shape)}, "
                       f"{tuple(std.shape)} and {tuple(target.shape)}")
    _lib.common_device("calibration", [t.device for t in (mean, std, target)])
    C = mean.shape[-1]
    n = mean.numel() // C
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    if edges.ndim != 2 or edges.shape[0] != C:
        raise DsxError(f"calibration: edges of shape {edges.shape}, expected ({C}, bins - 1)")
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    nbins, nz = edges.shape[1] + 1, z.size
    _lib.require_gpu()
    blocks = _lib.check(_lib.lib.dsx_calibration_blocks(n))
    row = C * (3 * nbins + nz)
    part = torch.empty((blocks, row), dtype=torch.float64, device=mean.device)
    out = torch.empty((C, 3 * nbins + nz), dtype=torch.float64, device=mean.device)
    _lib.check(_lib.lib.dsx_calibration(mean, std, target, n, C, edges, nbins, z, nz, part, out, None))
    return out


def stats_from_sums(sums, edges, z, n):
    """The result object of ``calibration_stats`` from the (C, 3 * nbins + nz) sums on the host."""
    sums = np.asarray(sums, dtype=np.float64)
    edges, z = np.asarray(edges, dtype=np.float64), np.asarray(z, dtype=np.float64).reshape(-1)
    nbins = edges.shape[1] + 1
    bins = sums[:, :3 * nbins].reshape(-1, nbins, 3)
    count, sv, se = bins[..., 0], bins[..., 1], bins[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        rmv = np.where(count > 0, np.sqrt(sv / count), np.nan)
        rmse = np.where(count > 0, np.sqrt(se / count), np.nan)
    covered = sums[:, 3 * nbins:]
    return types.SimpleNamespace(edges=edges, z=z, n=int(n), count=count.astype(np.int64), sv=sv, se=se, rmv=rmv, rmse=rmse,
                                 covered=covered.astype(np.int64), coverage=covered / float(n))


def calibration_stats(mean, std, target, bins=30, z=(1, 2, 3), edges=None):
    """The calibration curve of (..., C) CUDA fp32 canvases -> an object of float64 numpy arrays: ``edges`` (C, bins - 1),
    ``count`` (C, bins) int64, ``rmv`` and ``rmse`` (C, bins) (NaN in an empty bin: many std values tying on an edge
    leave one, which is no error), ``coverage`` (C, len(z)) the share of pixels with |target - mean| <= z std, ``n``
    pixels per channel; also the raw ``sv``, ``se``, ``covered`` and ``z``.  ``edges=None``: equal-count bins of this
    very spread (``bin_edges``); given edges score another spread on the same bins."""
    std = _canvas(std, "std")
    if edges is None:
        edges = bin_edges(std, bins)
    edges = np.asarray(edges, dtype=np.float64)
    sums = calibration_sums(mean, std, target, edges, z).cpu().numpy()
    return stats_from_sums(sums, edges, z, std.numel() // std.shape[-1])


def fit(stats):
    """The line through the curve, per channel, float64 on the host -> {"a", "c", "scale"} of (C,) arrays.
    ``scale = sqrt(sum Se / sum Sv)``: the one factor that equates the mean predicted variance with the mean squared
    error.  ``(a, c)`` minimise ``sum_b count_b (rmse_b - a rmv_b - c)^2`` over the non-empty bins (closed form); with
    fewer than two non-empty bins, or rmv values that do not differ, ``a = scale`` and ``c = 0``."""
    C = stats.count.shape[0]
    a, c, scale = np.empty(C), np.empty(C), np.empty(C)
    for ch in range(C):
        tv, te = math.fsum(stats.sv[ch]), math.fsum(stats.se[ch])
        scale[ch] = math.sqrt(te / tv) if tv > 0 else float("nan")
        ok = stats.count[ch] > 0
        w, x, y = stats.count[ch][ok].astype(np.float64), stats.rmv[ch][ok], stats.rmse[ch][ok]
        a[ch], c[ch] = scale[ch], 0.0
        if w.size >= 2:
            W = w.sum()
            xm, ym = (w * x).sum() / W, (w * y).sum() / W
            sxx, sxy = (w * (x - xm) ** 2).sum(), (w * (x - xm) * (y - ym)).sum()
            if sxx > 0:
                a[ch] = sxy / sxx
                c[ch] = ym - a[ch] * xm
    return {"a": a, "c": c, "scale": scale}


def _floats(v):
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def _json_floats(v):
    """NaN (an empty bin) as null: strict JSON has no NaN; every other float64 as its repr, which reads back exactly"""
    return [None if math.isnan(x) else x for x in _floats(v)]


class Calibration:
    """A calibration curve with its fit, the sample count it holds for and the dataset's ``std_target``.

    The error of an N-sample mean depends on N, so a calibration fitted at ``samples`` posterior samples per tile is
    applied to spreads of ``samples`` samples only (``split --apply-calibration`` checks it)."""

    def __init__(self, stats, line, samples, std_target=None):
        self.stats, self.samples = stats, int(samples)
        self.a, self.c, self.scale = (np.asarray(line[k], dtype=np.float64).reshape(-1) for k in ("a", "c", "scale"))
        self.channels = int(stats.count.shape[0])
        self.std_target = None if std_target is None else np.asarray(std_target, dtype=np.float64).reshape(-1)
        if not (self.a.size == self.c.size == self.scale.size == self.channels):
            raise DsxError(f"calibration: a fit of {self.a.size} channels for a curve of {self.channels}")
        if self.samples < 2:
            raise DsxError(f"calibration: samples = {self.samples}; a spread needs 2 or more")

    @classmethod
    def from_stats(cls, stats, samples, std_target=None):
        return cls(stats, fit(stats), samples, std_target)

    def apply(self, std):
        """The recalibrated spread of a (..., C) tensor: ``(std.double() * a + c).clamp_min(0).float()`` per channel."""
        if std.shape[-1] != self.channels:
            raise DsxError(f"calibration: the spread has {std.shape[-1]} channels, the calibration {self.channels}")
        a = torch.as_tensor(self.a, dtype=torch.float64, device=std.device)
        c = torch.as_tensor(self.c, dtype=torch.float64, device=std.device)
        return (std.double() * a + c).clamp_min(0).float()

    def save(self, path):
        s = self.stats
        doc = {"format": FORMAT, "version": VERSION, "channels": self.channels, "samples": self.samples,
               "std_target": None if self.std_target is None else _floats(self.std_target),
               "fit": {"a": _json_floats(self.a), "c": _json_floats(self.c), "scale": _json_floats(self.scale)},
               "curve": {"bins": int(s.count.shape[1]), "n": int(s.n), "z": _floats(s.z), "edges": _floats(s.edges),
                         "count": [int(v) for v in s.count.reshape(-1)], "sv": _floats(s.sv), "se": _floats(s.se),
                         "rmv": _json_floats(s.rmv), "rmse": _json_floats(s.rmse),
                         "covered": [int(v) for v in s.covered.reshape(-1)], "coverage": _floats(s.coverage)}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, allow_nan=False)
            f.write("\n")

    @classmethod
    def load(cls, path):
        with open(path) as f:
            try:
                doc = json.load(f)
            except ValueError as e:
                raise DsxError(f"{path}: not a calibration file ({e})")
        if not isinstance(doc, dict) or doc.get("format") != FORMAT:
            raise DsxError(f"{path}: format {doc.get('format') if isinstance(doc, dict) else type(doc).__name__!r}, "
                           f"expected {FORMAT!r} (written by split --calibration)")
        if doc.get("version") != VERSION:
            raise DsxError(f"{path}: version {doc.get('version')!r} of the calibration file, this build reads version {VERSION}")
        try:
            C, cur, line = int(doc["channels"]), doc["curve"], doc["fit"]
            bins, nz = int(cur["bins"]), len(cur["z"])
            arr = lambda key, shape, dtype=np.float64: np.array(
                [np.nan if v is None else v for v in cur[key]], dtype=dtype).reshape(shape)
            stats = types.SimpleNamespace(
                edges=arr("edges", (C, bins - 1)), z=arr("z", (nz,)), n=int(cur["n"]), count=arr("count", (C, bins), np.int64),
                sv=arr("sv", (C, bins)), se=arr("se", (C, bins)), rmv=arr("rmv", (C, bins)), rmse=arr("rmse", (C, bins)),
                covered=arr("covered", (C, nz), np.int64), coverage=arr("coverage", (C, nz)))
            return cls(stats, {k: np.array([np.nan if v is None else v for v in line[k]], dtype=np.float64) for k in ("a", "c", "scale")}, doc["samples"],
                       doc["std_target"])
        except (KeyError, TypeError, ValueError) as e:
            raise DsxError(f"{path}: not a complete calibration file ({type(e).__name__}: {e})")


# ---------------------------------------------------------------------------------------------------------------------
# The rank histogram (Talagrand diagram): a check of the N samples against ground truth that assumes no distribution.
# If the target is exchangeable with a pixel's N samples, its rank among them -- the number of samples strictly below
# it, ``predict_stack(..., ranks=True)['rank']`` -- is uniform on 0..N, and the band between the m-th smallest and the
# m-th largest sample holds the target with probability (N + 1 - 2 m) / (N + 1).
RANK_FORMAT = "diffsplitting_amd.rank_histogram"
RANK_VERSION = 1


def rank_histogram(rank, n):
    """The counts of a channel-last rank canvas (..., C) of ``n`` samples -> (C, n + 1) int64 numpy: ``hist[c][k]`` pixels
    of channel c have rank k.  One ``torch.bincount`` per channel on the integer image, exact; a value that is no
    integer in 0..n is refused."""
    n = int(n)
    if n < 1:
        raise DsxError(f"rank_histogram: n = {n} samples, must be positive")
    rank = rank if isinstance(rank, torch.Tensor) else torch.as_tensor(np.asarray(rank))
    if rank.dim() < 1 or rank.numel() == 0:
        raise DsxError(f"rank_histogram: a rank canvas (..., C) with pixels, got shape {tuple(rank.shape)}")
    C = rank.shape[-1]
    flat = rank.reshape(-1, C)
    ints = flat.to(torch.int64)
    if not bool((ints.to(flat.dtype) == flat).all()) or int(ints.min()) < 0 or int(ints.max()) > n:
        raise DsxError(f"rank_histogram: every rank must be an integer in 0..{n}")
    return np.stack([torch.bincount(ints[:, c], minlength=n + 1).cpu().numpy().astype(np.int64) for c in range(C)])


def interval_coverage(hist):
    """What a rank histogram (C, n + 1) says about the central bands -> an object of numpy arrays: ``m`` = 1 .. n // 2,
    ``nominal`` (len(m),) = (n + 1 - 2 m) / (n + 1), ``observed`` (C, len(m)) = hist[c][m : n - m + 1].sum() / pixels:
    the share of pixels whose target lies between the m-th smallest and the m-th largest sample; ``pixels`` per channel."""
    hist = np.asarray(hist, dtype=np.int64)
    if hist.ndim != 2 or hist.shape[1] < 2:
        raise DsxError(f"interval_coverage: a histogram (C, n + 1), got shape {hist.shape}")
    n = hist.shape[1] - 1
    pixels = hist.sum(axis=1)
    if (pixels < 1).any() or (pixels != pixels[0]).any():
        raise DsxError(f"interval_coverage: every channel must hold the same positive pixel count, got {pixels.tolist()}")
    m = np.arange(1, n // 2 + 1, dtype=np.int64)
    nominal = (n + 1 - 2 * m) / float(n + 1)
    observed = np.array([[hist[c, k:n - k + 1].sum() / float(pixels[c]) for k in m] for c in range(hist.shape[0])],
                        dtype=np.float64).reshape(hist.shape[0], m.size)
    return types.SimpleNamespace(m=m, nominal=nominal, observed=observed, pixels=int(pixels[0]), samples=n)


def save_rank_histogram(path, hist):
    """The histogram and its bands as JSON: {"format", "version", "channels", "samples", "pixels", "hist" (channels rows
    of samples + 1 counts), "intervals" (one {"m", "nominal", "observed" per channel} per band)}."""
    hist = np.asarray(hist, dtype=np.int64)
    cov = interval_coverage(hist)
    doc = {"format": RANK_FORMAT, "version": RANK_VERSION, "channels": int(hist.shape[0]), "samples": cov.samples,
           "pixels": cov.pixels, "hist": [[int(v) for v in row] for row in hist],
           "intervals": [{"m": int(m), "nominal": float(cov.nominal[j]), "observed": _floats(cov.observed[:, j])}
                         for j, m in enumerate(cov.m)]}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, allow_nan=False)
        f.write("\n")
    return doc


def load_rank_histogram(path):
    """-> the (C, n + 1) int64 histogram of a file ``save_rank_histogram`` wrote."""
    with open(path) as f:
        try:
            doc = json.load(f)
        except ValueError as e:
            raise DsxError(f"{path}: not a rank histogram file ({e})")
    if not isinstance(doc, dict) or doc.get("format") != RANK_FORMAT:
        raise DsxError(f"{path}: format {doc.get('format') if isinstance(doc, dict) else type(doc).__name__!r}, "
                       f"expected {RANK_FORMAT!r} (written by split --rank-histogram)")
    if doc.get("version") != RANK_VERSION:
        raise DsxError(f"{path}: version {doc.get('version')!r} of the rank histogram file, this build reads version "
                       f"{RANK_VERSION}")
    try:
        hist = np.array(doc["hist"], dtype=np.int64).reshape(int(doc["channels"]), int(doc["samples"]) + 1)
        if int(doc["pixels"]) != int(hist[0].sum()):
            raise ValueError(f"{doc['pixels']} pixels, the counts sum to {int(hist[0].sum())}")
    except (KeyError, TypeError, ValueError) as e:
        raise DsxError(f"{path}: not a complete rank histogram file ({type(e).__name__}: {e})")
    return hist
