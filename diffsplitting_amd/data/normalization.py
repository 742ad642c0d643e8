"""The normalisation of a dataset as a file: what ``SplitDataset.get_normalization_dict()`` returns, with the settings
it was computed under, written once where the training data is and read where only a stack to split is
(``split --save-norm`` / ``split --input ... --norm``).

One JSON object.  Every number is written as ``float(value)``: ``json`` writes ``repr``, which reads back as the same
float64, so a set normalised with the loaded dict cuts the same tiles bit for bit.  ``load_normalization`` returns the
scalars as ``np.float64`` and the arrays as float64 numpy arrays: the normalisation arithmetic runs in float64 because its
statistics are "strong" float64 values (``quantile_device`` in split_dataset.py), a Python float would do the same, a
float32 would not."""
import json
import math

import numpy as np

from .._lib import DsxError

FORMAT = "diffsplitting_amd.normalization"
VERSION = 1
SCALARS = ("mean_input", "std_input", "target0_max", "target1_max", "input_max")
ARRAYS = ("mean_target", "std_target")
_OPTIONAL = ("target0_max", "target1_max", "input_max")      # None in a dict that was given without them
SETTINGS = ("data_type", "channel_weights", "max_qval", "upper_clip", "target_channel_idx")


def _number(v, what):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise DsxError(f"normalisation: {what} = {v!r} is not a number")
    if not math.isfinite(f):
        raise DsxError(f"normalisation: {what} = {f!r} is not finite")
    return f


def save_normalization(path, normalization_dict, *, data_type, channel_weights, max_qval, upper_clip,
                       target_channel_idx):
    """Write ``normalization_dict`` (the seven entries of ``get_normalization_dict()``) and the dataset settings to
    ``path``.  Non-finite values and a non-positive std are refused here too: such a file could not be loaded."""
    nd = {}
    for k in SCALARS + ARRAYS:
        if k not in normalization_dict:
            raise DsxError(f"normalisation: the dict has no {k!r}")
        v = normalization_dict[k]
        if k in ARRAYS:
            nd[k] = [_number(x, k) for x in np.asarray(v, dtype=np.float64).reshape(-1)]
        else:
            nd[k] = None if (v is None and k in _OPTIONAL) else _number(v, k)
    _check_std(nd)
    doc = {"format": FORMAT, "version": VERSION, "data_type": str(data_type),
           "channel_weights": None if channel_weights is None else [_number(w, "channel_weights") for w in channel_weights],
           "max_qval": None if max_qval is None else _number(max_qval, "max_qval"), "upper_clip": bool(upper_clip),
           "target_channel_idx": None if target_channel_idx is None else int(target_channel_idx), "normalization": nd}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, allow_nan=False)
        f.write("\n")


def _check_std(nd):
    if len(nd["mean_target"]) != len(nd["std_target"]) or not nd["std_target"]:
        raise DsxError(f"normalisation: mean_target / std_target hold {len(nd['mean_target'])} / {len(nd['std_target'])} "
                       "values: one pair per target channel")
    for k, vals in (("std_input", [nd["std_input"]]), ("std_target", nd["std_target"])):
        for v in vals:
            if not v > 0.0:
                raise DsxError(f"normalisation: {k} = {v!r} must be positive")


def load_normalization(path):
    """-> ``(normalization_dict, meta)``: the dict with ``np.float64`` scalars and float64 arrays (usable as
    ``SplitDataset(..., normalization_dict=...)``), ``meta`` the settings (``data_type``, ``channel_weights``,
    ``max_qval``, ``upper_clip``, ``target_channel_idx``).  Another format or version, a missing key, a non-finite
    number and a non-positive std are refused by name."""
    with open(path) as f:
        try:
            doc = json.load(f)
        except ValueError as e:
            raise DsxError(f"{path}: not a normalisation file ({e})")
    if not isinstance(doc, dict) or doc.get("format") != FORMAT:
        raise DsxError(f"{path}: format {doc.get('format') if isinstance(doc, dict) else type(doc).__name__!r}, "
                       f"expected {FORMAT!r} (written by split --save-norm)")
    if doc.get("version") != VERSION:
        raise DsxError(f"{path}: version {doc.get('version')!r} of the normalisation file, this build reads version {VERSION}")
    for k in SETTINGS + ("normalization",):
        if k not in doc:
            raise DsxError(f"{path}: the key {k!r} is missing")
    raw = doc["normalization"]
    if not isinstance(raw, dict):
        raise DsxError(f"{path}: 'normalization' must be an object")
    nd = {}
    for k in SCALARS + ARRAYS:
        if k not in raw:
            raise DsxError(f"{path}: the key 'normalization.{k}' is missing")
        v = raw[k]
        if k in ARRAYS:
            if not isinstance(v, list):
                raise DsxError(f"{path}: normalization.{k} must be a list")
            nd[k] = [_number(x, f"{path}: {k}") for x in v]
        else:
            nd[k] = None if (v is None and k in _OPTIONAL) else _number(v, f"{path}: {k}")
    try:
        _check_std(nd)
    except DsxError as e:
        raise DsxError(f"{path}: {e}")
    out = {k: (None if nd[k] is None else np.float64(nd[k])) for k in SCALARS}
    out.update({k: np.asarray(nd[k], dtype=np.float64) for k in ARRAYS})
    meta = {k: doc[k] for k in SETTINGS}
    meta.update(format=doc["format"], version=doc["version"])
    return out, meta
