"""Writes tests/golden/validation_L.npz and validation_RGB.npz with the REFERENCE's own text doing the work.

    python tools/gen_validation_golden.py /path/to/reference/checkout

The validation block of the reference's training loop is not a function, so its text is read from ``split.py`` at run
time, cut between two anchor statements -- from ``visuals = diffusion.get_current_visuals()`` up to the first
``Metrics.save_img(`` -- dedented and ``exec``-ed with stand-ins for the names it uses: a ``diffusion`` whose
``get_current_visuals`` returns one item, a ``val_set`` with ``get_normalization_dict``, the reference's own
``core.psnr.PSNR`` and a ``psnr_values`` dict.  It runs once up to ``if mode != 'RGB'`` (the quantised arrays and the
PSNR values) and once in full (the [0, 1] images).  Only arrays are stored: inputs, normalisation, quantised arrays,
PSNR values, images, and the integer statistics and numerators that this script derives from the reference's quantised
arrays in int64 numpy (and checks against the reference's images).  None of the block's text is stored.

Cases: 'L' (B = 3, Cin = 1, C = 2) on planes of 5 x 7 (keys p5x7_*) and 64 x 64 (p64x64_*), 'RGB' (B = 2, Cin = 3,
C = 6) on 8 x 8.  Targets are float32((raw - mean) / std) of integer raw counts.
"""
import os
import sys
import textwrap
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A0, A1, AMID = "visuals = diffusion.get_current_visuals()", "Metrics.save_img(", "if mode != 'RGB':"


def cut_block(ref):
    lines = open(os.path.join(ref, "split.py")).read().split("\n")
    i0 = [i for i, l in enumerate(lines) if l.strip() == A0]
    assert len(i0) >= 1, "first anchor not found"
    i0 = i0[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(A1))
    full = textwrap.dedent("\n".join(lines[i0:i1]))
    imid = next(i for i in range(i0, i1) if lines[i].strip() == AMID)
    head = textwrap.dedent("\n".join(lines[i0:imid]))
    compile(full, "<validation block>", "exec")
    compile(head, "<validation block, first part>", "exec")
    return head, full


class _Diffusion:
    def __init__(self, item):
        self.item = item

    def get_current_visuals(self):
        return {k: torch.from_numpy(v.copy()) for k, v in self.item.items()}


class _ValSet:
    def __init__(self, nd):
        self.nd = nd

    def get_normalization_dict(self):
        return self.nd


def run(text, item, nd, PSNR):
    ns = {"np": np, "torch": torch, "diffusion": _Diffusion(item), "val_set": _ValSet(nd), "PSNR": PSNR,
          "psnr_values": defaultdict(list)}
    exec(text, ns)
    return ns


def make_case(rng, B, Cin, C, H, W, nd, raw_lo, raw_hi):
    """Inputs of one case: integer raw counts, normalised as the dataset does; the prediction is the target plus noise
    with a few pixels pushed past both ends of the clamp."""
    mean_t, std_t = nd["mean_target"], nd["std_target"]
    raw = rng.integers(raw_lo, raw_hi, size=(B, C, H, W)).astype(np.float64)
    target = ((raw - mean_t) / std_t).astype(np.float32)
    raw_in = raw.reshape(B, C // Cin, Cin, H, W).sum(axis=1)           # the input is the sum of the C / Cin images
    inp = ((raw_in - nd["mean_input"]) / nd["std_input"]).astype(np.float32)
    pred = (target + rng.normal(0.0, 0.35, size=target.shape)).astype(np.float32)
    flat = pred.reshape(B, C, -1)
    flat[:, :, 1] = ((-37.5 - mean_t) / std_t).reshape(1, C)           # below 0: clamped to 0
    flat[:, :, 3] = ((70000.0 - mean_t) / std_t).reshape(1, C)         # above 65535: clamped to 65535
    return {"input": inp, "target": target, "prediction": pred, "raw": raw}


def reference_case(head, full, PSNR, case, nd):
    B = case["target"].shape[0]
    out = defaultdict(list)
    for b in range(B):
        item = {k: case[k][b:b + 1] for k in ("input", "target", "prediction")}
        ns = run(head, item, nd, PSNR)
        for k in ("input_img", "target_img", "pred_img"):
            assert ns[k].dtype == np.uint16, (k, ns[k].dtype)
            out[k[:-4] + "_q"].append(ns[k])
        keys = sorted(ns["psnr_values"])
        out["psnr"].append([ns["psnr_values"][k][0] for k in keys])
        out["mode"] = ns["mode"]
        out["psnr_keys"] = keys
        if ns["mode"] != "RGB":
            ns = run(full, item, nd, PSNR)
            for k in ("input_img", "target_img", "pred_img"):
                assert ns[k].dtype == np.float64, (k, ns[k].dtype)
                out[k].append(ns[k])
    res = {k: (np.stack(v) if isinstance(v, list) and k not in ("psnr_keys",) else v) for k, v in out.items()}
    res["psnr"] = np.asarray(out["psnr"], dtype=np.float64)
    res["psnr_keys"] = np.asarray(out["psnr_keys"], dtype=np.int64)
    return res


def derive_and_check(case, ref, nd):
    """Integer statistics and numerators from the reference's quantised arrays (int64 numpy), the fixture's own
    properties, and undefined == 0 for these inputs."""
    tq, pq, iq = (ref[k].astype(np.int64) for k in ("target_q", "pred_q", "input_q"))
    B, C = tq.shape[:2]
    f = lambda a: a.reshape(a.shape[0], a.shape[1], -1)
    st = {"ssd": ((f(tq) - f(pq)) ** 2).sum(axis=2), "tmin": f(tq).min(axis=2), "tmax": f(tq).max(axis=2),
          "imin": f(iq).min(axis=2), "imax": f(iq).max(axis=2)}
    # the values in front of the casts, restated: nothing undefined in the reference's own inputs
    tv = case["target"] * nd["std_target"] + nd["mean_target"]
    pv = case["prediction"] * nd["std_target"] + nd["mean_target"]
    iv = (case["input"] * nd["std_input"] + nd["mean_input"]) / 2
    assert tv.dtype == pv.dtype == iv.dtype == np.float64
    for v in (tv, iv):
        assert np.isfinite(v).all() and (v >= 0).all() and (v < 65536).all()
    assert np.isfinite(pv).all()
    st["undefined"] = np.int64(0)
    assert np.array_equal(tv.astype(np.uint16), ref["target_q"]) and np.array_equal(iv.astype(np.uint16), ref["input_q"])
    # truncation is exercised, both sides of the clamp, and the wrap below the target's minimum
    assert (tq == case["raw"].astype(np.int64) - 1).any(), "no target pixel quantises to raw - 1"
    assert (pv < 0).any() and (pv > 65535).any(), "the clamp is not exercised on both sides"
    below = pq < st["tmin"][:, :, None, None]
    assert below.reshape(B, C, -1).any(axis=2).all(), "a channel without a prediction below the target's minimum"
    if ref["mode"] != "RGB":
        tmin, tden = st["tmin"][:, :, None, None], (st["tmax"] - st["tmin"])[:, :, None, None]
        imin_item = st["imin"].min(axis=1)[:, None, None, None]
        iden = st["imax"][:, :, None, None] - imin_item
        st["target_n"] = (tq - tmin).astype(np.uint16)
        st["input_n"] = (iq - imin_item).astype(np.uint16)
        st["pred_n"] = np.minimum((pq - tmin) % 65536, tden).astype(np.uint16)
        assert np.array_equal(st["target_n"] / tden.astype(np.uint16), ref["target_img"])
        assert np.array_equal(st["input_n"] / iden.astype(np.uint16), ref["input_img"])
        assert np.array_equal(st["pred_n"] / tden.astype(np.uint16), ref["pred_img"])
        assert (ref["pred_img"][below] == 1.0).all()                   # the wrapped pixels come out as 1
    return st


def pack(prefix, case, ref, st, nd):
    out = {k: case[k] for k in ("input", "target", "prediction")}
    out.update({k: np.asarray(nd[k], dtype=np.float64) for k in ("mean_input", "std_input", "mean_target", "std_target")})
    out.update({k: ref[k] for k in ref if k != "mode"})
    out.update(st)
    return {prefix + k: v for k, v in out.items()}


def save(name, arrs):
    arrs.update(torch_version=np.array(torch.__version__), numpy_version=np.array(np.__version__))
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def main(ref):
    head, full = cut_block(ref)
    sys.path.insert(0, ref)
    from core.psnr import PSNR
    rng = np.random.default_rng(20251018)
    # 'L': the Hagen normalisation (mean = std = quantile / 2, compute_normalization_dict)
    t0, t1 = np.float64(1519.37), np.float64(973.81)
    nd = {"mean_input": (t0 + t1) / 2, "std_input": (t0 + t1) / 2,
          "mean_target": np.array([t0 / 2, t1 / 2]).reshape(-1, 1, 1), "std_target": np.array([t0 / 2, t1 / 2]).reshape(-1, 1, 1)}
    arrs = {}
    for H, W in ((5, 7), (64, 64)):
        case = make_case(rng, 3, 1, 2, H, W, nd, 90, 1400)
        ref_out = reference_case(head, full, PSNR, case, nd)
        assert ref_out["mode"] == "L" and list(ref_out["psnr_keys"]) == [0, 1]
        arrs.update(pack(f"p{H}x{W}_", case, ref_out, derive_and_check(case, ref_out, nd), nd))
    save("validation_L", arrs)
    # 'RGB': the uint8 normalisation (127.5 per channel, the input the sum of two images)
    nd = {"mean_input": np.float64(255.0), "std_input": np.float64(255.0),
          "mean_target": np.array([127.5] * 6).reshape(-1, 1, 1), "std_target": np.array([127.5] * 6).reshape(-1, 1, 1)}
    case = make_case(rng, 2, 3, 6, 8, 8, nd, 3, 256)
    ref_out = reference_case(head, full, PSNR, case, nd)
    assert ref_out["mode"] == "RGB" and list(ref_out["psnr_keys"]) == [0, 3]
    save("validation_RGB", pack("", case, ref_out, derive_and_check(case, ref_out, nd), nd))


if __name__ == "__main__":
    main(sys.argv[1])
