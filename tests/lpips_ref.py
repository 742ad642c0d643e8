"""LPIPS (AlexNet trunk, v0.1 linear heads, spatial off) restated in torch on the CPU, float64 by default.

Written from the description of the algorithm, not from any package source; parity of the device code is pinned against
this restatement and is unpinned against the ``lpips`` package itself (tests/test_lpips_cpu.py compares the two when the
package and a local weight file are present).

  scaling layer   (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  trunk           conv 3->64 11x11 /4 pad 2 + ReLU [tap 1] - maxpool 3x3 /2 (floor) - conv 64->192 5x5 pad 2 + ReLU [tap 2]
                  - maxpool 3x3 /2 - conv 192->384 3x3 pad 1 + ReLU [tap 3] - conv 384->256 + ReLU [tap 4]
                  - conv 256->256 + ReLU [tap 5]
  per tap         f / (sqrt(sum_c f^2) + 1e-10) for both images, squared difference, 1x1 `lin` weights (no bias), mean
                  over space
  result          sum of the five tap values

Also here: the seeded weight synthesiser (lpips key layout), the test cases shared by the CPU and GPU suites, and the
tolerance the GPU suite uses -- derived from the error of this same restatement evaluated in float32, never from the
device's output.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
TRUNK = ((1, 0, (64, 3, 11, 11)), (2, 3, (192, 64, 5, 5)), (3, 6, (384, 192, 3, 3)), (4, 8, (256, 384, 3, 3)),
         (5, 10, (256, 256, 3, 3)))
LIN_CHANNELS = (64, 192, 384, 256, 256)
DEFECTS = ("no_eps", "ceil_pool", "conv2_pad1", "swap_lin", "fold_scaling")


def synth_state_dict(seed=0):
    """Seeded weights in the key layout of lpips.LPIPS.state_dict().  Trunk weights are He-scaled (std sqrt(2 / fan_in))
    so activations stay O(1) through the five layers; biases are small, those of conv1 negative so that an input whose
    scaled value is zero gives all-zero tap-1 features (the case in which the 1e-10 of the normalisation matters); `lin`
    weights are non-negative, as the trained ones are."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, idx, shape in TRUNK:
        fan_in = shape[1] * shape[2] * shape[3]
        sd[f"net.slice{k}.{idx}.weight"] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        b = torch.randn(shape[0], generator=g) * 0.1
        sd[f"net.slice{k}.{idx}.bias"] = -(b.abs() + 0.05) if k == 1 else b
    for k, ch in enumerate(LIN_CHANNELS):
        sd[f"lin{k}.model.1.weight"] = torch.rand((1, ch, 1, 1), generator=g) * 0.2
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def to_split_layout(sd):
    """The same weights under the split key layout: torchvision ``features.*`` + alex.pth's ``lin*``."""
    out = {}
    for k, idx, _ in TRUNK:
        for leaf in ("weight", "bias"):
            out[f"features.{idx}.{leaf}"] = sd[f"net.slice{k}.{idx}.{leaf}"]
    for k in range(5):
        out[f"lin{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    return out


def lpips_ref(sd, in0, in1, dtype=torch.float64, defect=None, per_layer=False):
    """LPIPS of (B, 3, H, W) pairs in [-1, 1] -> (B,) tensor of ``dtype`` (and the (B, 5) tap values).  ``defect``: one
    of DEFECTS, a deliberate mistake for the sensitivity test."""
    assert defect is None or defect in DEFECTS
    w = [sd[f"net.slice{k}.{idx}.weight"].to(dtype) for k, idx, _ in TRUNK]
    b = [sd[f"net.slice{k}.{idx}.bias"].to(dtype) for k, idx, _ in TRUNK]
    lin = [sd[f"lin{k}.model.1.weight"].to(dtype).view(1, -1, 1, 1) for k in range(5)]
    if defect == "swap_lin":
        lin[3], lin[4] = lin[4], lin[3]
    # the constants are the float32 values the device applies
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    eps = 0.0 if defect == "no_eps" else 1e-10
    ceil = defect == "ceil_pool"

    def trunk(x):
        x = x.to(dtype)
        if defect == "fold_scaling":
            # the constant term of the scaling layer moved into conv1's bias: equal inside, wrong where conv1 pads
            b0 = b[0] - (w[0] * (shift / scale)).sum(dim=(1, 2, 3))
            h = F.relu(F.conv2d(x / scale, w[0], b0, stride=4, padding=2))
        else:
            h = F.relu(F.conv2d((x - shift) / scale, w[0], b[0], stride=4, padding=2))
        taps = [h]
        h = F.max_pool2d(h, 3, 2, ceil_mode=ceil)
        h = F.relu(F.conv2d(h, w[1], b[1], padding=1 if defect == "conv2_pad1" else 2))
        taps.append(h)
        h = F.max_pool2d(h, 3, 2, ceil_mode=ceil)
        for l in (2, 3, 4):
            h = F.relu(F.conv2d(h, w[l], b[l], padding=1))
            taps.append(h)
        return taps

    t0, t1 = trunk(in0), trunk(in1)
    vals = []
    for k in range(5):
        n0 = t0[k] / (t0[k].pow(2).sum(dim=1, keepdim=True).sqrt() + eps)
        n1 = t1[k] / (t1[k].pow(2).sum(dim=1, keepdim=True).sqrt() + eps)
        vals.append(((n0 - n1) ** 2 * lin[k]).sum(dim=1).mean(dim=(1, 2)))
    taps = torch.stack(vals, dim=1)
    total = taps.sum(dim=1)
    return (total, taps) if per_layer else total


def frames_prepare(target, pred, ch):
    """compute_lpips' preparation of one channel (notebooks/EvaluateJointIndiIterative.ipynb cell 28), in the float32
    numpy arithmetic the notebook runs on float32 frames: (N, H, W, C) -> two (N, 3, H, W) arrays."""
    target = np.asarray(target, dtype=np.float32).transpose(0, 3, 1, 2)
    pred = np.asarray(pred, dtype=np.float32).transpose(0, 3, 1, 2)
    tar = np.repeat(target[:, ch:ch + 1], 3, axis=1)
    prd = np.repeat(pred[:, ch:ch + 1], 3, axis=1)
    max_val, min_val = tar.max(), tar.min()
    tar = 2 * (tar - min_val) / (max_val - min_val) - 1
    prd = 2 * (prd - min_val) / (max_val - min_val) - 1
    assert tar.dtype == np.float32 and prd.dtype == np.float32
    return tar, prd


def frames_ref(sd, target, pred, dtype=torch.float64):
    """compute_lpips(target, pred) -> {channel: (N,) tensor}."""
    out = {}
    for ch in range(target.shape[3]):
        tar, prd = frames_prepare(target, pred, ch)
        out[ch] = lpips_ref(sd, torch.from_numpy(tar), torch.from_numpy(prd), dtype)
    return out


# ---------------------------------------------------------------- cases shared by the CPU and GPU suites
# name -> (B, H, W, seed)
CASES = {"b1_64": (1, 64, 64, 1), "b3_64": (3, 64, 64, 2), "b1_97x131": (1, 97, 131, 3), "b3_97x131": (3, 97, 131, 4),
         "b1_255x256": (1, 255, 256, 5), "b1_512": (1, 512, 512, 6)}


def make_pair(B, H, W, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    in0 = torch.rand((B, 3, H, W), generator=g) * 2 - 1
    in1 = (in0 + 0.3 * torch.randn((B, 3, H, W), generator=g)).clamp(-1, 1)
    return in0, in1


def constant_image(B, H, W):
    """Every pixel equal to the scaling layer's shift: the scaled input is exactly zero, and with synth_state_dict's
    negative conv1 biases every tap-1 feature vector is all zero."""
    return torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1).expand(B, 3, H, W).contiguous()


def make_frames(seed=7, shape=(3, 160, 192, 2)):
    """Target and prediction frame stacks with a non-trivial range (nothing like [-1, 1] or [0, 1])."""
    g = torch.Generator().manual_seed(2000 + seed)
    target = torch.rand(shape, generator=g) * 37.5 + 3.25
    target[..., 1] = target[..., 1] * 0.01 - 4.0
    pred = target + torch.randn(shape, generator=g) * torch.tensor([3.0, 0.03])
    return target.numpy(), pred.numpy()


ABS_FLOOR = 1e-7     # about one float32 ulp at the metric's O(1) scale: for values near 0
MARGIN = 4.0         # the MFMA chain sums K (up to 3456 terms) in another order than ATen's float32 kernels


@functools.lru_cache(maxsize=None)
def fp32_yardstick(seed=0):
    """The yardstick of the device tolerance: over CASES (totals and per-tap values), the constant-image case and the
    frames case, the largest relative error of THIS restatement evaluated in float32 against its float64 form."""
    sd = synth_state_dict(seed)
    worst = 0.0

    def upd(a32, a64):
        nonlocal worst
        rel = ((a32.double() - a64).abs() / a64.abs().clamp_min(1e-30)).max().item()
        worst = max(worst, rel)

    with torch.no_grad():
        for B, H, W, s in CASES.values():
            in0, in1 = make_pair(B, H, W, s)
            t64, p64 = lpips_ref(sd, in0, in1, torch.float64, per_layer=True)
            t32, p32 = lpips_ref(sd, in0, in1, torch.float32, per_layer=True)
            upd(t32, t64)
            upd(p32, p64)
        in0, in1 = constant_image(1, 64, 64), make_pair(1, 64, 64, 9)[1]
        upd(lpips_ref(sd, in0, in1, torch.float32), lpips_ref(sd, in0, in1, torch.float64))
        tgt, prd = make_frames()
        r64, r32 = frames_ref(sd, tgt, prd, torch.float64), frames_ref(sd, tgt, prd, torch.float32)
        for ch in r64:
            upd(r32[ch], r64[ch])
    return worst


def bound(expected, seed=0):
    """|device - float64| allowed at each element of ``expected``: MARGIN x yardstick, relative, plus ABS_FLOOR."""
    return MARGIN * fp32_yardstick(seed) * expected.abs().double() + ABS_FLOOR
