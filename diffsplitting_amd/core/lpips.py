"""LPIPS (AlexNet, version 0.1, spatial off) on the MI355X: the ``lpips.LPIPS(net='alex')`` the evaluation notebooks
build (notebooks/EvaluateJointIndi.ipynb cell 31, EvaluateJointIndiIterative.ipynb cell 28), on ``dsx_lpips_*``
(include/dsx.h).

Weights are always supplied by the caller -- a state dict, a local file, or the file(s) the environment variable
``DSX_LPIPS_WEIGHTS`` names -- and are never fetched.  Two key layouts are accepted: ``lpips.LPIPS.state_dict()``'s
(``net.slice{1..5}.{0,3,6,8,10}.{weight,bias}``, ``lin{0..4}.model.1.weight``) and the split form (torchvision's
AlexNet ``features.{0,3,6,8,10}.*`` plus the ``lin{k}.model.1.weight`` of the package's ``alex.pth``).  There is no CPU
fallback: ``forward`` raises DsxError without a HIP device.  Parity is checked against a float64 restatement of the
algorithm (tests/lpips_ref.py); it is unpinned against the ``lpips`` package itself.
"""
import ctypes as C
import os

import torch

from .. import _lib
from .._lib import DsxError, check, lib

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (slice, index inside torchvision's features, weight shape)
TRUNK = ((1, 0, (64, 3, 11, 11)), (2, 3, (192, 64, 5, 5)), (3, 6, (384, 192, 3, 3)), (4, 8, (256, 384, 3, 3)),
         (5, 10, (256, 256, 3, 3)))
LIN_CHANNELS = (64, 192, 384, 256, 256)
ENV = "DSX_LPIPS_WEIGHTS"

_NO_WEIGHTS = (
    "LPIPS needs its weights from the caller and never fetches them. Supply two local files (or one state dict "
    "holding both): torchvision's ImageNet AlexNet checkpoint (keys features.{0,3,6,8,10}.weight/bias) and the lpips "
    "package's weights/v0.1/alex.pth (keys lin{0..4}.model.1.weight) -- as state_dict=, as weights_path= (one path or "
    f"a list of paths), or as {ENV}=<path>[{os.pathsep}<path>]. A saved lpips.LPIPS(net='alex').state_dict() "
    "holds both.")


def _load_files(paths):
    if isinstance(paths, (str, os.PathLike)):
        paths = [p for p in os.fspath(paths).split(os.pathsep) if p]
    sd = {}
    for p in paths:
        if not os.path.isfile(p):
            raise DsxError(f"LPIPS weight file {p!r} does not exist. " + _NO_WEIGHTS)
        part = torch.load(p, map_location="cpu", weights_only=True)
        if not isinstance(part, dict):
            raise DsxError(f"LPIPS weight file {p!r} does not hold a state dict")
        sd.update(part)
    return sd


def split_state_dict(sd):
    """A state dict in either accepted key layout -> (10 trunk tensors, 5 lin tensors), fp32 CPU contiguous, shapes
    checked by key name.  Raises DsxError on a missing or unknown key, a wrong shape, or scaling-layer buffers that
    differ from the constants the kernels apply."""
    sd = dict(sd)
    trunk, lin = [], []
    used = set()

    def take(names, shape):
        for n in names:
            if n in sd:
                t = torch.as_tensor(sd[n]).detach()
                if tuple(t.shape) != tuple(shape):
                    raise DsxError(f"LPIPS weights: {n} has shape {tuple(t.shape)}, expected {tuple(shape)}")
                used.add(n)
                return t.to(torch.float32).cpu().contiguous()
        raise DsxError(f"LPIPS weights: missing {' (or '.join(names)}{')' if len(names) > 1 else ''}. " + _NO_WEIGHTS)

    for k, idx, shape in TRUNK:
        trunk.append(take((f"net.slice{k}.{idx}.weight", f"features.{idx}.weight"), shape))
        trunk.append(take((f"net.slice{k}.{idx}.bias", f"features.{idx}.bias"), shape[:1]))
    for k, ch in enumerate(LIN_CHANNELS):
        lin.append(take((f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"), (1, ch, 1, 1)))
    for name, const in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
        if name in sd:
            got = torch.as_tensor(sd[name]).detach().to(torch.float32).flatten()
            if got.numel() != 3 or not torch.equal(got, torch.tensor(const, dtype=torch.float32)):
                raise DsxError(f"LPIPS weights: {name} = {got.tolist()} differs from the v0.1 constants {const}")
            used.add(name)
    known = _alias_names()
    for n in sd:
        # the other layout's spelling of a tensor already taken, the package's `lins` list, torchvision's classifier
        if n in used or n in known or n.startswith(("lins.", "classifier.")):
            continue
        raise DsxError(f"LPIPS weights: unexpected key {n!r} (an AlexNet v0.1 state dict has net.slice*/features.*, "
                       "lin*.model.1.weight and scaling_layer.* only)")
    return trunk, lin


def _alias_names():
    names = set()
    for k, idx, _ in TRUNK:
        for leaf in ("weight", "bias"):
            names.add(f"net.slice{k}.{idx}.{leaf}")
            names.add(f"features.{idx}.{leaf}")
    for k in range(5):
        names.add(f"lin{k}.model.1.weight")
    return names


STAGES = ("x0", "f1", "p1", "f2", "p2", "f3", "f4", "f5")
# the launch that writes each stage (dsx_lpips.hip)
STAGE_LAUNCH = {"x0": "k_lpips_input_nchw", "f1": "k_lpips_conv1", "p1": "k_lpips_pool", "f2": "k_lpips_conv<5>",
                "p2": "k_lpips_pool", "f3": "k_lpips_conv<3>", "f4": "k_lpips_conv<3>", "f5": "k_lpips_conv<3>"}
TAP_STAGES = ("f1", "f2", "f3", "f4", "f5")


def geometry(H, W):
    """Stage name -> (H, W, C) of every stage of the trunk for an H x W input (dsx_lpips.cpp's geometry())."""
    if H < 31 or W < 31:
        raise DsxError(f"LPIPS(alex) needs H, W >= 31: below that the second max-pool has no output (got {H} x {W})")
    conv1 = lambda n: (n + 4 - 11) // 4 + 1
    pool = lambda n: (n - 3) // 2 + 1
    h1, w1 = conv1(H), conv1(W)
    h2, w2 = pool(h1), pool(w1)
    h3, w3 = pool(h2), pool(w2)
    return {"x0": (H, W, 3), "f1": (h1, w1, 64), "p1": (h2, w2, 64), "f2": (h2, w2, 192), "p2": (h3, w3, 192),
            "f3": (h3, w3, 384), "f4": (h3, w3, 256), "f5": (h3, w3, 256)}


class LPIPS(torch.nn.Module):
    """``lpips.LPIPS(net='alex', version='0.1', spatial=False)`` with caller-supplied weights.

    ``forward(in0, in1, retPerLayer=False, normalize=False)``: (B, 3, H, W) (or (3, H, W)) pairs in [-1, 1]
    ([0, 1] with ``normalize=True``) -> (B, 1, 1, 1) on the device, plus the list of the five tap values with
    ``retPerLayer=True``."""

    def __init__(self, net='alex', version='0.1', spatial=False, state_dict=None, weights_path=None):
        super().__init__()
        if net not in ('alex', 'alexnet'):
            raise DsxError(f"LPIPS(net={net!r}) is not built: only net='alex' (VGG and SqueezeNet trunks are out of scope)")
        if str(version) != '0.1':
            raise DsxError(f"LPIPS(version={version!r}) is not built: only version='0.1'")
        if spatial:
            raise DsxError("LPIPS(spatial=True) is not built: only the spatial average (spatial=False)")
        if state_dict is None:
            path = weights_path or os.environ.get(ENV)
            if not path:
                raise DsxError(_NO_WEIGHTS)
            state_dict = _load_files(path)
        trunk, lin = split_state_dict(state_dict)
        self._keep = trunk + lin                                       # host tensors the library reads during create
        cnt = lambda ts: (C.c_int64 * len(ts))(*[t.numel() for t in ts])
        h = C.c_void_p()
        check(lib.dsx_lpips_create(_lib.host_pointers(trunk), cnt(trunk), _lib.host_pointers(lin), cnt(lin), C.byref(h)))
        self._h = h
        self._keep = None

    def __del__(self):
        h = self.__dict__.get("_h")
        if h:
            self.__dict__["_h"] = None
            lib.dsx_lpips_destroy(h)

    @staticmethod
    def _device(*tensors):
        _lib.require_gpu()
        for t in tensors:
            if t.is_cuda:
                return t.device
        return torch.device("cuda", torch.cuda.current_device())

    @torch.no_grad()
    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        dev = self._device(in0, in1)
        if in0.dim() == 3:
            in0, in1 = in0[None], in1[None]
        if in0.shape != in1.shape or in0.dim() != 4 or in0.shape[1] != 3:
            raise ValueError(f"LPIPS takes two (B, 3, H, W) tensors of one shape, got {tuple(in0.shape)} and "
                             f"{tuple(in1.shape)}")
        a = in0.to(dev, torch.float32).contiguous()
        b = in1.to(dev, torch.float32).contiguous()
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        B, _, H, W = a.shape
        out = torch.empty((B,), dtype=torch.float32, device=dev)
        taps = torch.empty((B, 5), dtype=torch.float32, device=dev) if retPerLayer else None
        check(lib.dsx_lpips_forward(self._h, a, b, B, H, W, out, taps, None))
        self._table_dev = dev
        val = out.view(B, 1, 1, 1)
        if retPerLayer:
            return val, [taps[:, k].reshape(B, 1, 1, 1) for k in range(5)]
        return val

    @torch.no_grad()
    def layer_table(self, stages=None):
        """Every stage of the last ``forward`` copied out of the workspace (dsx_lpips_layers), for per-launch checks:
        ``{"pairs": B, "stages": {name: dict(out=(2B, H, W, C) fp32 NHWC device tensor, launch=<kernel that wrote
        it>)}, "taps": [dict(stage, launch, part=(B, nblk) float64 partial rows, nblk, hw) x 5]}``.  Images b < B are
        in0's, B + b in1's.  ``stages``: the names to copy (default all of STAGES); the taps are always copied.
        Raises DsxError before any forward and after ``frames``, which reuses the workspace per chunk."""
        info = _lib.LpipsLayerTable()
        check(lib.dsx_lpips_layers(self._h, C.byref(info)))
        dev = self._table_dev                                          # the device of that forward
        B, nimg = int(info.pairs), int(info.nimg)
        out = {"pairs": B, "stages": {}, "taps": []}
        for s, name in enumerate(STAGES):
            if stages is not None and name not in stages:
                continue
            t = torch.empty((nimg, info.H[s], info.W[s], info.C[s]), dtype=torch.float32, device=dev)
            check(lib.dsx_lpips_copy_workspace(self._h, info.stage[s], t.numel() * 4, t, None))
            out["stages"][name] = dict(out=t, launch=STAGE_LAUNCH[name])
        for k, name in enumerate(TAP_STAGES):
            p = torch.empty((B, info.nblk[k]), dtype=torch.float64, device=dev)
            check(lib.dsx_lpips_copy_workspace(self._h, info.part[k], p.numel() * 8, p, None))
            out["taps"].append(dict(stage=name, launch=f"k_lpips_dist<{LIN_CHANNELS[k] // 64}>", part=p,
                                    nblk=int(info.nblk[k]), hw=int(info.hw[k])))
        torch.cuda.current_stream(dev).synchronize()
        return out

    @torch.no_grad()
    def frames(self, target, pred, channel, chunk=0):
        """compute_lpips of the notebooks for one channel: ``target`` / ``pred`` (N, H, W, C) fp32 channel-last device
        tensors -> N values (device tensor).  ``chunk``: frames per pass (0 = the library's choice); the values do
        not depend on it."""
        dev = self._device(target, pred)
        if target.shape != pred.shape or target.dim() != 4:
            raise ValueError(f"target and pred must be (N, H, W, C) of one shape, got {tuple(target.shape)} and "
                             f"{tuple(pred.shape)}")
        t = target.to(dev, torch.float32).contiguous()
        p = pred.to(dev, torch.float32).contiguous()
        N, H, W, Cn = t.shape
        out = torch.empty((N,), dtype=torch.float32, device=dev)
        check(lib.dsx_lpips_frames(self._h, t, p, N, H, W, Cn, int(channel), int(chunk), out, None))
        return out
