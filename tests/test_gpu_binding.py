"""The Python binding (diffsplitting_amd/_lib.py) on the device: a call with tensors and a None stream computes what
the same call with raw addresses and the explicit stream computes, a non-default current stream is the one the wrappers
launch on, and tensors on another device than the current one take the call there."""
import ctypes as C

import pytest
import torch

from diffsplitting_amd import _lib, engine
from diffsplitting_amd._lib import Dev, DsxError, Handle, Host, Stream, check, lib
from diffsplitting_amd.data.tiling import TilePlan
from tests.bits import same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _addr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _current():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_randn_tensors_against_raw_pointers():
    n = 1027                                            # no multiple of 4: the tail of the last Philox block
    a = torch.full((n,), -7.25, device="cuda")
    b = a.clone()
    assert check(lib.dsx_randn(a, n, 11, 5, None)) == 0
    assert check(lib.dsx_randn(_addr(b), n, 11, 5, _current())) == 0
    torch.cuda.synchronize()
    assert same_bits(a, b) and not bool((a == -7.25).any())


@pytest.mark.parametrize("injected", [True, False])
def test_q_sample_tensors_against_raw_pointers(injected):
    B, Cn, H, W = 2, 3, 5, 7                            # H * W is no multiple of 4: the scalar path
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn((B, Cn, H, W), generator=g).cuda()
    c0, c2 = torch.rand(B, generator=g).cuda(), torch.rand(B, generator=g).cuda()
    z = torch.randn((B, Cn, H, W), generator=g).cuda() if injected else None
    outs = []
    for raw in (False, True):
        p = _addr if raw else (lambda t: t)
        dst = torch.full((B, Cn, H, W), -7.25, device="cuda")
        z_out = None if injected else torch.full((B, Cn, H, W), -7.25, device="cuda")
        assert check(lib.dsx_q_sample(p(x0), None, B, Cn, 1, H, W, p(c0), None, p(c2), p(z), 21, 4, p(z_out), p(dst), Cn, 0,
                                      _current() if raw else None)) == 0
        outs.append((dst, z_out))
    torch.cuda.synchronize()
    assert same_bits(outs[0][0], outs[1][0]) and not bool((outs[0][0] == -7.25).any())
    if not injected:
        assert same_bits(outs[0][1], outs[1][1]) and not bool((outs[0][1] == -7.25).any())


def test_wrappers_launch_on_a_non_default_current_stream():
    plan = TilePlan((2, 16, 16), (1, 4, 4), (1, 8, 8))
    frames = torch.randn((2, 16, 16), generator=torch.Generator().manual_seed(5)).cuda()
    ref = plan.stitch(plan.gather(frames)[:, None].contiguous())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = plan.stitch(plan.gather(frames)[:, None].contiguous())
    s.synchronize()
    assert got.shape == (2, 16, 16, 1) and same_bits(got, ref)


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *args):
        self.calls.append((args, torch.cuda.current_device()))
        return 0


def test_call_path_with_device_tensors():
    """Against a recording stand-in: what a CUDA tensor must be, and what the stand-in is handed for one."""
    rec = Recorder()
    f = _lib.bind("dsx_fake", rec, [Handle, Dev("float"), C.c_int, Host, Dev("void"), Stream])
    x = torch.zeros((4, 4), device="cuda")
    for bad, word in ((x.t(), "strided"), (x.double(), "float64")):
        with pytest.raises(DsxError, match=rf"dsx_fake: argument 1 .*{word}"):
            f(None, bad, 3, None, None, None)
    with pytest.raises(DsxError, match="dsx_fake: argument 4 .*strided"):
        f(None, x, 3, None, x.t(), None)
    with pytest.raises(DsxError, match="dsx_fake: argument 3 takes host memory"):
        f(None, None, 3, x, None, None)
    assert rec.calls == []
    s = torch.cuda.Stream()
    half = x.half()
    with torch.cuda.stream(s):
        f(None, x, 3, None, half, None)                         # None: the current stream of the tensors' device
    f(None, x[2:], 3, None, None, s)                            # a torch stream as it is; a slice is its own address
    f(None, x, 3, None, None, 0x40)
    (a0, d0), (a1, _), (a2, _) = rec.calls
    assert a0 == (None, x.data_ptr(), 3, None, half.data_ptr(), s.cuda_stream) and d0 == x.device.index
    assert a1 == (None, x.data_ptr() + 32, 3, None, None, s.cuda_stream) and a2[5] == 0x40


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_tensors_on_another_device_than_the_current_one():
    assert torch.cuda.current_device() == 0
    ids, shape = [5, 9], (2, 3, 5, 7)
    outs = {}
    for dev in ("cuda:0", "cuda:1"):
        z = engine.randn_samples(shape, 17, ids, draw=2, device=dev)
        x0 = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dev)
        c = torch.tensor([0.25, 0.5], device=dev)
        q, _ = engine.q_sample(x0, c, 1 - c, z=z)
        torch.cuda.synchronize(dev)
        assert z.device == q.device == torch.device(dev)
        outs[dev] = (z, q)
    assert torch.cuda.current_device() == 0
    assert same_bits(outs["cuda:0"][0], outs["cuda:1"][0]) and same_bits(outs["cuda:0"][1], outs["cuda:1"][1])
    with pytest.raises(DsxError, match="dsx_q_sample: tensors on cuda:1 and on cuda:0"):
        lib.dsx_q_sample(outs["cuda:1"][1], None, 2, 3, 1, 5, 7, outs["cuda:0"][0][:, 0, 0, 0].contiguous(), None,
                         outs["cuda:0"][0][:, 0, 0, 1].contiguous(), None, 0, 0, None, outs["cuda:1"][0], 3, 0, None)
