"""Helpers of the single-step, objective and solver tests on the MI355X: the torch fp32 expressions of q_sample, one reverse
step and the start of interpolate, a recording noise source, misaligned device operands, and the UNet that returns a
constant."""
import torch

from tests import nets

BIAS = (0.3, -0.45)


def off(t):
    """The same values on the device, 4 bytes past a 16-byte boundary."""
    o = torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()[1:].view(t.shape)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


def ref_q(x0, c0, c2, z, xe=None, c1=None):
    """The reference's q_sample on the CPU in fp32: separately rounded products and sums, left to right."""
    v = lambda c: c.view(-1, 1, 1, 1)
    out = v(c0) * x0
    if xe is not None:
        out = out + v(c1) * torch.cat([xe] * (x0.shape[1] // xe.shape[1]), dim=1)
    return out + v(c2) * z


def ref_step(x, net, co, z, predict_eps, clip, repeat=False):
    """dsx_posterior_step in torch fp32 on the CPU: separately rounded products and sums."""
    v = lambda k: co[k].view(-1, 1, 1, 1)
    x0 = net
    if predict_eps:
        x0 = v("a") * x - v("b") * net
        if clip:
            x0 = x0.clamp(-1.0, 1.0)
    mean = v("c1") * x0 + v("c2") * x
    if repeat:
        z = z.repeat(x.shape[0], 1, 1, 1)
    return x0, mean, torch.where(v("sigma") != 0, mean + z * v("sigma"), mean)


def ref_interp(x1, x2, a0, s0, lam, z1, z2):
    """dsx_interp_start in torch fp32 on the CPU (ddpm diffusion.py:249-259): the two q_sample results and their lerp,
    1 - lam formed in double and each scalar rounded to fp32 once, as torch does for a python scalar."""
    v = lambda c: c.view(-1, 1, 1, 1)
    xt1, xt2 = v(a0) * x1 + v(s0) * z1, v(a0) * x2 + v(s0) * z2
    return (1 - lam) * xt1 + lam * xt2


class Source:
    """A noise_source that hands out the given draws in order and records the shapes asked for."""

    def __init__(self, draws=()):
        self.draws, self.shapes = list(draws), []

    def __call__(self, shape):
        self.shapes.append(tuple(shape))
        return self.draws.pop(0) if self.draws else torch.zeros(shape)


def constant_unet(net, B):
    """With the final conv's weights zero the UNet returns its bias, BIAS, in every executor."""
    net.final_conv__block__3__weight.zero_()
    net.final_conv__block__3__bias.copy_(torch.tensor(BIAS))
    out = net(nets.rand((B, 2, 16, 16), 50).cuda(), torch.full((B,), 0.5).cuda())
    assert torch.equal(out.cpu(), torch.tensor(BIAS).view(1, 2, 1, 1).expand(B, 2, 16, 16))
