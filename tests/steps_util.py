"""Helpers of the single-step and solver tests on the MI355X: a recording noise source, misaligned device operands, and
the UNet that returns a constant."""
import torch

from tests import nets

BIAS = (0.3, -0.45)


def off(t):
    """The same values on the device, 4 bytes past a 16-byte boundary."""
    o = torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()[1:].view(t.shape)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


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
