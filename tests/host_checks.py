"""Helpers of the tests that drive the library's host-side checks without a GPU: fake device pointers, the last error's
text, small tile plans, and samplers that never reach a network."""
import ctypes as C

ERR_INVALID = -1
FAKE = C.c_void_p(4096)                                               # non-NULL, never dereferenced
# (frames, patch, grid): ragged extents with a shifted last row / column, up to 12 contributors, a single tile
BLEND_PLANS = [((1, 40, 56), 32, 16), ((1, 37, 50), 24, 8), ((1, 64, 96), 32, 16), ((1, 33, 33), 32, 16), ((1, 45, 70), 30, 10),
               ((1, 32, 32), 32, 32)]


def binding():
    from diffsplitting_amd import _lib
    return _lib


def last_error():
    return binding().lib.dsx_last_error().decode()


def tile_plan(shape, patch, grid):
    from diffsplitting_amd.data.tiling import TilePlan
    return TilePlan(shape, (1, grid, grid), (1, patch, patch))


def cpu_samplers():
    """A Gaussian, an InDI and a JointIndi sampler on the CPU, with schedules and without networks."""
    import torch
    from diffsplitting_amd.model.samplers import GaussianSampler, InDISampler, JointIndiSampler
    sched = {"schedule": "linear", "n_timestep": 12, "linear_start": 1e-4, "linear_end": 2e-2}
    g = GaussianSampler(None, 32, channels=2, conditional=True)
    g.set_new_noise_schedule(sched, "cpu")
    i = InDISampler(None, 32, channels=1, out_channel=2, conditional=False)
    i.set_new_noise_schedule({"n_timestep": 3}, "cpu")
    j = JointIndiSampler(None, 32, channels=1, out_channel=1, conditional=False, denoise_fn_ch1=torch.nn.Identity(),
                         denoise_fn_ch2=torch.nn.Identity())
    j.set_new_noise_schedule({"n_timestep": 4}, "cpu")
    return g, i, j
