"""The objective's host side (no GPU): ABI symbols, the seeded host draws against the reference-written fixtures
(tools/gen_objective_golden.py), sample_t's modes, the coefficient vectors handed to dsx_q_sample, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from oracle import cases
from tests.bits import same_bits
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INDI = 20


def _seed(g):
    torch.manual_seed(int(g["seed_torch"]))
    np.random.seed(int(g["seed_numpy"]))


def _sr3():
    from diffsplitting_amd.model.samplers import GaussianSampler
    s = GaussianSampler(None, 32, channels=3, loss_type="l1", conditional=True)
    s.set_new_noise_schedule(cases.SCHEDULES["lin_25"], "cpu")
    return s


def _ddpm():
    from diffsplitting_amd.model.samplers import GaussianSamplerDdpm
    s = GaussianSamplerDdpm(None, 32, channels=1, loss_type="l2", lr_reduction="mean", conditional=True)
    s.set_new_noise_schedule(cases.SCHEDULES["lin_8"], "cpu")
    return s


def _indi(**kw):
    from diffsplitting_amd.model.samplers import InDISampler
    s = InDISampler(None, 32, channels=2, loss_type="l1", out_channel=2, conditional=False,
                    val_schedule_opt={"n_timestep": N_INDI}, **kw)
    s.set_new_noise_schedule({"n_timestep": N_INDI}, "cpu")
    return s


def _joint(full):
    from diffsplitting_amd.model.samplers import JointIndiSampler
    s = JointIndiSampler(None, 32, channels=1, loss_type="l1", out_channel=1, denoise_fn_ch1=nn.Identity(),
                         denoise_fn_ch2=nn.Identity(), conditional=False, val_schedule_opt={"n_timestep": N_INDI},
                         allow_full_translation=full)
    s.set_new_noise_schedule({"n_timestep": N_INDI}, "cpu")
    return s


# ----------------------------------------------------------------------------- ABI
def test_objective_symbols_declared_bound_exported():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in ("dsx_q_sample", "dsx_loss_blocks", "dsx_loss"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    assert _lib.lib.dsx_abi_version() == 2 and "#define DSX_ABI_VERSION 2" in header


def test_loss_blocks_depend_on_the_shape_only():
    from diffsplitting_amd._lib import lib
    assert lib.dsx_loss_blocks(3, 5, 7) == 1                 # 105 elements: less than one workgroup's chunk
    assert lib.dsx_loss_blocks(3, 64, 67) > 1                # several workgroups per sample
    assert lib.dsx_loss_blocks(3, 64, 67) == lib.dsx_loss_blocks(3, 67, 64)
    assert lib.dsx_loss_blocks(0, 5, 7) < 0 and lib.dsx_loss_blocks(3, -1, 7) < 0


# ----------------------------------------------------------------------------- seeded host draws
def test_seeded_draws_sr3():
    g = load_golden("objective_sr3")
    _seed(g)
    t, c = _sr3()._sample_gamma(2)
    assert t == int(g["t"])
    assert c.dtype == torch.float32 and np.array_equal(c.numpy(), g["continuous_sqrt_alpha_cumprod"])
    # t given: only the uniform draw is made
    np.random.seed(0)
    np.random.uniform(size=2)
    nxt = np.random.uniform()
    np.random.seed(0)
    assert _sr3()._sample_gamma(2, t=3)[0] == 3
    assert np.random.uniform() == nxt


def test_seeded_draws_ddpm():
    g = load_golden("objective_ddpm")
    _seed(g)
    t = _ddpm()._sample_t(3)
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), g["t"])


def test_seeded_draws_indi():
    g = load_golden("objective_indi")
    _seed(g)
    t = _indi().sample_t(3, "cpu")
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), g["t"])


@pytest.mark.parametrize("tag,full", [("custom", False), ("full", True)])
def test_seeded_draws_joint(tag, full):
    """indi1's draws come before indi2's; between them the reference draws indi1's noise (randn_like) from the same
    generator."""
    g = load_golden("objective_joint")
    j = _joint(full)
    assert type(j.indi1).__name__ == ("IndiFullTranslation" if full else "IndiCustomT")
    assert type(j.indi2) is type(j.indi1)
    _seed(g)
    t1 = j.indi1.sample_t(2, "cpu")
    noise1 = torch.randn(2, 1, 32, 32)
    t2 = j.indi2.sample_t(2, "cpu")
    assert np.array_equal(t1.numpy(), g[f"{tag}_t1"]) and np.array_equal(t2.numpy(), g[f"{tag}_t2"])
    assert np.array_equal(noise1.numpy(), g[f"{tag}_noise1"])


# ----------------------------------------------------------------------------- sample_t modes
@pytest.mark.parametrize("mode,lo,hi", [
    ("uniform", 1, N_INDI),                                  # randint(1, n + 1)
    ("uniform_in_range", (2 * N_INDI) // 3, N_INDI),         # randint(2n // 3, n + 1)
    ("linear_ramp", 1, N_INDI - 1),                          # multinomial over arange(n): P(0) = 0
    ("quadratic_ramp", 1, N_INDI - 1),
])
def test_sample_t_modes(mode, lo, hi):
    s = _indi()
    s._t_sampling_mode = mode
    torch.manual_seed(11)
    t = s.sample_t(10000, "cpu")
    assert t.shape == (10000,) and t.dtype == torch.float32
    k = torch.round(t * N_INDI)
    assert torch.equal(t, k / N_INDI)                        # multiples of 1 / n
    assert int(k.min()) >= lo and int(k.max()) <= hi
    assert int(k.max()) == hi and len(torch.unique(k)) > (hi - lo) // 2
    if mode.endswith("ramp"):                                # the ramp: late times are drawn more often than early ones
        assert (k > (lo + hi) / 2).sum() > (k < (lo + hi) / 2).sum()


def test_sample_t_linear_indi_default_and_attributes():
    s = _indi()
    assert s._t_sampling_mode == "linear_indi" and s._linear_indi_a == 1.0
    torch.manual_seed(3)
    k = torch.round(s.sample_t(10000, "cpu") * N_INDI)
    assert int(k.min()) >= 1 and int(k.max()) == N_INDI
    assert 0.4 < float((k == N_INDI).float().mean()) < 0.6   # half of the mass at t = 1 (a = 1)
    j = _joint(False)
    torch.manual_seed(3)
    k = torch.round(j.indi1.sample_t(10000, "cpu") * N_INDI)
    assert int(k.min()) >= 1 and int(k.max()) == N_INDI // 2
    j = _joint(True)
    torch.manual_seed(3)
    k = torch.round(j.indi1.sample_t(10000, "cpu") * N_INDI)
    assert int(k.min()) >= 1 and int(k.max()) == N_INDI - 1
    assert 0.4 < float((k == N_INDI // 2).float().mean()) < 0.6


# ----------------------------------------------------------------------------- coefficient vectors
def test_coefficients_sr3_bitwise_and_reproduce_x_noisy():
    g = load_golden("objective_sr3")
    c = torch.from_numpy(g["continuous_sqrt_alpha_cumprod"])
    c0, c2 = _sr3().q_coefficients(c)
    cv = c.view(-1, 1, 1, 1)
    assert same_bits(c0, cv.reshape(-1))
    assert same_bits(c2, (1 - cv ** 2).sqrt().reshape(-1))
    x = c0.view(-1, 1, 1, 1) * torch.from_numpy(g["target"]) + c2.view(-1, 1, 1, 1) * torch.from_numpy(g["noise"])
    assert same_bits(x, torch.from_numpy(g["x_noisy"]))


def test_coefficients_ddpm_bitwise_and_reproduce_x_noisy():
    g = load_golden("objective_ddpm")
    s = _ddpm()
    t = torch.from_numpy(g["t"])
    c0, c2 = s.q_coefficients(t)
    assert same_bits(c0, s.sqrt_alphas_cumprod.gather(-1, t))
    assert same_bits(c2, s.sqrt_one_minus_alphas_cumprod.gather(-1, t))
    x = c0.view(-1, 1, 1, 1) * torch.from_numpy(g["target"]) + c2.view(-1, 1, 1, 1) * torch.from_numpy(g["noise"])
    assert same_bits(x, torch.from_numpy(g["x_noisy"]))
    # the plain gathers of the forward process
    mean, var, logvar = s.q_mean_variance(torch.from_numpy(g["target"]), t)
    assert torch.equal(mean, c0.view(-1, 1, 1, 1) * torch.from_numpy(g["target"]))
    assert torch.equal(var.reshape(-1), (1. - s.alphas_cumprod).gather(-1, t)) and logvar.shape == (3, 1, 1, 1)
    x0 = s.predict_start_from_noise(x, t, torch.from_numpy(g["noise"]))
    assert float((x0 - torch.from_numpy(g["target"])).abs().max()) < 1e-4
    pm, pv, plv = s.q_posterior(torch.from_numpy(g["target"]), x, t)
    assert pm.shape == x.shape and torch.equal(pv.reshape(-1), s.posterior_variance.gather(-1, t))
    assert torch.equal(plv.reshape(-1), s.posterior_log_variance_clipped.gather(-1, t))


def test_coefficients_indi_bitwise_and_reproduce_x_noisy():
    g = load_golden("objective_indi")
    s = _indi()
    t = torch.from_numpy(g["t"])
    c0, c1, c2 = s.q_coefficients(t)
    tv = t.reshape(-1, 1, 1, 1)
    assert same_bits(c0, (1 - tv).reshape(-1)) and same_bits(c1, t)
    assert same_bits(c2, (s.e * tv).reshape(-1))
    assert s.get_e(t) == s.e
    v = lambda c: c.view(-1, 1, 1, 1)
    x_end = torch.cat([torch.from_numpy(g["input"])] * 2, dim=1)
    x = v(c0) * torch.from_numpy(g["target"]) + v(c1) * x_end + torch.from_numpy(g["noise"]) * v(c2)
    assert same_bits(x, torch.from_numpy(g["x_noisy"]))


# ----------------------------------------------------------------------------- refusals
def test_refuses_unknown_loss_type_by_name():
    from diffsplitting_amd.model.samplers import GaussianSampler, GaussianSamplerDdpm, InDISampler
    for cls in (GaussianSampler, GaussianSamplerDdpm, InDISampler):
        s = cls(None, 32, loss_type="huber", conditional=False, val_schedule_opt={"n_timestep": 4})
        with pytest.raises(NotImplementedError, match="huber"):
            s.set_loss("cpu")
    for lt in ("l1", "l2"):
        s = GaussianSampler(None, 32, loss_type=lt)
        s.set_loss("cpu")
        assert s._reduction == "sum"                          # sr3: always 'sum'
    s = GaussianSamplerDdpm(None, 32, lr_reduction="mean")
    s.set_loss("cpu")
    assert s._reduction == "mean"
    s = InDISampler(None, 32, val_schedule_opt={"n_timestep": 4})
    s.set_loss("cpu")
    assert s._reduction == "sum"                              # lr_reduction None -> 'sum'


def test_refuses_brownian_by_name():
    s = _indi()
    s._noise_mode = "brownian"
    with pytest.raises(NotImplementedError, match="brownian"):
        s.get_t_times_e(torch.tensor([0.5]))
    with pytest.raises(NotImplementedError, match="brownian"):
        s.get_e(torch.tensor([0.5]))


def test_refuses_cpu_tensors():
    from diffsplitting_amd._lib import DsxError
    x, y = torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8)
    t = torch.tensor([0.5, 1.0])
    for s in (_sr3(), _ddpm(), _indi(), _joint(False)):
        s.set_loss("cpu")
        with pytest.raises(DsxError, match="no CPU fallback"):
            s({"target": x, "input": y})
    with pytest.raises(DsxError, match="no CPU fallback"):
        _sr3().q_sample(x, t)
    with pytest.raises(DsxError, match="no CPU fallback"):
        _ddpm().q_sample(x, torch.tensor([1, 2]))
    with pytest.raises(DsxError, match="no CPU fallback"):
        _indi().q_sample(x, y, t)
    with pytest.raises(DsxError, match="no CPU fallback"):
        _indi().get_prediction_during_training({"target": x, "input": y})


def test_q_sample_range_asserts_and_abi_refusals():
    from diffsplitting_amd._lib import lib
    s = _indi()
    x, y = torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8)
    with pytest.raises(AssertionError):
        s.q_sample(x, y, torch.tensor([0.0, 0.5]))
    with pytest.raises(AssertionError):
        s.q_sample(x, y, torch.tensor([0.5, 1.5]))
    fake, null = C.c_void_p(4096), C.c_void_p(0)
    err = lambda: lib.dsx_last_error().decode()

    def call(x0=fake, xe=fake, B=2, Cn=4, Ce=2, H=8, W=8, c0=fake, c1=fake, c2=fake, dst=fake, Cdst=4, coff=0):
        return lib.dsx_q_sample(x0, xe, B, Cn, Ce, H, W, c0, c1, c2, fake, 0, 0, null, dst, Cdst, coff, None)

    assert call(Cn=3, Ce=2, Cdst=3) < 0 and "C % Ce" in err()
    assert call(Cdst=5, coff=2) < 0 and "coff + C > Cdst" in err()
    assert call(coff=-1) < 0
    assert call(x0=null) < 0 and "null" in err()
    assert call(dst=null) < 0 and call(c0=null) < 0 and call(c2=null) < 0
    assert call(c1=null) < 0                                   # three terms need c1
    assert call(B=0) < 0 and call(H=0) < 0
    assert lib.dsx_loss(null, fake, 2, 3, 8, 8, 0, fake, fake, None) < 0 and "null" in err()
    assert lib.dsx_loss(fake, fake, 0, 3, 8, 8, 0, fake, fake, None) < 0
    assert lib.dsx_loss(fake, fake, 2, 0, 8, 8, 1, fake, fake, None) < 0


def test_optimize_parameters_still_raises_and_eval_loss_exists():
    from diffsplitting_amd.model.model import DDPM
    assert callable(DDPM.eval_loss)
    with pytest.raises(NotImplementedError):
        DDPM.optimize_parameters(object())
