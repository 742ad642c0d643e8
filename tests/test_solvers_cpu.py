"""Few-step solvers, host side (no GPU): the coefficient tables of model/solvers.py against the posterior columns and
against a closed-form probability-flow solution, timestep spacing, refusals by name, and the two entry points as
declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import solver_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsx_solver_loop", "dsx_solver_step")
SCHED = dict(schedule="linear", n_timestep=20, linear_start=1e-4, linear_end=1e-1)


def _solvers():
    from diffsplitting_amd.model import solvers
    return solvers


# ----------------------------------------------------------------------------- ddim(eta = 1) is the ancestral posterior
def test_ddim_eta1_over_every_timestep_is_the_posterior():
    S = _solvers()
    T = 100
    betas = np.linspace(1e-3, 0.15, T, dtype=np.float64)
    ac = np.cumprod(1.0 - betas)
    ac_prev = np.append(1.0, ac[:-1])
    coef1 = betas * np.sqrt(ac_prev) / (1.0 - ac)                      # posterior_mean_coef1: the weight of x0
    coef2 = (1.0 - ac_prev) * np.sqrt(1.0 - betas) / (1.0 - ac)        # posterior_mean_coef2: the weight of x_t
    var = betas * (1.0 - ac_prev) / (1.0 - ac)
    rows = S.solver_rows_f64(ac, range(T - 1, -1, -1), "ddim", eta=1.0)
    order = np.arange(T - 1, -1, -1)
    dev = {"c0": np.abs(rows["c0"] - coef1[order]).max(), "cx": np.abs(rows["cx"] - coef2[order]).max(),
           "sigma^2": np.abs(rows["sigma"][:-1] ** 2 - var[order][:-1]).max()}
    print("\nddim(eta=1) vs posterior columns, max deviation:", dev)
    assert all(v <= 1e-12 for v in dev.values()), dev
    # no draw at the last row (t = 0), whatever the posterior variance says there
    assert rows["sigma"][-1] == 0 and np.all(rows["cp"] == 0)


# ----------------------------------------------------------------------------- convergence on Gaussian data
S2 = 0.25                                                            # the data are N(0, 0.25)


def _gaussian_error(solver, K):
    """|state after row K-2 - exact probability-flow state at tau = 0| for x_T = 1, float64, logsnr spacing."""
    S = _solvers()
    T = 1000
    ac = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, T, dtype=np.float64))
    ts = S.solver_timesteps(ac, K, "logsnr")
    assert K - 1 <= len(ts) <= K and ts[0] == T - 1 and ts[-1] == 0    # near t = 0 two targets can share a timestep
    K = len(ts)
    rows = S.solver_rows_f64(ac, ts, solver)
    al, sg = np.sqrt(ac[ts]), np.sqrt(1.0 - ac[ts])
    rows.update(a=1.0 / al, b=sg / al)                                # x0 = (x - sigma eps) / alpha

    def eps(k, x):                                                   # the exact denoiser, as the noise it implies
        x0 = al[k] * S2 / (al[k] ** 2 * S2 + sg[k] ** 2) * x
        return (x - al[k] * x0) / sg[k]

    states, _ = solver_ref.run(rows, np.array([1.0]), eps, dtype=np.float64)
    marg = lambda t: np.sqrt(ac[t] * S2 + 1.0 - ac[t])
    return float(abs(states[K - 2][0] - marg(0) / marg(T - 1)))


def test_convergence_orders_on_gaussian_data():
    err = {(s, K): _gaussian_error(s, K) for s in ("ddim", "dpmpp2m") for K in (10, 20, 40)}
    for K in (10, 20, 40):
        print(f"\nK = {K}: ddim error {err['ddim', K]:.3e}, dpmpp2m error {err['dpmpp2m', K]:.3e}")
    assert 1.8 <= err["ddim", 10] / err["ddim", 20] <= 2.2            # first order
    assert err["dpmpp2m", 20] / err["dpmpp2m", 40] > 3                # second order
    for K in (10, 20, 40):
        assert err["dpmpp2m", K] < err["ddim", K] / 4


# ----------------------------------------------------------------------------- spacing
@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
@pytest.mark.parametrize("T, steps", [(20, 5), (20, 2), (20, 20), (1000, 50), (8, 7), (2, 2)])
def test_spacings_descend_and_keep_both_ends(spacing, T, steps):
    S = _solvers()
    ac = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, T, dtype=np.float64))
    ts = S.solver_timesteps(ac, steps, spacing)
    assert ts[0] == T - 1 and ts[-1] == 0 and len(ts) <= steps
    assert all(a > b for a, b in zip(ts, ts[1:])) and all(isinstance(t, int) for t in ts)


def test_spacing_definitions():
    S = _solvers()
    T = 20
    ac = np.cumprod(1.0 - np.linspace(1e-4, 1e-1, T, dtype=np.float64))
    assert S.solver_timesteps(ac, 5, "uniform") == [19, 14, 10, 5, 0]          # rint(linspace(0, 19, 5)), rint(9.5) = 10
    assert S.solver_timesteps(ac, 50, "uniform") == list(range(T - 1, -1, -1))    # steps > T: duplicates removed, T rows
    lam = np.log(np.sqrt(ac) / np.sqrt(1.0 - ac))
    want = [int(np.abs(lam - v).argmin()) for v in np.linspace(lam[-1], lam[0], 6)]
    assert S.solver_timesteps(ac, 6, "logsnr") == sorted(set(want), reverse=True)
    assert len(S.solver_timesteps(ac, 200, "logsnr")) <= T
    assert S.default_spacing("dpmpp2m") == "logsnr" and S.default_spacing("ddim") == "uniform"


# ----------------------------------------------------------------------------- refusals, by name
def test_refusals_name_the_argument():
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    S = _solvers()
    bufs, gamma = engine.gaussian_buffers(SCHED)
    ac = S.alphas_cumprod_f64(SCHED)
    tab = lambda **kw: S.solver_table(bufs, gamma, "sr3", ac, **kw)
    for ts, word in (([], "empty"), ([5, 5, 1], "strictly descending"), ([3, 7], "strictly descending"),
                     ([20, 3], r"0\.\.19"), ([4, -1], r"0\.\.19")):
        with pytest.raises(DsxError, match=word):
            tab(solver="ddim", timesteps=ts)
    for eta in (-0.1, 1.5):
        with pytest.raises(DsxError, match="eta must lie in"):
            tab(solver="ddim", steps=5, eta=eta)
    with pytest.raises(DsxError, match="eta != 0 with dpmpp2m"):
        tab(solver="dpmpp2m", steps=5, eta=0.5)
    with pytest.raises(DsxError, match="solver must be one of"):
        tab(solver="euler", steps=5)
    with pytest.raises(DsxError, match="spacing must be one of"):
        tab(solver="ddim", steps=5, spacing="karras")
    with pytest.raises(DsxError, match="steps= or timesteps="):
        tab(solver="ddim")
    with pytest.raises(DsxError, match="given or spaced"):
        tab(solver="ddim", steps=5, timesteps=[3, 1])
    with pytest.raises(DsxError, match="steps must be at least 2"):
        tab(solver="ddim", steps=1)
    t = tab(solver="dpmpp2m", steps=5)
    with pytest.raises(DsxError, match="x0 history"):
        t.step_table()


# ----------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("kind", ["sr3", "ddpm"])
@pytest.mark.parametrize("solver, eta", [("ddim", 0.0), ("ddim", 0.7), ("ddim", 1.0), ("dpmpp2m", 0.0)])
@pytest.mark.parametrize("run", [dict(steps=5, spacing="uniform"), dict(steps=5, spacing="logsnr"), dict(steps=5),
                                 dict(steps=2), dict(timesteps=[17, 9, 8, 2]), dict(timesteps=[6])])
def test_rows_of_every_solver_and_spacing(kind, solver, eta, run):
    from diffsplitting_amd import engine
    S = _solvers()
    bufs, gamma = engine.gaussian_buffers(SCHED)
    ac = S.alphas_cumprod_f64(SCHED)
    assert np.array_equal(ac.astype(np.float32), bufs["alphas_cumprod"].numpy())   # the float64 the buffers come from
    t = S.solver_table(bufs, gamma, kind, ac, solver=solver, eta=eta, **run)
    K = t.n_steps
    assert K == len(t.timesteps) and all(getattr(t, k).dtype == np.float32 and getattr(t, k).shape == (K,)
                                         for k in S.SOLVER_COLUMNS)
    assert t.cp[0] == 0 and t.sigma[-1] == 0
    assert (t.cx[-1], t.c0[-1], t.cp[-1]) == (0.0, 1.0, 0.0)          # the last row returns the predicted x0
    head = engine.gaussian_step_rows(bufs, gamma, kind, np.asarray(t.timesteps))
    for k in ("tcond", "a", "b"):
        assert np.array_equal(getattr(t, k), head[k]), k
    if "timesteps" in run:
        assert t.timesteps == run["timesteps"]
    if solver == "dpmpp2m":
        assert np.all(t.sigma == 0) and (K < 3 or np.all(t.cp[1:-1] < 0))          # cp = -g / (2 r), g > 0
        # row by row against the published form: x <- (sigma_n / sigma_s) x - alpha_n expm1(-h) D,
        # D = (1 + 1 / (2 r)) x0 - (1 / (2 r)) x0_prev
        lam = np.log(np.sqrt(ac) / np.sqrt(1.0 - ac))
        ts = t.timesteps
        for k in range(1, K - 1):
            h, hp = lam[ts[k + 1]] - lam[ts[k]], lam[ts[k]] - lam[ts[k - 1]]
            g = -np.sqrt(ac[ts[k + 1]]) * np.expm1(-h)
            # 1 / (2 r) = h / (2 h_prev); a float64 restatement rounds to the same fp32 but for the last bit
            assert np.isclose(t.c0[k], g * (1 + h / (2 * hp)), rtol=1e-6, atol=0), (k, t.c0[k])
            assert np.isclose(t.cp[k], -g * h / (2 * hp), rtol=1e-6, atol=0), (k, t.cp[k])
            assert np.isclose(t.cx[k], np.sqrt((1 - ac[ts[k + 1]]) / (1 - ac[ts[k]])), rtol=1e-6, atol=0)
    else:
        assert np.all(t.cp == 0) and (np.all(t.sigma[:-1] > 0) if eta else np.all(t.sigma == 0))
        st = t.step_table()
        assert np.array_equal(st.c1, t.c0) and np.array_equal(st.c2, t.cx) and st.predict_eps and st.n_steps == K


def test_sampler_keeps_its_parameter_lists():
    import inspect
    from diffsplitting_amd.model import samplers as SM
    from diffsplitting_amd.model.model import DDPM
    p = inspect.signature(SM.GaussianSampler.solver_sample_loop).parameters
    assert list(p) == ["self", "x_in", "steps", "solver", "eta", "spacing", "timesteps", "clip_denoised", "continous",
                       "seed", "sample_ids"]
    assert (p["steps"].default, p["solver"].default, p["eta"].default) == (50, "dpmpp2m", 0.0)
    assert SM.GaussianSamplerDdpm.solver_sample_loop is SM.GaussianSampler.solver_sample_loop
    assert not hasattr(SM.InDISampler, "solver_sample_loop") and not hasattr(SM.JointIndiSampler, "solver_sample_loop")
    assert list(inspect.signature(SM.GaussianSampler.p_sample_loop).parameters) == [
        "self", "x_in", "clip_denoised", "continous", "seed", "sample_ids"]
    assert list(inspect.signature(DDPM.set_solver).parameters) == ["self", "solver", "steps", "eta", "spacing"]
    assert DDPM.solver is None


def test_set_solver_without_a_device():
    import inspect
    from diffsplitting_amd import infer
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.model import samplers as SM
    from diffsplitting_amd.model.model import DDPM
    m = DDPM.__new__(DDPM)
    m.netG = SM.InDISampler(None, 32, channels=2, conditional=False)
    with pytest.raises(DsxError, match="InDISampler is not a Gaussian sampler"):
        m.set_solver("ddim", steps=5)
    m.netG = SM.GaussianSampler(None, 32)
    with pytest.raises(DsxError, match="needs steps="):
        m.set_solver("ddim")
    with pytest.raises(DsxError, match="eta != 0 with dpmpp2m"):
        m.set_solver("dpmpp2m", steps=5, eta=0.3)
    with pytest.raises(DsxError, match="spacing must be one of"):
        m.set_solver("ddim", steps=5, spacing="karras")
    m.set_solver("dpmpp2m", steps=20)
    assert m.solver == dict(solver="dpmpp2m", steps=20, eta=0.0, spacing=None)
    m.set_solver()
    assert m.solver is None
    src = inspect.getsource(infer.main)
    assert all(flag in src for flag in ("--solver", "--solver-steps", "--eta", "--spacing"))
    with pytest.raises(DsxError, match="set_new_noise_schedule"):
        m.netG.solver_sample_loop(None, steps=5)


# ----------------------------------------------------------------------------- the C entry points
def test_solver_symbols_declared_bound_exported():
    from diffsplitting_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib._cdll, name)
    assert "typedef struct dsx_solver_table" in header
    assert [f[0] for f in _lib.SolverTable._fields_] == ["n_steps", "clip", "tcond", "a", "b", "cx", "c0", "cp", "sigma"]
    assert _lib.lib.dsx_abi_version() == 2 and re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", header)
    assert len(_lib.StepTable._fields_) == 10 and len(_lib.SIGNATURES["dsx_sample_loop"][1]) == 11
    assert len(_lib.SIGNATURES["dsx_solver_loop"][1]) == 13 and len(_lib.SIGNATURES["dsx_solver_step"][1]) == 23
    assert "dsx_steps.hip" in open(os.path.join(ROOT, "diffsplitting_amd", "csrc", "build.sh")).read()


ONE = 16                                                             # a non-null address that is never dereferenced


def _refused(rc, word):
    from diffsplitting_amd import _lib
    msg = _lib.lib.dsx_last_error()
    assert rc == -1, (rc, msg)
    assert word in msg, msg


def test_solver_loop_refuses_without_an_executor():
    from diffsplitting_amd import _lib
    tab = _lib.SolverTable()
    _refused(_lib.lib.dsx_solver_loop(None, C.byref(tab), None, ONE, None, 1, None, 0, None, 0, None, None, 0),
             b"null executor")


def test_solver_step_refusals():
    from diffsplitting_amd import _lib
    lib = _lib.lib
    ids = (C.c_uint64 * 2)(5, 9)
    coefs = (ONE,) * 6
    call = lambda x=ONE, prev=None, B=2, co=coefs, z=None, recon=ONE, out=ONE, ids=None, n=0, draw=0: lib.dsx_solver_step(
        x, ONE, prev, B, 1, 2, 2, *co, 0, z, 7, 1, recon, out, None, ids, n, draw)
    _refused(call(B=0), b"solver_step: empty shape")
    _refused(call(x=None), b"solver_step: null argument")
    _refused(call(co=(ONE, ONE, None, ONE, ONE, ONE)), b"solver_step: null argument")
    _refused(call(prev=ONE, co=(ONE, ONE, ONE, ONE, None, ONE)), b"x0_prev without the column cp")
    _refused(call(recon=None), b"solver_step: null output")
    _refused(call(out=None), b"solver_step: null output")
    _refused(call(z=ONE, ids=ids, n=2), b"injected noise together with sample_ids")
    _refused(call(ids=ids, n=3), b"sample ids for a batch of 2")
    _refused(call(ids=(C.c_uint64 * 2)(5, 1 << 40), n=2), b"sample id")
    _refused(call(ids=ids, n=2, draw=1 << 24), b"draw ordinal")
