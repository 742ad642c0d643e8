"""Few-step sampling for the Gaussian models: the coefficient rows of DDIM(eta) and DPM-Solver++(2M, data prediction)
over a sub-sequence of the trained schedule (host arithmetic; the device evaluates the rows: ``dsx_solver_loop`` /
``dsx_solver_step``, include/dsx.h).

Notation: ``ac[t]`` the float64 cumulative product of ``1 - betas`` (as ``engine.gaussian_buffers`` forms it),
``alpha = sqrt(ac)``, ``sigma = sqrt(1 - ac)``, ``lam = log(alpha / sigma)``.  A run is a strictly descending list of
timesteps ``tau_0 > ... > tau_{K-1} >= 0``; row ``k`` moves the state from ``s = tau_k`` to ``n = tau_{k+1}``, the last
row to the clean image (``ac_n = 1``).  Every row holds ``SOLVER_COLUMNS``; the update is

    x0  = clamp?(a*x - b*net)
    x  <- c0*x0 + cx*x (+ cp*x0_prev where cp != 0) (+ sigma*z where a draw is taken)

``tcond, a, b`` are the very fp32 numbers ``engine.gaussian_step_columns`` holds at ``t = tau_k``, so ``x0`` is
``p_mean_variance``'s ``x_recon`` bit for bit.  The other columns are computed in float64 and rounded to fp32 once:

    ddim     sigma = eta * sqrt((1 - ac_n) / (1 - ac_s)) * sqrt(1 - ac_s / ac_n)
             cx = sqrt(1 - ac_n - sigma^2) / sigma_s,  c0 = alpha_n - cx * alpha_s,  cp = 0
    dpmpp2m  h = lam_n - lam_s,  cx = sigma_n / sigma_s,  g = -alpha_n * expm1(-h),  sigma = 0
             first row: c0 = g, cp = 0;  then, with r = h_prev / h: c0 = g * (1 + 1 / (2 r)), cp = -g / (2 r)
             last row: the ddim row with eta = 0 (cx = 0, c0 = 1, cp = 0): the result is the last predicted x0

``cp`` of row 0 and ``sigma`` of the last row are 0 for every solver: no x0 precedes the first step, and no draw is
taken at the last one, as SR3 takes none at t = 0.
"""
import ctypes as C

import numpy as np

from .. import _lib, engine
from .._lib import DsxError

SOLVERS = ("ddim", "dpmpp2m")
SPACINGS = ("uniform", "logsnr")
SOLVER_COLUMNS = ("tcond", "a", "b", "cx", "c0", "cp", "sigma")


def alphas_cumprod_f64(schedule_opt):
    """The float64 cumulative product ``engine.gaussian_buffers`` rounds to its fp32 ``alphas_cumprod`` buffer."""
    betas = engine.make_beta_schedule(schedule_opt["schedule"], schedule_opt["n_timestep"], schedule_opt["linear_start"],
                                      schedule_opt["linear_end"])
    return np.cumprod(1.0 - betas, axis=0)


def log_snr(alphas_cumprod):
    """``lam[t] = log(alpha / sigma)`` in float64 (strictly decreasing in t for betas in (0, 1))."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    return 0.5 * (np.log(ac) - np.log1p(-ac))


def default_spacing(solver):
    return "logsnr" if solver == "dpmpp2m" else "uniform"


def solver_timesteps(alphas_cumprod, steps, spacing="uniform"):
    """At most ``steps`` timesteps of 0 .. T-1, descending, ``T - 1`` and ``0`` always among them.

    "uniform": ``unique(rint(linspace(0, T - 1, steps)))``.  "logsnr": ``steps`` values of ``lam`` evenly spaced between
    ``lam[T - 1]`` and ``lam[0]``, each mapped to the timestep with the nearest ``lam`` (the lowest index on a tie),
    duplicates removed."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    T = int(ac.shape[0])
    steps = int(steps)
    if steps < 2 and T > 1:
        raise DsxError(f"steps must be at least 2 (a spacing holds both T - 1 and 0), got {steps}")
    if steps < 1:
        raise DsxError(f"steps must be at least 1, got {steps}")
    if spacing == "uniform":
        ts = np.rint(np.linspace(0, T - 1, steps)).astype(np.int64)
    elif spacing == "logsnr":
        lam = log_snr(ac)
        want = np.linspace(lam[T - 1], lam[0], steps)
        ts = np.abs(lam[None, :] - want[:, None]).argmin(axis=1).astype(np.int64)     # argmin: the first, lowest index
        ts[0], ts[-1] = T - 1, 0                                                      # the end points are exact values
    else:
        raise DsxError(f"spacing must be one of {SPACINGS}, got {spacing!r}")
    return [int(t) for t in np.unique(ts)[::-1]]


def check_timesteps(timesteps, T):
    """``timesteps`` as a list of ints, refused by name when empty, out of 0 .. T-1 or not strictly descending."""
    ts = [int(t) for t in timesteps]
    if not ts:
        raise DsxError("timesteps is empty: a run needs at least one timestep")
    if min(ts) < 0 or max(ts) >= T:
        raise DsxError(f"timesteps must lie in 0..{T - 1}, got {min(ts)}..{max(ts)}")
    if any(b >= a for a, b in zip(ts, ts[1:])):
        raise DsxError("timesteps must be strictly descending")
    return ts


def check_solver(solver, eta):
    if solver not in SOLVERS:
        raise DsxError(f"solver must be one of {SOLVERS}, got {solver!r}")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise DsxError(f"eta must lie in [0, 1], got {eta}")
    if solver == "dpmpp2m" and eta != 0.0:
        raise DsxError("eta != 0 with dpmpp2m: the multistep solver is deterministic (eta belongs to ddim)")
    return eta


def solver_rows_f64(alphas_cumprod, timesteps, solver, eta=0.0):
    """The float64 columns ``cx, c0, cp, sigma`` of the run ``timesteps`` (before the fp32 cast): a dict of (K,) arrays."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    ts = check_timesteps(timesteps, int(ac.shape[0]))
    eta = check_solver(solver, eta)
    K = len(ts)
    ac_s = ac[ts]
    ac_n = np.append(ac_s[1:], 1.0)                                  # the last row's target is the clean image
    al_s, al_n = np.sqrt(ac_s), np.sqrt(ac_n)
    sg_s, sg_n = np.sqrt(1.0 - ac_s), np.sqrt(1.0 - ac_n)
    # ddim rows; dpmpp2m keeps the last of them
    sigma = eta * np.sqrt((1.0 - ac_n) / (1.0 - ac_s)) * np.sqrt(np.maximum(1.0 - ac_s / ac_n, 0.0))
    sigma[-1] = 0.0
    cx = np.sqrt(np.maximum(1.0 - ac_n - sigma ** 2, 0.0)) / sg_s
    c0 = al_n - cx * al_s
    cp = np.zeros(K)
    if solver == "dpmpp2m" and K > 1:
        lam = log_snr(ac)
        h = lam[ts[1:]] - lam[ts[:-1]]                               # K - 1 steps between timesteps, all > 0
        g = -al_n[:-1] * np.expm1(-h)
        cx[:-1] = sg_n[:-1] / sg_s[:-1]
        c0[:-1] = g
        r = h[:-1] / h[1:]                                           # h_prev / h for rows 1 .. K-2
        c0[1:-1] = g[1:] * (1.0 + 1.0 / (2.0 * r))
        cp[1:-1] = -g[1:] / (2.0 * r)
        sigma[:] = 0.0
    return dict(cx=cx, c0=c0, cp=cp, sigma=sigma)


class SolverTableHost:
    """Host-side rows handed to ``dsx_solver_loop`` (include/dsx.h): fp32 columns ``SOLVER_COLUMNS`` of (K,) values,
    ``timesteps`` the run they belong to (None when built from bare columns)."""

    def __init__(self, tcond, a, b, cx, c0, cp, sigma, clip=True, timesteps=None):
        f = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
        self.tcond, self.a, self.b, self.cx, self.c0, self.cp, self.sigma = (f(v) for v in (tcond, a, b, cx, c0, cp, sigma))
        self.n_steps = int(self.tcond.shape[0])
        for k in SOLVER_COLUMNS:
            if getattr(self, k).shape[0] != self.n_steps:
                raise DsxError(f"solver table column {k} holds {getattr(self, k).shape[0]} values, tcond {self.n_steps}")
        if self.n_steps < 1:
            raise DsxError("a solver table needs at least one row")
        self.clip = bool(clip)
        self.timesteps = None if timesteps is None else [int(t) for t in timesteps]

    def c_struct(self):
        p = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
        return _lib.SolverTable(self.n_steps, int(self.clip), *(p(getattr(self, k)) for k in SOLVER_COLUMNS))

    def columns(self):
        return {k: getattr(self, k) for k in SOLVER_COLUMNS}

    def step_table(self):
        """The same rows as a ``StepTableHost`` (c1 = c0, c2 = cx) for ``dsx_sample_loop``: only without a history term."""
        if np.any(self.cp != 0):
            raise DsxError("rows with cp != 0 need the x0 history: they have no ancestral step table")
        return engine.StepTableHost(self.tcond, c1=self.c0, c2=self.cx, sigma=self.sigma, a=self.a, b=self.b,
                                    predict_eps=True, clip=self.clip)


def solver_table(bufs, gamma_table_f64, kind, alphas_cumprod, solver="dpmpp2m", steps=None, eta=0.0, spacing=None,
                 timesteps=None, clip_denoised=True):
    """The rows of ``solver`` for a Gaussian sampler's schedule (``bufs, gamma_table_f64`` of ``engine.gaussian_buffers``,
    ``kind`` "sr3" / "ddpm", ``alphas_cumprod`` float64).  The run is ``timesteps`` when given, else
    ``solver_timesteps(alphas_cumprod, steps, spacing)`` with the solver's default spacing (logsnr for dpmpp2m, uniform
    for ddim)."""
    eta = check_solver(solver, eta)
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    T = int(ac.shape[0])
    if T != int(bufs["betas"].shape[0]):
        raise DsxError(f"alphas_cumprod holds {T} timesteps, the schedule {int(bufs['betas'].shape[0])}")
    if timesteps is not None:
        if steps is not None or spacing is not None:
            raise DsxError("timesteps= together with steps= / spacing=: the run is given or spaced, not both")
        ts = check_timesteps(timesteps, T)
    else:
        if steps is None:
            raise DsxError("a solver table needs steps= or timesteps=")
        ts = solver_timesteps(ac, steps, default_spacing(solver) if spacing is None else spacing)
    head = engine.gaussian_step_rows(bufs, gamma_table_f64, kind, np.asarray(ts, dtype=np.int64))
    rows = solver_rows_f64(ac, ts, solver, eta)
    return SolverTableHost(head["tcond"], head["a"], head["b"], rows["cx"], rows["c0"], rows["cp"], rows["sigma"],
                           clip=clip_denoised, timesteps=ts)
