"""Reference for the few-step solver update (include/dsx.h, dsx_solver_loop / dsx_solver_step): the row recurrence
restated in numpy, one rounded operation at a time, in fp32 (what the device must reproduce bit for bit) and in
float64 (for the convergence check of the coefficient tables).

    x0  = clamp?(a*x - b*net)
    m   = c0*x0 + cx*x
    m   = cp != 0 ? m + cp*x0_prev : m
    out = sigma != 0 ? m + z*sigma : m

A coefficient is a scalar or an array that broadcasts against x, e.g. (B, 1, 1, 1) for per-sample values."""
import numpy as np

COLUMNS = ("a", "b", "cx", "c0", "cp", "sigma")


def step(row, x, net, x0_prev=None, z=None, clip=False, dtype=np.float32):
    """One update.  ``row``: dict of COLUMNS.  Returns (x0, out) in ``dtype``; every product and sum is one numpy
    operation on ``dtype`` operands, so each is rounded on its own."""
    c = {k: np.asarray(row[k], dtype=dtype) for k in COLUMNS}
    x, net = np.asarray(x, dtype=dtype), np.asarray(net, dtype=dtype)
    x0 = c["a"] * x - c["b"] * net
    if clip:
        x0 = np.clip(x0, dtype(-1), dtype(1))
    m = c["c0"] * x0 + c["cx"] * x
    if np.any(c["cp"] != 0):
        prev = np.asarray(x0_prev, dtype=dtype)
        with np.errstate(invalid="ignore"):
            # where cp == 0 the previous x0 is not read: whatever it holds (NaN included) must not reach the result
            m = np.where(np.broadcast_to(c["cp"] != 0, m.shape), m + c["cp"] * prev, m)
    if z is not None and np.any(c["sigma"] != 0):
        zs = np.asarray(z, dtype=dtype) * c["sigma"]
        m = np.where(np.broadcast_to(c["sigma"] != 0, m.shape), m + zs, m)
    assert x0.dtype == dtype and m.dtype == dtype
    return x0, m


def run(rows, x, net_fn, noise=None, clip=False, dtype=np.float32):
    """The recurrence over K rows.  ``rows``: dict of COLUMNS -> (K,) arrays; ``net_fn(k, x)`` the network output at row
    k; ``noise``: None or K draws.  Returns (states after every row, the x0 of every row)."""
    K = len(rows["c0"])
    states, x0s, prev = [], [], None
    for k in range(K):
        row = {c: rows[c][k] for c in COLUMNS}
        x0, x = step(row, x, net_fn(k, x), prev, None if noise is None else noise[k], clip, dtype)
        prev = x0
        states.append(x)
        x0s.append(x0)
    return states, x0s
