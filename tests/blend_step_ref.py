"""The contract of include/dsx.h (dsx_tileplan_blend_step) restated in numpy float32: the blend of tests/blend_ref.py,
then the three operations of the step in the contract's order, one numpy operation per rounding.  The noise is an input."""
import numpy as np

from tests import blend_ref


def blend_step_ref(plan, x0_tiles, wy, wx, X, c_x0, c_xt, sigma, Z, dtype=np.float32):
    """x0_tiles (total, C, ph, pw), state X and noise Z (N, H, W, C) -> the new state (N, H, W, C):
    v = blend; mean = c_x0 * v + c_xt * X; out = mean (sigma == 0: Z is not looked at) or mean + Z * sigma."""
    f = dtype
    v = blend_ref.blend_ref(plan, x0_tiles, wy, wx, dtype=f)
    X = np.asarray(X, dtype=f)
    assert v.shape == X.shape
    mean = ((f(c_x0) * v).astype(f) + (f(c_xt) * X).astype(f)).astype(f)
    if f(sigma) == 0:
        return mean
    Z = np.asarray(Z, dtype=f)
    assert Z.shape == X.shape
    return (mean + (Z * f(sigma)).astype(f)).astype(f)
