"""Plain-numpy restatement of the kernels of gingr_gpmm_build_radial, in the form the oracle's generic pivoted Cholesky takes
(`kfun(dim, rows, j)` of go.pivoted_cholesky_diagonal_kernel / go.build_gpmm_diagonal):

    k(x_i, x_j) = sum_t  w_t[i] w_t[j] scaling_t f_t(nn),      nn = |x_i - x_j|^2 = dx dx + dy dy + dz dz (unfused, left to right)

    gaussian             f = exp(-nn / sigma^2)
    rationalQuadratic    f = 1 - nn / (nn + beta^2)          (KernelHelper.scala:64-73)
    inverseMultiquadric  f = 1 / sqrt(nn + beta^2)           (KernelHelper.scala:53-61)

One term's value is ((scaling * f) * w[i]) * w[j], without the two weight factors when the term has no field; the terms are added left
to right, the first one assigned.  A term is the tuple (family, parameter, scaling, weight or None)."""
import numpy as np

from oracle import gingr_oracle as go

GAUSSIAN, RATIONAL_QUADRATIC, INVERSE_MULTIQUADRIC = "gaussian", "rationalQuadratic", "inverseMultiquadric"


def family_value(family, parameter, nn):
    p2 = parameter * parameter
    if family == GAUSSIAN:
        return np.exp(-nn / p2)
    if family == RATIONAL_QUADRATIC:
        return 1.0 - nn / (nn + p2)
    if family == INVERSE_MULTIQUADRIC:
        return 1.0 / np.sqrt(nn + p2)
    raise ValueError(family)


def kernel_values(P, terms, rows, j):
    """k(point rows[i], point j) as a vector"""
    d = P[rows] - P[j]
    nn = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    v = None
    for family, parameter, scaling, w in terms:
        e = scaling * family_value(family, parameter, nn)
        if w is not None:
            e = (e * w[rows]) * w[j]
        v = e if v is None else v + e
    return v


def kfun(P, terms_xyz):
    """terms_xyz: one list of terms for all three coordinates, or a tuple (terms_x, terms_y, terms_z)"""
    P = np.asarray(P, dtype=np.float64)
    per = terms_xyz if isinstance(terms_xyz, tuple) else (terms_xyz,) * 3
    return lambda dim, rows, j: kernel_values(P, per[dim], np.asarray(rows), int(j))


def dense(P, terms):
    P = np.asarray(P, dtype=np.float64)
    rows = np.arange(P.shape[0])
    return np.stack([kernel_values(P, terms, rows, j) for j in range(P.shape[0])], axis=1)


def change_point_terms(pars_a, pars_b, indicator):
    """scalismo's ChangePointKernel: the Gaussians (sigma, scaling) of A weighted by the indicator, then those of B by 1 - indicator"""
    s = np.asarray(indicator, dtype=np.float64)
    return [(GAUSSIAN, sg, sc, s) for sg, sc in pars_a] + [(GAUSSIAN, sg, sc, 1.0 - s) for sg, sc in pars_b]


def sigmoid_field(P, point, normal, width):
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.sqrt((n * n).sum())
    return 1.0 / (1.0 + np.exp(-((np.asarray(P, dtype=np.float64) - np.asarray(point, dtype=np.float64)) @ n) / width))


def factor(P, terms_xyz, rel_tol, max_cols=None):
    """L (3M x k) of the generic pivoted Cholesky over the restated kernels"""
    return go.pivoted_cholesky_diagonal_kernel(np.asarray(P).shape[0], kfun(P, terms_xyz), rel_tol, max_cols)


def model_of(P, L, keep=None):
    U, lam = go.approximate_eig(L)
    if keep is not None:
        U, lam = U[:, :keep], lam[:keep]
    P = np.asarray(P, dtype=np.float64)
    return go.PDM(ref=P, mean=np.zeros_like(P), U=np.ascontiguousarray(U), lam=lam)


def stop_margin(P, terms_xyz, L, rel_tol):
    """How far, relative to the threshold rel_tol * trace, the residual trace stayed from it around the stop: (trace before the last
    column - threshold) / threshold and (threshold - trace after it) / threshold.  Both must be positive for a stop at the tolerance,
    and at least 1e-6 for rounding not to move the stop."""
    k = kfun(P, terms_xyz)
    M = np.asarray(P).shape[0]
    tr0 = sum(float(k(dim, np.array([i]), i)[0]) for dim in range(3) for i in range(M))
    tr = tr0 - np.concatenate([[0.0], np.cumsum((L * L).sum(axis=0))])
    thr = rel_tol * tr0
    return (tr[-2] - thr) / thr, (thr - tr[-1]) / thr
