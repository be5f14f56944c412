"""numpy restatement of the low-rank non-rigid CPD Maximization (gingr_amd/csrc/classic_cpd_lowrank.hip) and the inputs its tests
share.  With G ~ L L^T, D = diag(P1), c = lambda sigma2 and B = D^-1 P X - Y, the reference's step (G + c D^-1) W = B,
TY = Y + G W (NonRigidCPD.scala:45-88) is, by the Woodbury identity,

    S = L^T D L     s = L^T (P X - D Y)     (c I + S) z = s     V = L z     TY = Y + V     W = D (B - V) / c

and L^T W = z holds exactly.  Not a test module (no test_ prefix): tests/test_lowrank_cpd_host.py checks it against the oracle's
dense step on the CPU, tests/test_gpu_classic_cpd_lowrank.py uses it as the host side of its comparisons."""
import math

import numpy as np

from oracle import gingr_oracle as go


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def pair(M, N, seed, noise=0.05, scale=1.1):
    """the random pair of tests/test_gpu_classic_cpd.py"""
    rng = np.random.default_rng(seed)
    Y = rng.normal(0, 10, (M, 3))
    R = go.euler_to_rot(0.1, -0.2, 0.15)
    X = scale * Y[rng.permutation(M)[:N] if N <= M else rng.integers(0, M, N)] @ R.T + np.array([1.0, 2.0, -1.0]) + rng.normal(0, noise, (N, 3))
    return Y, X


def hull(M, N=None, seed=5, noise=0.3):
    """M points on the ellipsoid 50 (1, 0.7, 0.5) (unit normals scaled); the target: N (default: three quarters) of them, rotated,
    scaled by 1.05, with noise"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(M, 3))
    Y = u / np.linalg.norm(u, axis=1)[:, None] * (50.0 * np.array([1.0, 0.7, 0.5]))
    N = (3 * M) // 4 if N is None else N
    R = go.euler_to_rot(0.1, -0.2, 0.15)
    X = 1.05 * Y[rng.permutation(M)[:N]] @ R.T + rng.normal(0, noise, (N, 3))
    return Y, X


def factor(Y, beta, tol, max_columns=0):
    """the oracle's pivoted Cholesky of exp(-|a - b|^2 / (2 beta^2)) under the library's ceiling of 512 columns"""
    return go.pivoted_cholesky_scalar(Y, math.sqrt(2.0) * beta, 1.0, tol, max_columns if max_columns > 0 else 512)


def residual_fraction(L, columns=None):
    """trace(G - L_j L_j^T) / trace(G) for the leading j columns of a factor of the Gaussian kernel matrix (its diagonal is 1)"""
    j = L.shape[1] if columns is None else columns
    return float((1.0 - (L[:, :j] ** 2).sum(1)).sum() / L.shape[0])


def woodbury_step_stats(Y, P1, PX, xPx, sigma2, L, lam):
    """the step from the statistics of the Expectation alone: (TY, sigma2', W, z)"""
    c = lam * sigma2
    k = L.shape[1]
    S = L.T @ (P1[:, None] * L)
    s = L.T @ (PX - P1[:, None] * Y)
    z = np.linalg.solve(c * np.eye(k) + S, s)
    V = L @ z
    TY = Y + V
    W = P1[:, None] * ((PX / P1[:, None] - Y) - V) / c
    yPy = float(P1 @ (TY * TY).sum(1))
    trPXY = float((TY * PX).sum())
    return TY, (xPx - 2 * trPXY + yPy) / (P1.sum() * 3), W, z


def woodbury_step(X, Y, P, sigma2, L, lam):
    """the arguments of go.classic_cpd_maximization_nonrigid with L in place of G"""
    P1, Pt1 = P.sum(1), P.sum(0)
    return woodbury_step_stats(Y, P1, P @ X, float(Pt1 @ (X * X).sum(1)), sigma2, L, lam)
