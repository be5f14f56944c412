"""numpy restatement of gingr_pca_leave_one_out (include/gingr_hip.h; gingr_amd/csrc/pca_leave_one_out.hip): the leave-one-out
generalization of a PCA shape model by two routes, and the tolerance constant the two test modules share.  No tests in here;
test_pca_loo_host.py checks the routes against each other and against hand-worked cases, test_gpu_pca_loo.py checks the device.

  loo_direct   the definition: for every shape i the PCA model of the other n - 1 shapes (pca_restatement.pca_model: the SVD of their
               centred data, no alignment), shape i projected onto its k leading components in longdouble
               (model_metrics_restatement.project_direct: the ridge regression with noise 1e-5), distances vertex to vertex
  loo_gram     the device's route in float64: one Gram matrix G = D^T D of the shapes centred on the mean of all n, every fold's Gram
               matrix a rank-two correction of it, every fold's error field D w with an n-vector w worked out in n-space
"""
from __future__ import annotations

import numpy as np

from tests import model_metrics_restatement as mm
from tests import pca_restatement as pr

EPS = mm.EPS  # GINGR_COEFF_NOISE

# The largest difference between loo_direct and loo_gram (avg and max, every rank, every shape) relative to max |shape - ref|, over
# CASES and LOW_RANK below: measured by test_pca_loo_host.py::test_route_spread_direct_against_gram, which prints every case and
# asserts that this constant covers them.  Measured 3.5e-13, worst at (M, n) = (17, 18) at full fold rank -- 1.8e-13 at (257, 17),
# 2.8e-13 at (130, 40), 3e-15 and below wherever the last rank stays under the fold rank: the ridge solve divides by lambda_j + 1e-5
# with lambda_j down at the noise level of the data set, and the smallest kept eigenvalue carries the route's rounding.
# The GPU tolerance is 1000 x this, the rule of pca_restatement.ROUTE_SPREAD.
LOO_ROUTE_SPREAD = 4.0e-13

# (M, n, ranks): a fold of two shapes; 3 M < n - 2 with the last rank clipped to the fold rank 3; small; the 16-column padding with
# ragged rows; full fold rank; 16 ranks and more than 512 weight columns; the last size on the batched register kernel (folds of
# 192, fold rank 180 = 3 M); the first size past it
CASES = [
    (37, 3, [1]),
    (1, 8, [1, 2, 3, 6]),
    (37, 5, [1, 2, 3]),
    (17, 16, [1, 5, 14]),
    (17, 17, [1, 8, 15]),
    (17, 18, [2, 9, 16]),
    (257, 17, [1, 4, 15]),
    (130, 40, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 20, 30, 38]),
    (60, 193, [1, 6, 12]),
    (60, 194, [1, 6, 12]),
]
# (M, n, r, ranks): shapes drawn from a model of rank r: a null space of many dimensions in every fold; ranks above r are clipped to r
LOW_RANK = [(300, 30, 4, [2, 4, 10])]


def fold_is_rank0(others: np.ndarray) -> bool:
    """the rule of gingr_model_from_shapes for "all shapes are identical": the total variance lies within the rounding of the mean"""
    nf = others.shape[0]
    mu = others.mean(axis=0)
    trace = float(((others - mu) ** 2).sum()) / (nf - 1.0)
    return not trace > (64.0 + nf * nf) * (2.0 ** -52) ** 2 * float((mu * mu).sum())


def loo_direct(shapes, ranks, relative_tolerance: float = 1e-10):
    """avg, max [n_ranks, n] (float64, from longdouble) and fold_rank [n]"""
    X = np.asarray(shapes, dtype=np.float64)
    n, M = X.shape[0], X.shape[1]
    ranks = [int(k) for k in ranks]
    avg, mx, fold_rank = np.zeros((len(ranks), n)), np.zeros((len(ranks), n)), np.zeros(n, dtype=np.int32)
    for i in range(n):
        others = np.delete(X, i, axis=0)
        if fold_is_rank0(others):
            dist = mm.vertex_distances(X[i].reshape(1, -1), np.asarray(others, dtype=mm.LD).mean(axis=0).reshape(1, -1))[0]
            avg[:, i], mx[:, i] = float(dist.sum() / mm.LD(M)), float(dist.max())
            continue
        ref = others.mean(axis=0)
        pm = pr.pca_model(ref, others, alignment=0, relative_tolerance=relative_tolerance, max_rank=0)
        fold_rank[i] = pm.rank
        model = mm.Model(pm.reference, pm.mean, pm.basis, pm.variance)
        _, a, m = mm.project_direct(model, X[i][None], [min(k, pm.rank) for k in ranks])
        avg[:, i], mx[:, i] = np.asarray(a[:, 0], dtype=np.float64), np.asarray(m[:, 0], dtype=np.float64)
    return avg, mx, fold_rank


def fold_weights(G: np.ndarray, i: int, ranks, relative_tolerance: float, rank0: bool = False):
    """(w [n_ranks, n], fold_rank) of fold i from the Gram matrix of the shapes centred on the mean of all n"""
    n = G.shape[0]
    a = 1.0 / (n - 1.0)
    J = np.array([j for j in range(n) if j != i])
    w = np.zeros((len(ranks), n))
    w[:, i] = -(1.0 + a)
    if rank0:
        return w, 0
    Gf = (G[np.ix_(J, J)] + a * (G[J, i][:, None] + G[i, J][None, :]) + a * a * G[i, i]) / (n - 2.0)
    shift = np.trace(Gf) / (n - 1.0)          # the mean eigenvalue: a centred Gram matrix is always singular (pca_model.hip)
    lam, V = np.linalg.eigh(Gf + shift * np.eye(n - 1))
    lam, V = np.maximum(lam[::-1] - shift, 0.0), V[:, ::-1]
    rank = 0
    while rank < n - 2 and lam[rank] > relative_tolerance * lam[0] and lam[rank] > 0.0:
        rank += 1
    g = (1.0 + a) * (G[J, i] + a * G[i, i])
    b = V.T @ g / np.sqrt(n - 2.0)
    for q, k in enumerate(ranks):
        kk = min(int(k), rank)
        alpha = b[:kk] / (lam[:kk] + EPS)
        c = V[:, :kk] @ alpha / np.sqrt(n - 2.0)
        w[q, J] = c
        w[q, i] = a * c.sum() - (1.0 + a)
    return w, rank


def loo_gram(shapes, ranks, relative_tolerance: float = 1e-10):
    """the same figures by the device's route, float64 throughout"""
    X = np.asarray(shapes, dtype=np.float64)
    n, M = X.shape[0], X.shape[1]
    D = (X - X.mean(axis=0)).reshape(n, -1)     # rows: the columns d_j of the text
    G = D @ D.T
    avg, mx, fold_rank = np.zeros((len(ranks), n)), np.zeros((len(ranks), n)), np.zeros(n, dtype=np.int32)
    for i in range(n):
        w, fold_rank[i] = fold_weights(G, i, ranks, relative_tolerance, fold_is_rank0(np.delete(X, i, axis=0)))
        E = (w @ D).reshape(len(ranks), M, 3)
        dist = np.sqrt((E * E).sum(axis=-1))
        avg[:, i], mx[:, i] = dist.sum(axis=1) / M, dist.max(axis=1)
    return avg, mx, fold_rank


def scale_of(ref, shapes) -> float:
    return float(np.abs(np.asarray(shapes) - np.asarray(ref)[None]).max())
