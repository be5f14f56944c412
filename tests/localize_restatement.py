"""Dense numpy restatement of gingr_model_localize (include/gingr_hip.h): the model whose covariance is the source's multiplied
element-wise by a Gaussian taper over the reference, and the cases and the tolerance constant the two test modules share.  No tests in
here; test_localize_model_host.py checks it against exact properties, test_gpu_localize_model.py checks the device against it.

    K[(i,a),(j,b)] = exp(-|x_i - x_j|^2 / sigma^2) * sum_k Q[3i+a, k] Q[3j+b, k]            (np.exp)
    K ~ L L^T   pivoted Cholesky over the 3M entries: the first maximal residual, until the residual trace is below tol * trace, 512
                columns are computed, or no positive residual is left
    L^T L = V diag(lam) V^T (eigh), Q' = L V; kept: lam_j > 1e-12 lam_1 and > 0, at most max_rank (0: 512) and 512

`expected` never takes the eigen-decomposition of K itself: `dense_eigh` does, for the cases small enough (the host test's second route)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests.augment_restatement import Model, probes, random_model  # noqa: F401  (probes: re-exported for the test modules)

CEILING = 512       # columns of the generic factor
CUTOFF = 1e-12      # noise floor of the Gram route


@dataclasses.dataclass
class Localized:
    model: Model                 # reference, mean, variance (kept), Q0 (kept), all_variance (every eigenvalue of L^T L, descending, >= 0)
    columns: int
    tolerance_reached: bool
    residual_fraction: float
    total_variance: float
    pivots: np.ndarray           # (columns,) entry indices 3 i + d
    traces: np.ndarray           # (columns + 1,) residual trace after 0 .. columns columns


def taper(ref: np.ndarray, sigma: float) -> np.ndarray:
    d = ref[:, None, :] - ref[None, :, :]
    return np.exp(-(d * d).sum(axis=2) / (sigma * sigma))


def dense_K(src: Model, sigma: float) -> np.ndarray:
    """(3M, 3M); built in place: one 3M x 3M array and one M x M"""
    M = src.reference.shape[0]
    K = src.Q0 @ src.Q0.T
    K.reshape(M, 3, M, 3)[...] *= taper(src.reference, sigma)[:, None, :, None]
    return K


def pivoted_cholesky(K: np.ndarray, tol: float, dtype=np.float64, ceiling: int = CEILING):
    """L (columns, n) with K ~ L^T L in this layout (row s = column s of the factor), pivots, residual traces.  Arithmetic in `dtype`
    (np.longdouble: the pivot-stability check); a column of K is converted when it is needed."""
    n = K.shape[0]
    cap = min(n, ceiling)
    d = np.diag(K).astype(dtype)
    free = np.ones(n, dtype=bool)
    L = np.zeros((cap, n), dtype=dtype)
    pivots, traces = [], []
    trace0 = d.sum()
    k = 0
    while True:
        tr = d[free].sum() if k > 0 else trace0
        traces.append(tr)
        if k >= cap or not free.any() or not (tr >= tol * trace0):
            break
        cand = np.where(free, d, -np.inf)
        p = int(np.argmax(cand))                    # the first maximal residual
        if not (cand[p] > 0.0):
            break
        lpk = np.sqrt(cand[p])
        col = (K[:, p].astype(dtype) - L[:k].T @ L[:k, p]) / lpk
        col[~free] = 0.0
        col[p] = lpk
        L[k] = col
        free[p] = False
        d = d - col * col
        pivots.append(p)
        k += 1
    return L[:k], np.array(pivots, dtype=np.int64), np.array(traces, dtype=dtype)


def keep_count(lam: np.ndarray, max_rank: int) -> int:
    kmax = min(max_rank, 512) if max_rank > 0 else 512
    k = 0
    while k < min(kmax, lam.shape[0]) and lam[k] > CUTOFF * lam[0] and lam[k] > 0.0:
        k += 1
    return k


def localize_from_K(src: Model, K: np.ndarray, tol: float, max_rank: int = 0) -> Localized:
    L, pivots, traces = pivoted_cholesky(K, tol)
    cols = L.shape[0]
    if cols < 1:
        raise ValueError("rank 0")
    lam, V = np.linalg.eigh(L @ L.T)
    lam, V = np.maximum(lam[::-1], 0.0), V[:, ::-1]
    k = keep_count(lam, max_rank)
    if k < 1:
        raise ValueError("no eigenvalue passes the cutoff (rank 0)")
    n = K.shape[0]
    reached = (not (traces[cols] >= tol * traces[0])) or cols < min(n, CEILING) or cols == n
    model = Model(src.reference, src.mean, lam[:k], L.T @ V[:, :k], lam)
    return Localized(model, cols, bool(reached), float(traces[cols] / traces[0]), float(traces[0]), pivots, traces)


def localize(src: Model, sigma: float, tol: float = 0.01, max_rank: int = 0) -> Localized:
    return localize_from_K(src, dense_K(src, sigma), tol, max_rank)


def dense_eigh(src: Model, K: np.ndarray, max_rank: int = 0) -> Model:
    """the same model from the eigen-decomposition of K itself (no factor, no tolerance): the second route of the full factorisations"""
    lam, U = np.linalg.eigh(K)
    lam, U = np.maximum(lam[::-1], 0.0), U[:, ::-1]
    k = keep_count(lam, max_rank)
    return Model(src.reference, src.mean, lam[:k], U[:, :k] * np.sqrt(lam[:k])[None, :], lam)


# ------------------------------------------------------------------------------------------------ shared by the two test modules
# (M, r, sigma, tol)
FULL_CASES = [
    (5, 3, 40.0, 0.0),        # 15 entries, far below one workgroup
    (37, 1, 25.0, 0.0),       # rank-1 source: K has rank 37 of 111 entries, the factor stops by exhaustion
    (37, 16, 25.0, 0.0),      # 111 entries, no multiple of 16
    (86, 20, 30.0, 0.0),      # 258 entries: two past the 256-entry workgroup
    (150, 100, 15.0, 0.0),    # 450 entries, the basis dot product longer than the factor's for the first 100 steps, rp = 112
    (170, 8, 60.0, 0.0),      # 510 entries: the swap log almost full
]
STOPPED_CASES = [
    (171, 8, 60.0, 0.0),      # 513 entries: the ceiling with the tolerance unreachable
    (700, 8, 400.0, 1e-8),    # several workgroups, stops at the tolerance
    (2500, 3, 500.0, 1e-8),   # ten workgroups
    (700, 40, 900.0, 1e-8),   # the ceiling above the tolerance
    (300, 512, 400.0, 1e-8),  # the widest source (rp = 512)
    (700, 8, 400.0, 1e-2),    # a loose tolerance
]
CASES = FULL_CASES + STOPPED_CASES
PIVOT_STABLE = [(700, 8, 400.0, 1e-8), (2500, 3, 500.0, 1e-8)]   # the host test asserts it; the GPU test then asks for equal columns
TOLERANCE_REACHED = {c: c not in [(171, 8, 60.0, 0.0), (700, 40, 900.0, 1e-8), (300, 512, 400.0, 1e-8)] for c in CASES}


@functools.lru_cache(maxsize=None)
def source(M: int, r: int) -> Model:
    rng = np.random.default_rng(1000 * M + r)
    ref = rng.normal(0.0, 30.0, (M, 3))
    m = random_model(rng, ref, r, 400.0, 12.0)
    for arr in (m.reference, m.mean, m.variance, m.Q0):
        arr.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def case_K(M: int, r: int, sigma: float) -> np.ndarray:
    K = dense_K(source(M, r), sigma)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def expected(M: int, r: int, sigma: float, tol: float, max_rank: int = 0) -> Localized:
    x = localize_from_K(source(M, r), case_K(M, r, sigma), tol, max_rank)
    for arr in (x.model.variance, x.model.Q0, x.model.all_variance, x.pivots, x.traces):
        arr.setflags(write=False)
    return x


def spread(x: Model, y: Model):
    """(eigenvalues relative to lambda_1, operator on the 8 probes relative to the result) between two routes to the same model"""
    assert x.rank == y.rank
    d_lam = float(np.abs(x.variance - y.variance).max() / x.variance[0])
    P = probes(x.Q0.shape[0])
    u, v = x.operator(P), y.operator(P)
    return d_lam, float((np.linalg.norm(u - v, axis=0) / np.linalg.norm(u, axis=0)).max())


# The largest discrepancy between the two routes to the same model in here (localize: pivoted Cholesky, Gram matrix, eigh; dense_eigh:
# eigh of K itself) over FULL_CASES, relative to lambda_1 (eigenvalues) resp. to the result (operator on probes): measured by
# test_localize_model_host.py::test_route_spread, which prints every case and asserts that this constant covers them.  The GPU
# tolerance is 1000 x this, the margin the PCA and augment tests give a device that sums in another order.
ROUTE_SPREAD = 5e-15
