"""Dense numpy restatement of gingr_model_augment (include/gingr_hip.h): the model whose mean is the sum of two models' means and whose
covariance is the sum of their covariances, and the cases and the tolerance constant the two test modules share.  No tests in here;
test_augment_model_host.py checks it against closed forms, test_gpu_augment_model.py checks the device against it.

The re-diagonalisation goes through the SVD of F = [Q_a | Q_b] -- on purpose a different route from the device's, which decomposes the
(ra + rb) x (ra + rb) Gram matrix F^T F; `augment_by_gram` is that second route on the host, kept to measure how far two correct
routes drift apart."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np


@dataclasses.dataclass
class Model:
    reference: np.ndarray   # (M, 3)
    mean: np.ndarray        # (M, 3) displacement
    variance: np.ndarray    # (r,)
    Q0: np.ndarray          # (3M, r) = basis sqrt(variance), rows 3 m + d
    all_variance: np.ndarray = None   # every eigenvalue the route produced, descending (results of augment only)

    @property
    def rank(self) -> int:
        return int(self.variance.shape[0])

    @property
    def basis(self) -> np.ndarray:
        return self.Q0 / np.sqrt(self.variance)[None, :]

    def operator(self, probes: np.ndarray) -> np.ndarray:
        """Q0 (Q0^T p) for the columns p of `probes` (3M, q)"""
        return self.Q0 @ (self.Q0.T @ probes)


def _keep(lam: np.ndarray, relative_tolerance: float, max_rank: int) -> int:
    kmax = min(max_rank, 512) if max_rank > 0 else 512
    k = 0
    while k < min(kmax, lam.shape[0]) and lam[k] > relative_tolerance * lam[0] and lam[k] > 0.0:
        k += 1
    return k


def _check(a: Model, b: Model):
    if a.reference.shape != b.reference.shape or not np.array_equal(a.reference, b.reference):
        raise ValueError("the two models need the same reference")
    if a.rank + b.rank > 512:
        raise ValueError("more than 512 columns: truncate first")


def augment(a: Model, b: Model, relative_tolerance: float = 1e-10, max_rank: int = 0) -> Model:
    """The definition, by the SVD of F = [Q_a | Q_b] = U diag(s) W^T: F F^T = Q_a Q_a^T + Q_b Q_b^T = U diag(s^2) U^T, variance s^2,
    Q0 = U diag(s)."""
    _check(a, b)
    F = np.concatenate([a.Q0, b.Q0], axis=1)
    U, s, _ = np.linalg.svd(F, full_matrices=False)
    lam = s * s
    k = _keep(lam, relative_tolerance, max_rank)
    if k < 1:
        raise ValueError("no eigenvalue passes the cutoff (rank 0)")
    return Model(a.reference, a.mean + b.mean, lam[:k], U[:, :k] * s[None, :k], lam)


def augment_by_gram(a: Model, b: Model, relative_tolerance: float = 1e-10, max_rank: int = 0) -> Model:
    """The same model through G = F^T F = [[S_a, C], [C^T, S_b]] = V diag(lambda) V^T, Q0 = Q_a V[:ra, :k] + Q_b V[ra:, :k] (the
    device's route, with LAPACK)."""
    _check(a, b)
    ra = a.rank
    C = a.Q0.T @ b.Q0
    G = np.block([[a.Q0.T @ a.Q0, C], [C.T, b.Q0.T @ b.Q0]])
    lam, V = np.linalg.eigh(G)
    lam, V = np.maximum(lam[::-1], 0.0), V[:, ::-1]
    k = _keep(lam, relative_tolerance, max_rank)
    if k < 1:
        raise ValueError("no eigenvalue passes the cutoff (rank 0)")
    return Model(a.reference, a.mean + b.mean, lam[:k], a.Q0 @ V[:ra, :k] + b.Q0 @ V[ra:, :k], lam)


def spectrum(r: int, top: float, span: float = 1e-4) -> np.ndarray:
    """r variances from `top` down to `top * span`, geometrically"""
    return top * span ** (np.arange(r) / max(r - 1, 1))


def random_model(rng: np.random.Generator, ref: np.ndarray, r: int, top: float, mean_size: float) -> Model:
    """orthonormal basis (r <= 3M), geometric spectrum, and a mean displacement of `mean_size` per coordinate, independent from vertex
    to vertex: with mean_size of the order of the reference's spread the spatial order of ref + mean has nothing to do with ref's"""
    M = ref.shape[0]
    assert r <= 3 * M
    U, _ = np.linalg.qr(rng.normal(size=(3 * M, r)))
    lam = spectrum(r, top)
    return Model(ref, rng.normal(0.0, mean_size, (M, 3)), lam, U * np.sqrt(lam)[None, :])


# ------------------------------------------------------------------------------------------------ shared by the two test modules
# (M, ra, rb): M below one tile; M no multiple of 16; several workgroups and slabs; every class of the padded widths (16, 32, 112 / 128,
# 256, above); ra + rb = 512 exactly; more columns than 3 M
CASES = [(5, 3, 4), (5, 10, 10), (37, 1, 16), (150, 17, 100), (150, 112, 113), (700, 40, 300), (2500, 100, 8), (300, 200, 312)]


@functools.lru_cache(maxsize=None)
def case(M: int, ra: int, rb: int):
    """(a, b) on one reference spread over 30 units, with means of 12 and 9 units per coordinate and total variances that differ"""
    rng = np.random.default_rng(100000 * M + 1000 * ra + rb)
    ref = rng.normal(0.0, 30.0, (M, 3))
    a = random_model(rng, ref, ra, 400.0, 12.0)
    b = random_model(rng, ref, rb, 90.0, 9.0)
    for m in (a, b):
        for arr in (m.reference, m.mean, m.variance, m.Q0):
            arr.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def expected(M: int, ra: int, rb: int) -> Model:
    m = augment(*case(M, ra, rb))
    for arr in (m.mean, m.variance, m.Q0, m.all_variance):
        arr.setflags(write=False)
    return m


def probes(rows: int) -> np.ndarray:
    return np.random.default_rng(9).normal(size=(rows, 8))


def spread(x: Model, y: Model):
    """(eigenvalues relative to lambda_1, operator on 8 probes relative to the result) between two routes to the same model"""
    assert x.rank == y.rank
    d_lam = float(np.abs(x.variance - y.variance).max() / x.variance[0])
    P = probes(x.Q0.shape[0])
    u, v = x.operator(P), y.operator(P)
    return d_lam, float((np.linalg.norm(u - v, axis=0) / np.linalg.norm(u, axis=0)).max())


# The largest discrepancy between the two routes to the same model in here (augment: SVD of [Q_a | Q_b], augment_by_gram:
# eigen-decomposition of its Gram matrix), relative to lambda_1 (eigenvalues) resp. to the result (operator on probes): measured by
# test_augment_model_host.py::test_route_spread_svd_against_gram over CASES; it prints every case and asserts that this constant covers
# them.  The GPU tolerance is 1000 x this, the margin the PCA tests give a device that sums in another order.
ROUTE_SPREAD = 1.4e-14
