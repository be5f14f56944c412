"""Dense numpy restatement of gingr_model_from_shapes (include/gingr_hip.h): Kabsch, the generalised Procrustes loop and PCA, and the
data sets and the tolerance constant the two test modules share.  No tests in here; test_pca_model_host.py checks it against closed forms, test_gpu_pca_model.py checks the device against it.

The PCA goes through the SVD of the centred data matrix -- on purpose a different route from the device's, which decomposes the n x n
Gram matrix; `pca_by_gram` is that second route on the host, kept to measure how far two correct routes drift apart."""
from __future__ import annotations

import dataclasses

import numpy as np


def kabsch(x: np.ndarray, target: np.ndarray):
    """(R, cx, ct) minimising sum |R (x_m - cx) + ct - target_m|^2 over rotations: centroids, 3 x 3 cross-covariance, SVD, last
    singular vector flipped when the determinant is negative, no scale."""
    x, target = np.asarray(x, dtype=np.float64), np.asarray(target, dtype=np.float64)
    cx, ct = x.mean(axis=0), target.mean(axis=0)
    S = (target - ct).T @ (x - cx) / x.shape[0]
    U, _, Vt = np.linalg.svd(S)
    D = np.diag([1.0, 1.0, -1.0 if np.linalg.det(S) < 0 else 1.0])
    return U @ D @ Vt, cx, ct


def align(x: np.ndarray, target: np.ndarray) -> np.ndarray:
    R, cx, ct = kabsch(x, target)
    return (x - cx) @ R.T + ct


@dataclasses.dataclass
class Aligned:
    shapes: np.ndarray      # (n, M, 3) aligned shapes
    reference: np.ndarray   # (M, 3): the model's reference (mode 2: the final target)
    sweeps: int
    last_change: float


def align_shapes(ref, shapes, alignment: int, gpa_max_iterations: int = 3, gpa_tolerance: float = 1e-5) -> Aligned:
    ref = np.asarray(ref, dtype=np.float64)
    X = np.array(shapes, dtype=np.float64)
    if alignment == 0:
        return Aligned(X, ref, 0, 0.0)
    if alignment == 1:
        return Aligned(np.stack([align(x, ref) for x in X]), ref, 0, 0.0)
    target, sweeps, change = ref, 0, 0.0
    for _ in range(gpa_max_iterations if gpa_max_iterations > 0 else 3):
        X = np.stack([align(x, target) for x in X])
        new = X.mean(axis=0)
        change = float(np.sqrt(((new - target) ** 2).sum() / ref.shape[0]))
        target = new
        sweeps += 1
        if change < gpa_tolerance:
            break
    return Aligned(X, target, sweeps, change)


@dataclasses.dataclass
class PcaModel:
    reference: np.ndarray   # (M, 3)
    mean: np.ndarray        # (M, 3) displacement: mean shape - reference
    variance: np.ndarray    # (k,)
    Q0: np.ndarray          # (3M, k) = U sqrt(variance), rows 3 m + d
    all_variance: np.ndarray  # every eigenvalue of the sample covariance the route produced, descending
    aligned: Aligned

    @property
    def rank(self) -> int:
        return int(self.variance.shape[0])

    @property
    def basis(self) -> np.ndarray:
        return self.Q0 / np.sqrt(self.variance)[None, :]

    def operator(self, probes: np.ndarray) -> np.ndarray:
        """Q0 (Q0^T p) for the columns p of `probes` (3M, q)"""
        return self.Q0 @ (self.Q0.T @ probes)


def _keep(lam: np.ndarray, n: int, relative_tolerance: float, max_rank: int) -> int:
    kmax = min(n - 1, min(max_rank, 512) if max_rank > 0 else 512)
    k = 0
    while k < min(kmax, lam.shape[0]) and lam[k] > relative_tolerance * lam[0] and lam[k] > 0.0:
        k += 1
    return k


def _centred(al: Aligned):
    n = al.shapes.shape[0]
    mu = al.shapes.mean(axis=0)
    Xc = (al.shapes - mu).reshape(n, -1).T / np.sqrt(n - 1.0)     # (3M, n)
    return mu, Xc


def pca_model(ref, shapes, alignment: int = 0, gpa_max_iterations: int = 3, gpa_tolerance: float = 1e-5, relative_tolerance: float = 1e-10,
              max_rank: int = 0) -> PcaModel:
    """The definition, PCA by the SVD of the centred data: Xc = U diag(s) W^T, variance s^2, Q0 = U diag(s)."""
    al = align_shapes(ref, shapes, alignment, gpa_max_iterations, gpa_tolerance)
    n = al.shapes.shape[0]
    mu, Xc = _centred(al)
    U, s, _ = np.linalg.svd(Xc, full_matrices=False)
    lam = s * s
    k = _keep(lam, n, relative_tolerance, max_rank)
    if k < 1:
        raise ValueError("all shapes identical (rank 0)")
    return PcaModel(al.reference, mu - al.reference, lam[:k], U[:, :k] * s[None, :k], lam, al)


def pca_by_gram(ref, shapes, alignment: int = 0, gpa_max_iterations: int = 3, gpa_tolerance: float = 1e-5, relative_tolerance: float = 1e-10,
                max_rank: int = 0) -> PcaModel:
    """The same model through the n x n Gram matrix Xc^T Xc = V diag(lambda) V^T, Q0 = Xc V (the device's route, with LAPACK)."""
    al = align_shapes(ref, shapes, alignment, gpa_max_iterations, gpa_tolerance)
    n = al.shapes.shape[0]
    mu, Xc = _centred(al)
    lam, V = np.linalg.eigh(Xc.T @ Xc)
    lam, V = np.maximum(lam[::-1], 0.0), V[:, ::-1]
    k = _keep(lam, n, relative_tolerance, max_rank)
    if k < 1:
        raise ValueError("all shapes identical (rank 0)")
    return PcaModel(al.reference, mu - al.reference, lam[:k], Xc @ V[:, :k], lam, al)


def known_spectrum_shapes(rng: np.random.Generator, M: int, n: int, lam) -> tuple:
    """(ref, shapes, U): shapes ref + sum_j sqrt(lam_j) a_ij u_j with orthonormal u_j (3M) and centred orthonormal coefficient columns
    a_j scaled by sqrt(n - 1): the sample covariance has exactly the eigenvalues lam_j with eigenvectors u_j.  len(lam) <= min(n - 1, 3M)."""
    lam = np.asarray(lam, dtype=np.float64)
    k = lam.shape[0]
    assert k <= min(n - 1, 3 * M)
    ref = rng.normal(0.0, 30.0, (M, 3))
    U, _ = np.linalg.qr(rng.normal(size=(3 * M, k)))
    A = rng.normal(size=(n, k))
    A -= A.mean(axis=0)
    A, _ = np.linalg.qr(A)                       # orthonormal columns; still centred (the span of centred columns is centred)
    A *= np.sqrt(n - 1.0)
    shapes = ref[None] + ((A * np.sqrt(lam)[None]) @ U.T).reshape(n, M, 3)
    return ref, shapes, U


def random_rigid(rng: np.random.Generator, translation: float = 20.0):
    """a proper rotation (QR of a Gaussian matrix, determinant fixed) and a translation"""
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))[None]
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q, rng.normal(0.0, translation, 3)


# ------------------------------------------------------------------------------------------------ shared by the two test modules
# (M, n) of the GPU tests and of the route-spread measurement: rank 1; small; across the 16-column padding with a ragged row count;
# several blocks; the first size past the register eigen-solver; 3 M < n - 1; the upper limit of n
SHAPES = [(37, 2), (37, 5), (257, 17), (1000, 40), (300, 193), (5, 20), (700, 512)]

# The largest discrepancy between the two routes to the same model in here (pca_model: SVD of the centred data, pca_by_gram:
# eigen-decomposition of its Gram matrix), relative to lambda_1 (eigenvalues) resp. to the result (operator on probes): measured by
# test_pca_model_host.py::test_route_spread_svd_against_gram over SHAPES (without alignment and with Procrustes) and LOW_RANK; it
# prints every case and asserts that this constant covers them.  The GPU tolerance is 1000 x this, the rule DESIGN.md section 4 uses
# for the posterior model.
ROUTE_SPREAD = 6.2e-15


def dataset(M, n, seed=0, modes=12, noise=0.05):
    """n shapes on a reference of M points: a few strong smooth modes plus a little noise in every coordinate (a full spectrum)"""
    rng = np.random.default_rng(1000 * M + n + seed)
    ref = rng.normal(0.0, 30.0, (M, 3))
    k = min(modes, 3 * M)
    B = rng.normal(size=(3 * M, k)) * (8.0 / np.sqrt(3 * M)) * (0.7 ** np.arange(k))[None]
    X = ref[None] + (rng.normal(size=(n, k)) @ B.T).reshape(n, M, 3) * np.sqrt(3 * M) + rng.normal(0.0, noise, (n, M, 3))
    return ref, X


# (M, n, r): n shapes drawn from a model of rank r < n - 1 -- what a chain's samples are; the Gram matrix has a null space of n - r
# dimensions with nothing special about its directions
LOW_RANK = [(300, 30, 4), (120, 200, 10)]


def low_rank_dataset(M, n, r):
    rng = np.random.default_rng(M + n + r)
    ref = rng.normal(0.0, 30.0, (M, 3))
    B = rng.normal(size=(3 * M, r)) * (0.7 ** np.arange(r))[None] * 3.0
    return ref, ref[None] + (rng.normal(size=(n, r)) @ B.T).reshape(n, M, 3)
