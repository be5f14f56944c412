"""numpy restatement of the model metrics (gingr_amd/csrc/model_metrics.hip) in np.longdouble, and the error bounds the device results
are held to.  Not a test module: tests/test_model_metrics_host.py and tests/test_gpu_model_metrics.py import it.

The model is (ref, mean, Q) with Q = basis * sqrt(variance) rounded to float64 -- what the device keeps as Q0 -- rows 3 i + d in the
caller's point order.  Everything below that is longdouble (unit roundoff 2^-64: its own error does not show beside 2^-53).

  projection     alpha_k = (Q_k^T Q_k / eps + I)^-1 Q_k^T (x - ref - mean) / eps, eps = 1e-5, Q_k the k leading columns: the leading
                 block solved DIRECTLY (project_direct), and through the one factor the device uses (project_nested):
                 B = Q^T Q / eps + I = L L^T, W = L^-T, alpha_k = W_k W_k^T (b_k / eps) with W_k the leading k x k block
  distances      vertex to corresponding vertex; mean = (sum over the vertices) / M
  specificity    the smallest mean distance over the training shapes, the lowest index on an exact tie (np.argmin)
"""
import dataclasses

import numpy as np

LD = np.longdouble
U = 2.0 ** -53   # unit roundoff of float64
EPS = 1e-5       # GINGR_COEFF_NOISE


@dataclasses.dataclass
class Model:
    ref: np.ndarray       # (M, 3)
    mean: np.ndarray      # (M, 3)
    basis: np.ndarray     # (3 M, r)
    variance: np.ndarray  # (r,)

    @property
    def M(self):
        return self.ref.shape[0]

    @property
    def rank(self):
        return self.variance.shape[0]

    @property
    def Q(self):
        """float64, as the device packs it: one correctly rounded square root and one product per entry"""
        return np.asarray(self.basis, dtype=np.float64) * np.sqrt(np.asarray(self.variance, dtype=np.float64))[None, :]


def variances(r):
    """r values from 64 down to 0.25, geometrically spaced (one value: 64)"""
    return 64.0 * (0.25 / 64.0) ** (np.arange(r) / max(r - 1, 1))


def random_model(M, r, seed, scale=None):
    """A basis of random columns, NOT orthonormalised (Q^T Q is full, and so is (Q^T Q / eps + I)^-1), columns of norm about 1;
    variances within [0.25, 64]."""
    rng = np.random.default_rng(seed)
    ref = rng.normal(0.0, 30.0, (M, 3))
    mean = rng.normal(0.0, 1.0, (M, 3))
    basis = rng.normal(0.0, 1.0, (3 * M, r)) / np.sqrt(3.0 * M)
    return Model(ref, mean, basis, variances(r))


# ----------------------------------------------------------------------------------------------------- longdouble linear algebra
def cholesky(B):
    n = B.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = B[j, j] - L[j, :j] @ L[j, :j]
        assert s > 0, "not positive definite"
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (B[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, rhs):
    x = np.array(rhs, dtype=LD)
    for j in range(L.shape[0]):
        x[j] = (x[j] - L[j, :j] @ x[:j]) / L[j, j]
    return x


def solve_upper(Uu, rhs):
    x = np.array(rhs, dtype=LD)
    for j in range(Uu.shape[0] - 1, -1, -1):
        x[j] = (x[j] - Uu[j, j + 1:] @ x[j + 1:]) / Uu[j, j]
    return x


def solve_spd(B, rhs):
    L = cholesky(B)
    return solve_upper(L.T, solve_lower(L, rhs))


def norm_inf(A):
    return np.abs(A).sum(axis=1).max()


def system(Q, k):
    """B_k = Q_k^T Q_k / eps + I in longdouble"""
    Qk = np.asarray(Q, dtype=LD)[:, :k]
    return Qk.T @ Qk / LD(EPS) + np.eye(k, dtype=LD)


def condition(Q, k=None):
    """the infinity-norm condition number of B_k, in longdouble"""
    B = system(Q, Q.shape[1] if k is None else k)
    return float(norm_inf(B) * norm_inf(solve_spd(B, np.eye(B.shape[0], dtype=LD))))


# ------------------------------------------------------------------------------------------------------------- the three measures
def centred(model, shapes):
    """(n, 3 M): x - ref - mean"""
    X = np.asarray(shapes, dtype=LD).reshape(-1, 3 * model.M)
    return X - np.asarray(model.ref, dtype=LD).reshape(1, -1) - np.asarray(model.mean, dtype=LD).reshape(1, -1)


def vertex_distances(A, B):
    """(..., M): |a_v - b_v| for arrays of (..., 3 M)"""
    D = (np.asarray(A, dtype=LD) - np.asarray(B, dtype=LD))
    D = D.reshape(D.shape[:-1] + (-1, 3))
    return np.sqrt((D * D).sum(axis=-1))


def measure(model, D, coef, ranks):
    """avg, max [n_ranks, n] of |Q alpha - d| per vertex"""
    Q = np.asarray(model.Q, dtype=LD)
    avg, mx = np.zeros(coef.shape[:2], dtype=LD), np.zeros(coef.shape[:2], dtype=LD)
    for q in range(len(ranks)):
        dist = vertex_distances(coef[q] @ Q.T, D)
        avg[q], mx[q] = dist.sum(axis=1) / LD(model.M), dist.max(axis=1)
    return avg, mx


def project_direct(model, shapes, ranks):
    """coef [n_ranks, n, r] (zero from entry k on), avg, max [n_ranks, n]: every leading block solved on its own"""
    Q, D = np.asarray(model.Q, dtype=LD), centred(model, shapes)
    coef = np.zeros((len(ranks), D.shape[0], model.rank), dtype=LD)
    for q, k in enumerate(ranks):
        coef[q, :, :k] = solve_spd(system(Q, k), Q[:, :k].T @ D.T / LD(EPS)).T
    return (coef,) + measure(model, D, coef, ranks)


def project_nested(model, shapes, ranks):
    """the same through one factorisation: W = L^-T of the full system, alpha_k = W_k W_k^T (b_k / eps)"""
    Q, D = np.asarray(model.Q, dtype=LD), centred(model, shapes)
    r = model.rank
    W = solve_lower(cholesky(system(Q, r)), np.eye(r, dtype=LD)).T
    rhs = Q.T @ D.T / LD(EPS)
    coef = np.zeros((len(ranks), D.shape[0], r), dtype=LD)
    for q, k in enumerate(ranks):
        coef[q, :, :k] = (W[:k, :k] @ (W[:k, :k].T @ rhs[:k])).T
    return (coef,) + measure(model, D, coef, ranks)


def instances(model, alphas):
    """(n, M, 3): ref + mean + Q alpha"""
    A = np.asarray(alphas, dtype=LD).reshape(-1, model.rank)
    base = np.asarray(model.ref, dtype=LD).reshape(1, -1) + np.asarray(model.mean, dtype=LD).reshape(1, -1)
    return (base + A @ np.asarray(model.Q, dtype=LD).T).reshape(A.shape[0], model.M, 3)


def truncated(alphas, k):
    A = np.array(alphas, dtype=np.float64).reshape(-1, np.shape(alphas)[-1])
    A[:, k:] = 0.0
    return A


def specificity(model, train, alphas, ranks):
    """means [n_ranks, S, n_train], min_avg [n_ranks, S], argmin [n_ranks, S]"""
    T = np.asarray(train, dtype=LD).reshape(-1, 3 * model.M)
    S = np.asarray(alphas).reshape(-1, model.rank).shape[0]
    means = np.zeros((len(ranks), S, T.shape[0]), dtype=LD)
    for q, k in enumerate(ranks):
        smp = instances(model, truncated(alphas, k)).reshape(S, 1, -1)
        means[q] = vertex_distances(smp, T[None]).sum(axis=-1) / LD(model.M)
    return means, means.min(axis=-1), means.argmin(axis=-1)


def compactness(variance):
    v = np.asarray(variance, dtype=LD)
    return np.cumsum(v) / v.sum()


# ------------------------------------------------------------------------------------------------------------------- the bounds
# Derived from the summation lengths, the unit roundoff u and the conditioning of the solve -- not from what any implementation gives.
# A sum of n products in any order (FMA or not) is off by at most (n + 2) u sum |terms| (gamma_n, first order, with slack).
def instance_bound(model, alphas):
    """(n, M, 3), per coordinate: the sum of r products, the two additions of ref and mean, and 4 u relative on Q itself (a model
    that went through a download: basis = Q0 / sd, Q = basis * sd)."""
    A = np.abs(np.asarray(alphas, dtype=LD).reshape(-1, model.rank))
    absQ = np.abs(np.asarray(model.Q, dtype=LD))
    got = np.abs(instances(model, alphas)).reshape(A.shape[0], -1)
    base = np.abs(np.asarray(model.ref, dtype=LD)).reshape(1, -1) + np.abs(np.asarray(model.mean, dtype=LD)).reshape(1, -1)
    b = (model.rank + 6) * LD(U) * (A @ absQ.T) + 3 * LD(U) * (base + got)
    return b.reshape(A.shape[0], model.M, 3).astype(np.float64)


def projection_bounds(model, shapes, ranks):
    """cond [n_ranks], coef [n_ranks, n], avg [n_ranks, n], max [n_ranks, n] for one route from the shapes to the figures.
      d = x - ref - mean          two roundings: |dd| <= 2 u (|x| + |ref| + |mean|)
      b = Q_k^T d                 3 M products: |db| <= (3 M + 2) u |Q_k|^T |d| + |Q_k|^T |dd|
      B = S / eps + I             S from 3 M products per entry, one division, one addition:
                                  |dB|_inf <= 2 ((3 M + 2) u | |Q_k|^T |Q_k| |_inf / eps + 2 u |B|_inf)
      alpha = B^-1 (b / eps)      through the explicit triangular inverse W = L^-T (or the inverse B^-1 = W W^T) and two products of
                                  length k: a computed triangular inverse is off by gamma_k |W| |L^T| |W|, i.e. by k u sqrt(cond) in norm,
                                  the products by gamma_k each, all of it acting on | |W| |W^T| |_inf |b / eps|_inf <= k |B^-1| |b / eps|:
                                  |dalpha| <= |B^-1| |db| / eps + |B^-1| |dB| |alpha| + 4 k^2 (1 + sqrt(cond)) u |B^-1| |b / eps|
      (Q alpha)_row               k products: <= |Q_row|_1 |dalpha| + (k + 6) u |Q_row| |alpha|     (+ 4 u on Q itself, see instance_bound)
      |Q alpha - d|_vertex        | |a| - |b| | <= |a - b|: the three rows' errors and dd add up; the norm itself 4 u of the distance
      mean                        the slab sums: (M + 2) u of the mean
    """
    u = LD(U)
    Q, D = np.asarray(model.Q, dtype=LD), centred(model, shapes)
    M, n = model.M, D.shape[0]
    X = np.abs(np.asarray(shapes, dtype=LD).reshape(n, -1))
    dd = 2 * u * (X + np.abs(np.asarray(model.ref, dtype=LD)).reshape(1, -1) + np.abs(np.asarray(model.mean, dtype=LD)).reshape(1, -1))
    coef, avg, mx = project_direct(model, shapes, ranks)
    out = {"cond": np.zeros(len(ranks)), "coef": np.zeros((len(ranks), n)), "avg": np.zeros((len(ranks), n)), "max": np.zeros((len(ranks), n))}
    for q, k in enumerate(ranks):
        Qk, absQ = Q[:, :k], np.abs(Q[:, :k])
        B = system(Q, k)
        nB, nBinv = norm_inf(B), norm_inf(solve_spd(B, np.eye(k, dtype=LD)))
        cond = nB * nBinv
        rhs = np.abs(Qk.T @ D.T).max(axis=0) / LD(EPS)                                           # |b / eps|_inf per shape
        db = ((3 * M + 2) * u * (absQ.T @ np.abs(D).T) + absQ.T @ dd.T).max(axis=0)               # per shape
        dB = 2 * ((3 * M + 2) * u * norm_inf(absQ.T @ absQ) / LD(EPS) + 2 * u * nB)
        a = np.abs(coef[q, :, :k])
        dalpha = nBinv * db / LD(EPS) + nBinv * dB * a.max(axis=1) + 4 * k * k * (1 + np.sqrt(cond)) * u * nBinv * rhs
        rows = absQ.sum(axis=1)[None, :] * dalpha[:, None] + (k + 6) * u * (a @ absQ.T) + dd + u * np.abs(D)
        vertex = rows.reshape(n, M, 3).sum(axis=2).max(axis=1)
        out["cond"][q] = float(cond)
        out["coef"][q] = dalpha.astype(np.float64)
        out["max"][q] = (vertex + 4 * u * mx[q]).astype(np.float64)
        out["avg"][q] = (vertex + 4 * u * mx[q] + (M + 2) * u * avg[q]).astype(np.float64)
    return out


def specificity_bound(model, train, alphas, ranks):
    """[n_ranks, S, n_train] on a mean distance: the three coordinates of the sample (instance_bound), the norm (4 u of the distance,
    taken at its largest) and the slab sums ((M + 2) u of the mean)."""
    means, _, _ = specificity(model, train, alphas, ranks)
    T = np.asarray(train, dtype=LD).reshape(-1, 3 * model.M)
    out = np.zeros(means.shape)
    for q, k in enumerate(ranks):
        A = truncated(alphas, k)
        vertex = instance_bound(model, A).sum(axis=2).max(axis=1)                                 # [S]
        largest = vertex_distances(instances(model, A).reshape(A.shape[0], 1, -1), T[None]).max(axis=-1)
        out[q] = (vertex[:, None] + 4 * LD(U) * largest + (model.M + 2) * LD(U) * means[q]).astype(np.float64)
    return out
