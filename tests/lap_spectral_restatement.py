"""Dense numpy restatement of gingr_model_from_laplacian (include/gingr_hip.h; gingr_amd/csrc/lap_spectral.hip and
lap_spectral_plan.h): the same deflation, start block, degree rule, scaled Chebyshev recurrence, Cholesky-QR twice, Rayleigh-Ritz and
stop rule, in the same order, on a dense Laplacian.  Sums run in numpy's order, so results agree with the device to rounding, not to
the bit.  Shared by tests/test_laplacian_model_host.py (against numpy.linalg.eigh, and the plan header's driver against the plan
functions here) and tests/test_gpu_laplacian_model.py (the meshes and the expected models)."""
import dataclasses
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAX_PAIRS, MAX_BLOCK, MIN_GUARD = 170, 192, 8
CUTOFF = 1e-5
DEFAULT_TOLERANCE = 1e-10
SPREAD_BOUND = 1e6
MAX_STEP_DEGREE = 512
DEFAULT_MAX_DEGREE = 4000


class LaplacianError(ValueError):
    pass


class NotConverged(RuntimeError):
    def __init__(self, text, info):
        super().__init__(text)
        self.info = info


# ---------------------------------------------------------------------------------------------------------------- meshes
def femur_full():
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    m = np.load(os.path.join(HERE, "golden", "femur_mesh.npz"))
    return d["femur"].astype(np.float64), np.ascontiguousarray(m["femur_cells"], dtype=np.int32)


def femur_small(n=220):
    from gingr_amd.simple import cluster_decimate
    v, c = femur_full()
    v, c = cluster_decimate(v, c, n)
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(c, dtype=np.int32)


def doubled_with_isolated(v, c):
    """two copies of a mesh (the second shifted) and one vertex no cell names, between them"""
    n = v.shape[0]
    shift = np.array([2.5 * (v[:, 0].max() - v[:, 0].min()), 0.0, 0.0])
    lone = v.mean(axis=0) + 0.5 * shift
    return (np.concatenate([v, lone[None, :], v + shift]), np.ascontiguousarray(np.concatenate([c, c + n + 1]), dtype=np.int32))


def strip(N):
    """a flat band of 2 x N vertices and 2 (N - 1) triangles: the most elongated mesh there is; from N ~ 1 100 on its smallest non-zero
    eigenvalue (~ 12.3 / N^2) lies below the 1e-5 cut-off"""
    v = np.array([[float(i), float(r), 0.0] for i in range(N) for r in range(2)])
    i = 2 * np.arange(N - 1, dtype=np.int32)
    c = np.concatenate([np.stack([i, i + 2, i + 1], axis=1), np.stack([i + 1, i + 2, i + 3], axis=1)])
    return v, np.ascontiguousarray(c, dtype=np.int32)


def tetrahedron():
    v = np.array([[0.0, 0, 0], [10.0, 0, 0], [0, 10.0, 0], [0, 0, 10.0]])
    return v, np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- plan (lap_spectral_plan.h)
def edges_from_cells(n, cells):
    """unique undirected edges p1 < p2, ascending; no loops"""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    if c.shape[0] < 1:
        raise LaplacianError("no cells")
    if c.min() < 0 or c.max() >= n:
        raise LaplacianError("cell index outside the mesh")
    e = np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.sort(e, axis=1), axis=0)
    return e.astype(np.int32).reshape(-1, 2)


def laplacian(n, cells):
    e = edges_from_cells(n, cells)
    L = np.zeros((n, n))
    L[e[:, 0], e[:, 1]] = -1.0
    L[e[:, 1], e[:, 0]] = -1.0
    L[np.arange(n), np.arange(n)] = -L.sum(axis=1)
    return L


def components(L):
    """labels numbered by each component's lowest vertex (nicp_graph.h)"""
    n = L.shape[0]
    lab = np.full(n, -1, dtype=np.int64)
    k = 0
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = k
        stack = [s]
        while stack:
            i = stack.pop()
            for j in np.nonzero(L[i] < 0)[0]:
                if lab[j] < 0:
                    lab[j] = k
                    stack.append(int(j))
        k += 1
    return lab, k


def block_plan(k, dim):
    m = min(MAX_BLOCK, (k + MIN_GUARD + 15) // 16 * 16)
    return m, int(min(m, dim))


@dataclasses.dataclass
class Filter:
    a: float
    bound: float
    c: float
    e: float
    sigma1: float
    degree: int


def filter_plan(theta_max, bound, max_degree):
    a = min(max(theta_max, 1e-12 * bound), 0.95 * bound)
    c, e = 0.5 * (bound + a), 0.5 * (bound - a)
    d = math.floor(math.acosh(SPREAD_BOUND) / math.acosh(c / e))
    return Filter(a, bound, c, e, -e / c, int(min(max(d, 1), min(max_degree, MAX_STEP_DEGREE))))


def filter_spread(f, degree):
    return math.cosh(degree * math.acosh(f.c / f.e))


def recurrence_steps(f):
    """[(alpha, beta, gamma)] of T_next = alpha L T_cur + beta T_cur + gamma T_prev, steps 1 .. degree"""
    out, sigma = [], f.sigma1
    out.append((f.sigma1 / f.e, -f.sigma1 * f.c / f.e, 0.0))
    for _ in range(2, f.degree + 1):
        nxt = 1.0 / (2.0 / f.sigma1 - sigma)
        out.append((2.0 * nxt / f.e, -2.0 * nxt * f.c / f.e, -sigma * nxt))
        sigma = nxt
    return out


def start_block(n, m, active):
    """the counter hash of lap_start_kernel: splitmix64 of (vertex, column) mapped to [-1, 1)"""
    i = np.arange(n, dtype=np.uint64)[:, None]
    c = np.arange(m, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = i * np.uint64(0x9E3779B97F4A7C15) + (c + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    X = (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -52) - 1.0
    X[:, active:] = 0.0
    return X


# ---------------------------------------------------------------------------------------------------------------- iteration
@dataclasses.dataclass
class Info:
    n_components: int = 0
    n_dropped: int = 0
    block_columns: int = 0
    outer_iterations: int = 0
    total_degree: int = 0
    converged: int = 0
    max_residual: float = 0.0
    cut_gap: float = 0.0


def _deflate(X, lab, ncomp):
    for q in range(ncomp):
        rows = lab == q
        X[rows] -= X[rows].sum(axis=0) / rows.sum()
    return X


def _cholesky_qr(X, active):
    G = X[:, :active].T @ X[:, :active]
    R = np.linalg.cholesky(G)                       # G = R R^T
    X[:, :active] = np.linalg.solve(R, X[:, :active].T).T   # X R^-T
    return X


def solve(L, k, tolerance=None, max_degree=None):
    """(theta [k], V [n][k], info): the k smallest eigenpairs above the cut-off, signs fixed; raises like the C ABI refuses"""
    n = L.shape[0]
    tol = DEFAULT_TOLERANCE if tolerance is None or tolerance <= 0 else tolerance
    budget = DEFAULT_MAX_DEGREE if max_degree is None or max_degree <= 0 else max_degree
    if k < 1 or k > MAX_PAIRS:
        raise LaplacianError("k out of range")
    lab, ncomp = components(L)
    dim = n - ncomp
    info = Info(n_components=ncomp, n_dropped=ncomp)
    if k > dim:
        raise LaplacianError("k larger than the number of eigenvalues above the cut-off")
    bound = 2.0 * float(np.diag(L).max())
    m, active = block_plan(k, dim)
    info.block_columns = m
    X = _cholesky_qr(_cholesky_qr(_deflate(start_block(n, m, active), lab, ncomp), active), active)
    wanted = k
    while True:
        if info.total_degree + 2 > budget:
            raise NotConverged("degree budget", info)
        LX = L @ X
        H = X[:, :active].T @ LX[:, :active]
        theta, V = np.linalg.eigh(0.5 * (H + H.T))
        X[:, :active] = X[:, :active] @ V
        LX = L @ X
        info.total_degree += 2
        res = np.linalg.norm(LX[:, :active] - X[:, :active] * theta[None, :], axis=0) / bound
        info.max_residual = float(res[:wanted].max())
        if np.all(res[:wanted] <= tol):
            t = int(np.sum(theta[:wanted] <= CUTOFF))
            if k + t > dim:
                raise LaplacianError("k larger than the number of eigenvalues above the cut-off")
            if k + t <= wanted:
                break
            wanted = k + t
            if wanted > active - (1 if active < dim else 0):
                raise LaplacianError("too many eigenvalues below the cut-off for one block")
            continue
        left = budget - info.total_degree - 2
        if left < 1:
            raise NotConverged("degree budget", info)
        f = filter_plan(float(theta[-1]), bound, left)
        prev, cur = None, X
        for alpha, beta, gamma in recurrence_steps(f):
            nxt = alpha * (L @ cur) + beta * cur + (gamma * prev if prev is not None else 0.0)
            prev, cur = cur, nxt
        info.total_degree += f.degree
        info.outer_iterations += 1
        X = _cholesky_qr(_cholesky_qr(_deflate(cur, lab, ncomp), active), active)
    t = wanted - k
    info.n_dropped = ncomp + t
    info.converged = 1
    th = theta[t:t + k]
    info.cut_gap = float((theta[t + k] - th[-1]) / th[-1]) if t + k < active else math.inf
    Vk = X[:, t:t + k].copy()
    for j in range(k):                                    # the component of largest magnitude positive, lowest index on a tie
        if Vk[np.argmax(np.abs(Vk[:, j])), j] < 0:
            Vk[:, j] = -Vk[:, j]
    return th, Vk, info


# ---------------------------------------------------------------------------------------------------------------- expected models
@dataclasses.dataclass
class Model:
    rank: int
    lam: np.ndarray
    U: np.ndarray


def expand(theta, V, scaling):
    """the rank-3k model of k pairs: variance scaling / mu_j three times, v_j on one coordinate each"""
    n, k = V.shape
    U = np.zeros((3 * n, 3 * k))
    for d in range(3):
        U[d::3, d::3] = V
    return Model(3 * k, np.repeat(scaling / theta, 3), U)


def eigh_model(L, k, scaling):
    """the definition, by the dense eigen-decomposition: the k smallest eigenpairs above the cut-off"""
    mu, V = np.linalg.eigh(L)
    keep = np.nonzero(mu > CUTOFF)[0][:k]
    if keep.shape[0] < k:
        raise LaplacianError("k larger than the number of eigenvalues above the cut-off")
    return expand(mu[keep], V[:, keep], scaling), mu
