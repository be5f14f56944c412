"""numpy restatement of this package's Bayesian coherent point drift (Hirose 2020, Fig. 4; DESIGN.md section 5 lists where it leaves
the reference's draft cpd/BCPD.scala).  Two routes through the deformation step that must agree wherever G is invertible:

    literal    Sigma = pinv(lambda pinv(G) + c2 diag nu), P formed densely
    woodbury   Sigma = K - K D^1/2 A^-1 D^1/2 K with K = G / lambda, D = c2 diag nu, A = I + D^1/2 K D^1/2 (what the device does)

State: (yhat, sig = diag Sigma, s, R, t, sigma2, alpha).  `iterate` returns the new state and the by-products the C ABI exposes.

Past DENSE_LIMIT pairs the soft assignment and the initial variance go by slabs of target points (a slab of columns is complete for
den_n), so nothing of size M x N is kept; below it the dense arithmetic is what it always was.  The last part restates the device's
bookkeeping (chunk planner, padding, clamp condition) and builds the inputs of the edge tests (tests/test_gpu_bcpd_edges.py)."""
from dataclasses import dataclass, replace

import numpy as np
from scipy.special import digamma

D = 3
DENSE_LIMIT = 1 << 21      # M N above which `iterate` and `initial` go by slabs (the grid cases stay below: 343 x 308 = 1.1e5)
SLAB_PAIRS = 1 << 21       # pairs to a slab


@dataclass
class State:
    yhat: np.ndarray
    sig: np.ndarray
    alpha: np.ndarray
    s: float
    R: np.ndarray
    t: np.ndarray
    sigma2: float
    # by-products of the iteration that produced this state (None at the start)
    vhat: np.ndarray = None
    nu: np.ndarray = None
    nu_prime: np.ndarray = None
    PX: np.ndarray = None
    Nhat: float = None
    sigma_bar2: float = None

    def copy(self):
        return replace(self, **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})


class Problem:
    def __init__(self, y, x, w=0.0, lambda_=2.0, gamma=1.0, kappa=1.0, beta=2.0):
        self.y, self.x = np.asarray(y, float), np.asarray(x, float)
        self.M, self.N = self.y.shape[0], self.x.shape[0]
        self.w, self.lam, self.gamma, self.kappa, self.beta = w, lambda_, gamma, kappa, beta
        d2 = ((self.y[:, None, :] - self.y[None, :, :]) ** 2).sum(-1)
        self.G = np.exp(-d2 / (2.0 * beta * beta))
        ext = self.x.max(0) - self.x.min(0)
        V = float(np.prod(ext))
        self.p_out = 1.0 / V if w > 0 else 0.0

    def slabs(self, pairs=None):
        """slices of the target points, about `pairs` (SLAB_PAIRS) pairs to a slab"""
        step = max(1, (pairs or SLAB_PAIRS) // self.M)
        return [slice(n0, min(n0 + step, self.N)) for n0 in range(0, self.N, step)]

    def initial(self) -> State:
        if self.M * self.N > DENSE_LIMIT:
            tot = sum(float(((self.x[None, sl, :] - self.y[:, None, :]) ** 2).sum()) for sl in self.slabs())
        else:
            tot = ((self.x[None, :, :] - self.y[:, None, :]) ** 2).sum()
        return State(self.y.copy(), np.ones(self.M), np.full(self.M, 1.0 / self.M), 1.0, np.eye(3), np.zeros(3),
                     self.gamma * tot / (D * self.N * self.M))

    # -- step 1 ---------------------------------------------------------------------------------------------------
    def assignment(self, st: State):
        a = (1.0 - self.w) * st.alpha * np.exp(-1.5 * st.s ** 2 * st.sig / st.sigma2)
        d2 = ((self.x[None, :, :] - st.yhat[:, None, :]) ** 2).sum(-1)           # M x N
        e = np.exp(-d2 / (2.0 * st.sigma2))
        c = self.w * self.p_out * (2.0 * np.pi * st.sigma2) ** 1.5
        den = (a[:, None] * e).sum(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            P = a[:, None] * e / (den + c)[None, :]
        nu, nu_prime = P.sum(1), P.sum(0)
        return nu, nu_prime, P @ self.x, float((nu_prime * (self.x ** 2).sum(1)).sum())

    def assignment_blocked(self, st: State, pairs=None):
        """`assignment` one slab of target points at a time: nu' of the slab, and the slab's share of nu, PX and xPx"""
        a = (1.0 - self.w) * st.alpha * np.exp(-1.5 * st.s ** 2 * st.sig / st.sigma2)
        c = self.w * self.p_out * (2.0 * np.pi * st.sigma2) ** 1.5
        nu, PX, nu_prime, xPx = np.zeros(self.M), np.zeros((self.M, D)), np.empty(self.N), 0.0
        for sl in self.slabs(pairs):
            xs = self.x[sl]
            P = np.subtract.outer(st.yhat[:, 0], xs[:, 0]) ** 2                      # M x slab, reused for d2, e, a e and P
            for d in (1, 2):
                P += np.subtract.outer(st.yhat[:, d], xs[:, d]) ** 2
            P /= -2.0 * st.sigma2
            np.exp(P, out=P)
            P *= a[:, None]
            den = P.sum(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                P /= (den + c)[None, :]
            nu_prime[sl] = P.sum(0)
            nu += P.sum(1)
            PX += P @ xs
            xPx += float((nu_prime[sl] * (xs ** 2).sum(1)).sum())
        return nu, nu_prime, PX, xPx

    # -- step 2 ---------------------------------------------------------------------------------------------------
    def deformation(self, st: State, nu, PX, route):
        c2 = st.s ** 2 / st.sigma2
        r = (PX - nu[:, None] * st.t[None, :]) @ st.R / st.s - nu[:, None] * self.y      # row m: (1/s) R^T (PX_m - nu_m t) - nu_m y_m
        if route == "literal":
            Sigma = np.linalg.pinv(self.lam * np.linalg.pinv(self.G, hermitian=True) + c2 * np.diag(nu), hermitian=True)
            vhat = c2 * Sigma @ r
            sig = np.diag(Sigma).copy()
        else:
            K = self.G / self.lam
            dh = np.sqrt(c2 * nu)
            A = np.eye(self.M) + dh[:, None] * K * dh[None, :]
            L = np.linalg.cholesky(A)
            z = K @ r
            q = np.linalg.solve(A, dh[:, None] * z)
            vhat = c2 * (z - K @ (dh[:, None] * q))
            Wm = np.linalg.solve(L, dh[:, None] * K)                                      # L^-1 D^1/2 K
            sig = np.diag(K) - (Wm ** 2).sum(0)
        return vhat, sig

    # -- steps 3 and 4 --------------------------------------------------------------------------------------------
    def similarity(self, nu, PX, u, sig):
        Nhat = nu.sum()
        xbar, ubar = PX.sum(0) / Nhat, (nu[:, None] * u).sum(0) / Nhat
        sbar2 = float((nu * sig).sum() / Nhat)
        uc = u - ubar[None, :]
        Sxu = (PX - nu[:, None] * xbar[None, :]).T @ uc / Nhat
        trSuu = float((nu * (uc ** 2).sum(1)).sum() / Nhat + D * sbar2)
        Phi, _, Psit = np.linalg.svd(Sxu)
        R = Phi @ np.diag([1.0, 1.0, np.linalg.det(Phi @ Psit)]) @ Psit
        s = float(np.trace(R.T @ Sxu) / trSuu)
        t = xbar - s * R @ ubar
        return float(Nhat), sbar2, s, R, t

    def iterate(self, st: State, route="woodbury") -> State:
        nu, nu_prime, PX, xPx = self.assignment_blocked(st) if self.M * self.N > DENSE_LIMIT else self.assignment(st)
        vhat, sig = self.deformation(st, nu, PX, route)
        u = self.y + vhat
        Nhat, sbar2, s, R, t = self.similarity(nu, PX, u, sig)
        if np.isinf(self.kappa):
            alpha = np.full(self.M, 1.0 / self.M)
        else:
            alpha = np.exp(digamma(self.kappa + nu) - digamma(self.kappa * self.M + Nhat))
        yhat = s * u @ R.T + t[None, :]
        sigma2 = (xPx - 2.0 * (PX * yhat).sum() + (nu * (yhat ** 2).sum(1)).sum()) / (Nhat * D) + s * s * sbar2
        return State(yhat, sig, alpha, s, R, t, float(sigma2), vhat, nu, nu_prime, PX, Nhat, sbar2)

    def run(self, iterations, route="woodbury", keep=()):
        """the states after 0 .. `iterations` iterations; `keep`: the iteration counts to return (all when empty)"""
        st = self.initial()
        out = {0: st}
        for i in range(1, iterations + 1):
            st = self.iterate(st, route)
            if not keep or i in keep:
                out[i] = st
        return out

    def registration(self, max_iteration, tolerance=1e-6, route="woodbury"):
        """the reference's loop (BCPD.Registration): stop when |sigma2' - sigma2| < tolerance; returns (state, iterations, converged)"""
        st, i, converged = self.initial(), 0, False
        while i < max_iteration and not converged:
            new = self.iterate(st, route)
            if abs(new.sigma2 - st.sigma2) < tolerance:
                converged = True
            else:
                i += 1
            st = new
        return st, i, converged


# ---------------------------------------------------------------------------------------------------- the tests' inputs
def grid_case(g, seed=0, cut=False, fraction=0.9):
    """template: the integer grid g^3 plus N(0, 0.25^2) jitter; target: the template warped, scaled 1.1, rotated 0.2 rad about z,
    shifted, 90 % of the points in random order, optionally cut to x < mean + 0.3, plus N(0, 0.02^2) noise"""
    rng = np.random.default_rng(seed)
    ax = np.arange(g, dtype=float)
    y = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + rng.normal(0, 0.25, (g ** 3, 3))
    warped = y + 0.3 * np.sin(0.7 * y[:, (1, 2, 0)])
    c, s = np.cos(0.2), np.sin(0.2)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    x = 1.1 * warped @ Rz.T + np.array([0.5, -0.3, 0.2])
    x = x[rng.permutation(x.shape[0])[: int(fraction * x.shape[0])]]
    if cut:
        x = x[x[:, 0] < x[:, 0].mean() + 0.3]
    x = x + rng.normal(0, 0.02, x.shape)
    return y, x


PARAMS = dict(lambda_=10.0, gamma=0.3, kappa=1.0)


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ------------------------------------------------------------------------------- the device's bookkeeping, restated
TILE, TARGET_GROUPS, MAX_CHUNKS, PANEL = 256, 1024, 256, 64
CLAMP_AT = 2.0 ** 41


def plan_chunks(owners, streamed):
    """bcpd_plan_chunks (gingr_amd/csrc/bcpd_math.h): (count, length) of the chunks of the streamed cloud of a pair pass; the column
    pass is plan_chunks(N, M), the row pass plan_chunks(M, N)"""
    groups, tiles = -(-owners // TILE), -(-streamed // TILE)
    want = max(1, min(-(-TARGET_GROUPS // groups), tiles, MAX_CHUNKS))
    length = -(-tiles // want) * TILE
    return -(-streamed // length), length


def padded(M):
    """(Mp, padded rows, 64-row blocks) of the M-sized kernels"""
    Mp = -(-M // PANEL) * PANEL
    return Mp, Mp - M, Mp // PANEL


def clamp_figure(x, yhat, sigma2):
    """what the pair passes hold against CLAMP_AT: 3 am^2 . 2048 log2(e) / (2 sigma2), am the largest |coordinate| of x about the
    centroid of x plus that of yhat about the same centroid; at or above CLAMP_AT the clamped copy of the inner loops runs"""
    c = x.mean(0)
    am = float(np.abs(x - c).max() + np.abs(yhat - c).max())
    return 3.0 * am * am * 2048.0 * np.log2(np.e) / (2.0 * sigma2)


# ------------------------------------------------------------------------------------------- the edge tests' inputs
POSE_S, POSE_ANGLE, POSE_AXIS, POSE_T = 1.3, 1.3, np.array([1.0, 2.0, -2.0]) / 3.0, np.array([3.0, -4.0, 5.0])
CLOUD_NOISE = 0.3


def pose_rotation():
    """POSE_ANGLE rad about POSE_AXIS (Rodrigues)"""
    k = POSE_AXIS
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(POSE_ANGLE) * Kx + (1.0 - np.cos(POSE_ANGLE)) * Kx @ Kx


def cloud_case(M, N, seed):
    """template: M points uniform in a cube of side 8; target: N points, each the posed image s R y_m + t of a template point chosen
    at random plus N(0, 0.3^2) -- under the pose of `crafted_state` every column has a template point within the noise"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-4.0, 4.0, (M, 3))
    x = POSE_S * y[rng.integers(0, M, N)] @ pose_rotation().T + POSE_T + rng.normal(0, CLOUD_NOISE, (N, 3))
    return y, x


def crafted_state(p, seed):
    """a state that needs no preceding iterations: yhat = s R y + t + N(0, 0.05^2) for a similarity well away from the identity,
    sigma_m^2 random in (0, K_mm), <alpha> a random point of the simplex, sigma2 = 0.1 (the target's noise is 0.3^2 = 0.09)"""
    rng = np.random.default_rng(seed)
    R = pose_rotation()
    yhat = POSE_S * p.y @ R.T + POSE_T + rng.normal(0, 0.05, (p.M, 3))
    sig = rng.uniform(0.02, 0.98, p.M) * np.diag(p.G) / p.lam
    return State(yhat, sig, rng.dirichlet(np.ones(p.M)), POSE_S, R, POSE_T.copy(), 0.1)
