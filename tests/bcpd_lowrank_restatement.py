"""numpy restatement of the low-rank deformation step of the Bayesian coherent point drift (gingr_amd/csrc/bcpd_lowrank.hip) on top of
tests/bcpd_restatement.py.  With G ~ L L^T (L: M x k), K = L L^T / lambda, c2 = s^2 / sigma2 and r as the dense step forms it,
Sigma = K - K D^1/2 (I + D^1/2 K D^1/2)^-1 D^1/2 K (D = c2 diag nu) is, by the push-through identity, L C^-1 L^T / lambda:

    S = L^T diag(nu) L     s = L^T r     C = I + (c2 / lambda) S = R R^T     z = C^-1 s
    vhat = (c2 / lambda) L z             sigma_m^2 = |R^-1 l_m|^2 / lambda   (l_m: row m of L)

Nothing of size M x M is formed.  Not a test module (no test_ prefix): tests/test_bcpd_lowrank_host.py checks it against
bcpd_restatement.Problem over G := L L^T on the CPU, tests/test_gpu_bcpd_lowrank.py uses it as the host side of its comparisons."""
import numpy as np
from scipy.linalg import solve_triangular

from tests import bcpd_restatement as br


def deformation_lowrank(problem, st, nu, PX, L):
    """(vhat, sigma_m^2) of step 2 by the k-space formulas above"""
    lam = problem.lam
    c2 = st.s ** 2 / st.sigma2
    r = (PX - nu[:, None] * st.t[None, :]) @ st.R / st.s - nu[:, None] * problem.y
    S = L.T @ (nu[:, None] * L)
    C = np.eye(L.shape[1]) + (c2 / lam) * S
    Rc = np.linalg.cholesky(C)
    w = solve_triangular(Rc, L.T @ r, lower=True)                 # R^-1 s
    z = solve_triangular(Rc.T, w, lower=False)                    # C^-1 s
    T = solve_triangular(Rc, L.T, lower=True)                     # column m: R^-1 l_m
    return (c2 / lam) * (L @ z), (T ** 2).sum(0) / lam


class Problem(br.Problem):
    """bcpd_restatement.Problem with G replaced by L L^T.  `deformation(route="woodbury")` uses K = G / lambda alone, so it works with
    a singular G; route "lowrank" is `deformation_lowrank` and needs no G.  dense=False never forms G (templates past the dense limit:
    only the route "lowrank" and the slab form of the assignment run then)."""

    def __init__(self, y, x, L, w=0.0, lambda_=2.0, gamma=1.0, kappa=1.0, beta=2.0, dense=True):
        self.y, self.x, self.L = np.asarray(y, float), np.asarray(x, float), np.asarray(L, float)
        self.M, self.N = self.y.shape[0], self.x.shape[0]
        self.w, self.lam, self.gamma, self.kappa, self.beta = w, lambda_, gamma, kappa, beta
        self.G = self.L @ self.L.T if dense else None
        self.kmax = float((self.L ** 2).sum(1).max() / lambda_)   # max_m K_mm
        self.p_out = 1.0 / float(np.prod(self.x.max(0) - self.x.min(0))) if w > 0 else 0.0

    def deformation(self, st, nu, PX, route):
        if route == "lowrank":
            return deformation_lowrank(self, st, nu, PX, self.L)
        return super().deformation(st, nu, PX, route)
