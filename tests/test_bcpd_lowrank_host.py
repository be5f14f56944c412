"""CPU test of the low-rank deformation step of the Bayesian coherent point drift: the k-space restatement
(tests/bcpd_lowrank_restatement.py) against the Woodbury route of tests/bcpd_restatement.py over G := L L^T, with factors from the
oracle's pivoted Cholesky.  The two differ by rounding alone: vhat to 1e-12 relative, sigma_m^2 to 1e-12 max K_mm absolute (measured:
1.3e-15 and 2.8e-15 at worst)."""
import functools

import numpy as np
import pytest

from tests import bcpd_lowrank_restatement as blr
from tests import bcpd_restatement as br
from tests import lowrank_cpd_restatement as lr

W_OUTLIER = 0.05
PAIRS = {"g6": 1.5, "g7": 1.5, "hull": 25.0, "pair": 10.0}           # name -> beta
FACTORS = [(1e-2, 0), (1e-4, 0), (1e-8, 0), (1e-8, 1)]               # (tolerance, maxColumns): the last is a single column


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "g6":
        return br.grid_case(6)
    if name == "g7":
        return br.grid_case(7)
    if name == "hull":
        return lr.hull(1500, 1125)
    return lr.pair(500, 420, 507, noise=0.3)


@pytest.mark.parametrize("tol,max_columns", FACTORS)
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_k_space_step_is_the_woodbury_step_over_the_factor(name, tol, max_columns):
    """Four iterations, each from the state the Woodbury route over L L^T left."""
    y, x = inputs(name)
    L = lr.factor(y, PAIRS[name], tol, max_columns)
    assert L.shape[1] == 1 if max_columns == 1 else 1 < L.shape[1] <= y.shape[0]
    p = blr.Problem(y, x, L, w=W_OUTLIER, beta=PAIRS[name], **br.PARAMS)
    st = p.initial()
    for it in range(4):
        nu, _, PX, _ = p.assignment(st)
        v_w, sig_w = p.deformation(st, nu, PX, "woodbury")
        v_k, sig_k = blr.deformation_lowrank(p, st, nu, PX, L)
        figures = (br.rel(v_k, v_w), float(np.abs(sig_k - sig_w).max() / p.kmax))
        print(f"{name} k {L.shape[1]} iteration {it}: vhat {figures[0]:.1e} sigma_m^2 {figures[1]:.1e} of max K_mm")
        assert figures[0] <= 1e-12 and figures[1] <= 1e-12, (it, figures)
        assert sig_k.min() >= 0.0
        st = p.iterate(st, "woodbury")


def test_route_lowrank_needs_no_dense_matrix():
    y, x = inputs("g6")
    L = lr.factor(y, 1.5, 1e-4)
    dense = blr.Problem(y, x, L, w=W_OUTLIER, beta=1.5, **br.PARAMS)
    slim = blr.Problem(y, x, L, w=W_OUTLIER, beta=1.5, dense=False, **br.PARAMS)
    assert slim.G is None
    a, b = dense.iterate(dense.initial(), "woodbury"), slim.iterate(slim.initial(), "lowrank")
    assert br.rel(b.yhat, a.yhat) < 1e-12 and abs(b.sigma2 - a.sigma2) < 1e-12 * a.sigma2
