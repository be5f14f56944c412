"""CPU pins of the sparse N-ICP step before any kernel runs: tests/nicp_pcg_restatement.py -- the algorithm of
gingr_amd/csrc/nicp_sparse.hip in numpy -- against the oracle's dense stacked least squares (go.nicp_iteration_t / _a, numpy's lstsq)
on the 220-vertex pair of test_gpu_nicp.py, and the component rule that keeps a singular system from being iterated on."""
import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import nicp_pcg_restatement as nr
from tests.test_gpu_nicp import oracle_landmarks, pair, sphere_mesh

GAMMA = 0.7


@pytest.fixture(scope="module")
def case():
    (tv, tt), (gv, gt), lm_t, lm_g = pair()
    ids, ul = oracle_landmarks(tv, gv, lm_t, lm_g)
    edges = go.nicp_edges(tt)
    cp, w, _ = go.surface_correspondence(tv, tt, gv, gt)[:3]
    return tv, tt, gv, gt, ids, ul, edges, cp, w


@pytest.mark.parametrize("alpha", [10.0, 4.0, 1.0])
@pytest.mark.parametrize("kind", ["T", "A"])
def test_restatement_matches_the_stacked_least_squares(case, kind, alpha):
    tv, tt, gv, gt, ids, ul, edges, cp, w = case
    beta = {10.0: 10.0, 4.0: 2.0, 1.0: 0.5}[alpha]            # the (alpha, beta) sequence of test_gpu_nicp.py
    moved, lm, info = nr.step(kind, tv, edges, w, cp, ids, ul, alpha, beta, GAMMA, rel_tol=1e-12)
    if kind == "T":
        want = go.nicp_iteration_t(tv, tt, gv, gt, edges, ids, ul, alpha, beta)[0]
        wlm = want[ids]
    else:
        want, _, wlm = go.nicp_iteration_a(tv, tt, gv, gt, edges, ids, ul, alpha, beta, GAMMA)
    err = np.abs(moved - want).max()
    print(kind, alpha, "iterations", info["iterations"], "max error", err, "true residual", (info["residual"] / info["rhs_norm"]).max())
    assert info["converged"] and info["iterations"] < 2000
    assert err < 1e-7 and np.abs(lm - wlm).max() < 1e-7          # the bound of test_gpu_nicp.py for this comparison


def test_a_column_with_a_zero_right_hand_side_stays_finite():
    """template on the target: U - V = 0, b = 0 -- the recurrence must not divide 0 by 0"""
    tv, tt = sphere_mesh(60, 5)
    edges = go.nicp_edges(tt)
    moved, _, info = nr.step("T", tv, edges, np.ones(60), tv, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), 10.0, 10.0)
    assert info["iterations"] == 0 and info["converged"] and np.array_equal(moved, tv)


def test_component_rule():
    tv, tt = sphere_mesh(40, 3)
    edges = go.nicp_edges(tt)
    none = np.zeros(0, dtype=np.int64)
    # a hull with all-zero weights and no landmark: singular, flagged before anything is solved
    for kind in ("T", "A"):
        with pytest.raises(np.linalg.LinAlgError, match="component"):
            nr.step(kind, tv, edges, np.zeros(40), tv, none, np.zeros((0, 3)), 10.0, 1.0)
    # one weighted vertex anchors it
    w = np.zeros(40)
    w[17] = 1.0
    moved, _, info = nr.step("T", tv, edges, w, tv + 0.5, none, np.zeros((0, 3)), 10.0, 1.0)
    assert info["converged"] and np.abs(moved - (tv + 0.5)).max() < 1e-9       # the whole hull follows its one anchor
    # two disjoint hulls, the second without weight; a landmark TERM anchors a component only where the system has one:
    # N-ICP-T keeps it in the first L columns (the first hull), N-ICP-A at the landmark's vertex
    v2 = np.concatenate([tv, tv + 100.0])
    e2 = np.concatenate([edges, edges + 40])
    w2 = np.concatenate([np.ones(40), np.zeros(40)])
    comp = nr.graph(80, e2)[3]
    assert np.array_equal(comp, np.repeat([0, 1], 40))
    lm, ul = np.array([55]), v2[[55]] + 1.0
    for kind, beta, singular in (("T", 1.0, True), ("A", 1.0, False), ("A", 0.0, True)):
        _, _, has = nr.host_terms(kind, v2, w2, v2, lm, ul, beta)
        assert (nr.unanchored_component(comp, has) == 1) == singular, (kind, beta)
    # an isolated vertex is a component of its own
    comp = nr.graph(41, edges)[3]
    assert comp[40] == 1 and nr.unanchored_component(comp, np.concatenate([np.ones(40), [0.0]])) == 1
