"""The restatement behind the device PCA model (tests/pca_restatement.py) against closed forms, and the spread between two correct
routes to the same model -- the figure the GPU tolerances of test_gpu_pca_model.py are set from.  CPU only."""
import numpy as np
import pytest

from scipy.spatial.transform import Rotation

from tests import pca_restatement as pr
from tests.pca_restatement import LOW_RANK, ROUTE_SPREAD, SHAPES, dataset, low_rank_dataset


def test_known_spectrum_comes_back_exactly():
    rng = np.random.default_rng(3)
    lam = np.array([400.0, 90.0, 25.0, 4.0, 0.5])
    ref, shapes, U = pr.known_spectrum_shapes(rng, 120, 9, lam)
    m = pr.pca_model(ref, shapes, relative_tolerance=1e-8)
    assert m.rank == 5
    np.testing.assert_allclose(m.variance, lam, rtol=1e-12)
    np.testing.assert_allclose(np.abs((m.basis * U).sum(axis=0)), 1.0, atol=1e-10)      # eigenvectors up to sign
    np.testing.assert_allclose(m.mean, 0.0, atol=1e-11)                                   # centred coefficients: the mean is the reference
    g = pr.pca_by_gram(ref, shapes, relative_tolerance=1e-8)
    assert g.rank == 5
    np.testing.assert_allclose(g.variance, lam, rtol=1e-12)


def test_kabsch_against_scipy():
    rng = np.random.default_rng(4)
    for trial in range(6):
        x = rng.normal(0, 10, (50, 3))
        Rt, t = pr.random_rigid(rng)
        y = x @ Rt.T + t + rng.normal(0, 0.3, x.shape)
        R, cx, cy = pr.kabsch(x, y)
        ref_rot, _ = Rotation.align_vectors(y - y.mean(axis=0), x - x.mean(axis=0))
        np.testing.assert_allclose(R, ref_rot.as_matrix(), atol=1e-10)
        np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
        np.testing.assert_allclose(cx, x.mean(axis=0))
        np.testing.assert_allclose(cy, y.mean(axis=0))
    # a reflected cloud: still a proper rotation
    x = rng.normal(0, 10, (30, 3))
    R, _, _ = pr.kabsch(x, x * np.array([1.0, 1.0, -1.0]))
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)


def test_kabsch_recovers_an_exact_motion_and_gpa_removes_it():
    rng = np.random.default_rng(5)
    ref, X = dataset(80, 7)
    moved = []
    for x in X:
        R, t = pr.random_rigid(rng)
        moved.append(x @ R.T + t)
    a, b = pr.align_shapes(ref, X, 2), pr.align_shapes(ref, np.stack(moved), 2)
    assert a.sweeps == b.sweeps
    np.testing.assert_allclose(a.shapes, b.shapes, atol=1e-9)
    np.testing.assert_allclose(a.reference, b.reference, atol=1e-9)
    r1 = pr.align_shapes(ref, np.stack(moved), 1)
    for x, y in zip(r1.shapes, X):
        np.testing.assert_allclose(x, pr.align(y, ref), atol=1e-9)


def route_spread(M, n, alignment, data=None):
    ref, X = data if data is not None else dataset(M, n)
    s, g = pr.pca_model(ref, X, alignment), pr.pca_by_gram(ref, X, alignment)
    assert s.rank == g.rank
    lam1 = s.variance[0]
    d_lam = np.abs(s.variance - g.variance).max() / lam1
    P = np.random.default_rng(9).normal(size=(3 * M, 8))
    a, b = s.operator(P), g.operator(P)
    d_op = (np.linalg.norm(a - b, axis=0) / np.linalg.norm(a, axis=0)).max()
    d_mean = np.abs(s.mean - g.mean).max()
    return d_lam, d_op, d_mean


def test_route_spread_svd_against_gram():
    """The SVD of the centred data and the eigen-decomposition of its Gram matrix give the same model; how far apart they land is the
    "route spread".  Printed per case, over every shape of the GPU tests; the largest value is the constant ROUTE_SPREAD of
    pca_restatement.py (the GPU tolerance is 1000 x that), and the assertion below keeps that constant from being too small.  (How
    far below it a run lands depends on the LAPACK build, so there is no lower bound.)"""
    worst = 0.0
    for (M, n) in SHAPES:
        for alignment in (0, 2):
            d_lam, d_op, d_mean = route_spread(M, n, alignment)
            print(f"route spread M={M} n={n} alignment={alignment}: eigenvalues {d_lam:.3e} (of lambda_1), operator {d_op:.3e}, mean {d_mean:.3e}")
            assert d_mean == 0.0                      # (the mean does not depend on the route)
            worst = max(worst, d_lam, d_op)
    for (M, n, r) in LOW_RANK:
        d_lam, d_op, _ = route_spread(M, n, 0, low_rank_dataset(M, n, r))
        print(f"route spread M={M} n={n} rank {r}: eigenvalues {d_lam:.3e} (of lambda_1), operator {d_op:.3e}")
        worst = max(worst, d_lam, d_op)
    print(f"route spread, largest: {worst:.3e}")
    assert worst <= ROUTE_SPREAD, (worst, ROUTE_SPREAD)


def test_rank_rules():
    ref, X = dataset(5, 20)
    m = pr.pca_model(ref, X)
    assert m.rank <= 15                                # 3 M = 15 < n - 1: the tolerance rule sets the rank
    ref, X = dataset(40, 6)
    assert pr.pca_model(ref, X).rank == 5              # n - 1
    assert pr.pca_model(ref, X, max_rank=3).rank == 3
    Xd = np.concatenate([X, X[:2]])                    # exact duplicates add no direction
    assert pr.pca_model(ref, Xd).rank == 5
    with pytest.raises(ValueError):
        pr.pca_model(ref, np.stack([X[0]] * 4))
