"""Host-side pieces of the per-vertex covariance maps: the helpers of gingr_amd.helper, the unchanged host path of
GPMMTriangleMesh3D.computeDistanceAbsMesh, and the declarations of the C ABI."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["gingr_model_marginal_covariance", "gingr_model_cross_covariance", "gingr_fitter_posterior_covariance_cpd",
             "gingr_fitter_posterior_covariance_icp", "gingr_fitter_posterior_covariance_icp_surface"]


def random_blocks(M, seed):
    A = np.random.default_rng(seed).normal(0, 1, (M, 3, 4))
    return A @ A.transpose(0, 2, 1)


def test_covariance6_to_matrices():
    from gingr_amd.helper import covariance6_to_matrices
    C = random_blocks(37, 1)
    cov6 = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)
    got = covariance6_to_matrices(cov6)
    assert got.shape == (37, 3, 3) and np.array_equal(got, C)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    assert covariance6_to_matrices(cov6[0]).shape == (1, 3, 3)


def test_posterior_variance_maps():
    from gingr_amd.helper import posteriorVarianceMaps
    C = random_blocks(50, 2)
    cov6 = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)
    n = np.random.default_rng(3).normal(0, 1, (50, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    total, normal = posteriorVarianceMaps(cov6, n)
    want_total = np.array([np.trace(c) for c in C])
    want_normal = np.array([v @ c @ v for c, v in zip(C, n)])
    assert np.abs(total - want_total).max() <= 4 * np.finfo(float).eps * want_total.max()
    assert np.abs(normal - want_normal).max() <= 16 * np.finfo(float).eps * want_total.max()
    assert (normal >= 0).all() and (normal <= total * (1 + 1e-12)).all()        # a direction carries at most the trace
    total2, none = posteriorVarianceMaps(cov6)
    assert none is None and np.array_equal(total2, total)


def test_compute_distance_abs_mesh_host_model_is_unchanged():
    import gingr_amd as ga
    rng = np.random.default_rng(4)
    M, r = 23, 7
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    lam = np.sort(rng.uniform(0.5, 9.0, r))[::-1].copy()
    model = ga.PointDistributionModel(rng.normal(0, 10, (M, 3)), np.zeros((M, 3)), U, lam)
    helper = ga.GPMMTriangleMesh3D.__new__(ga.GPMMTriangleMesh3D)         # the method reads the model only: no context needed
    got = helper.computeDistanceAbsMesh(model, 5)
    # the documented formula: sum_d |cov(lmId, pid)_dd|, cov = U diag(variance) U^T
    cov = (U * lam[None, :]) @ U.T
    want = np.array([sum(abs(cov[3 * 5 + d, 3 * p + d]) for d in range(3)) for p in range(M)])
    assert got.shape == (M,) and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


def test_header_and_prototypes_declare_the_new_names():
    from gingr_amd import _native
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES, name
    assert "scale is NOT applied" in header                                   # the posterior is that of model.transform(rigid)
