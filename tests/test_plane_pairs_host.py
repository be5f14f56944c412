"""CPU tests of the point-to-plane pairs (gingr_fitter_set_pairs_plane_async / gingr_fitter_update_plane_async): the numpy restatement
(tests/plane_pairs_restatement.py) against the oracle, the closed-form precision against the inverse of normalTangentCovariances, the
sigma2 recursion, the triangle quality the element-wise bound of tests/test_gpu_plane_pairs.py relies on, and the entries in the header,
the library, the loader and the package.

Bounds: the closed form against the np.longdouble inverse of the float64 covariance, per entry 8 u r / v_n -- forming
v_t I + (v_n - v_t) n n^T in float64 rounds at u v_t = u r v_n, which the inverse sees relative to its smallest eigenvalue v_n; the
restatement's posterior mean against the oracle's landmark route rel < 1e-5, the bound tests/test_pairs_cov_gram_host.py holds."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import pairs_cov_gram_restatement as pr
from tests import plane_pairs_restatement as pp
from tests.test_gpu_surface_icp import femur, grid_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["gingr_fitter_set_pairs_plane_async", "gingr_fitter_update_plane_async"]
EULER, CENTER, TRANSLATION = (0.03, -0.02, 0.01), (4.0, -3.0, 2.0), (1.0, -2.0, 0.5)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("ratio", [1.0, 100.0, 1e8])
def test_closed_form_precision_is_the_inverse_of_the_covariance(ratio):
    from gingr_amd.registration import normalTangentCovariances
    rng = np.random.default_rng(int(np.log10(ratio)) + 1)
    n = rng.normal(0, 1, (200, 3))
    n[3] = [0.0, 0.0, 2.0]
    unit = n / np.linalg.norm(n, axis=1)[:, None]
    for v_n in (1e-3, 1.0, 37.5):
        cov = normalTangentCovariances(n, v_n, ratio * v_n)
        want = pr.inverse3(cov.astype(np.longdouble))
        got = pp.closed_form(unit, v_n, ratio)
        err = float(np.abs(got - want).max())
        print(f"ratio {ratio:g} v_n {v_n:g}: worst error / bound {err / (8 * pp.U53 * ratio / v_n):.3e}")
        assert err <= 8 * pp.U53 * ratio / v_n
        assert np.array_equal(got, np.swapaxes(got, 1, 2))
    if ratio == 1.0:                                                                       # isotropic: (1 / sigma2) I, exactly
        assert np.array_equal(pp.closed_form(unit, 0.7, 1.0), np.broadcast_to(np.eye(3) / 0.7, (200, 3, 3)))
    # a zero normal (degenerate triangle): (1 / v_t) I, normalTangentCovariances' rule
    z = pp.closed_form(np.zeros((1, 3)), 2.0, ratio)[0]
    assert np.array_equal(z, np.eye(3) / (ratio * 2.0))
    assert np.allclose(np.linalg.inv(normalTangentCovariances(np.zeros((1, 3)), 2.0, ratio * 2.0)[0]), z, rtol=1e-15, atol=0)


def grid_case(n_template, rank=16):
    tv, tt = grid_mesh(17, 40.0, 6.0, 3)
    sv, sc = grid_mesh(n_template, 34.0, 5.0, 2)
    mo = go.build_gaussian_gpmm(sv, 60.0, 20.0, rel_tol=1e-9, max_rank=rank)
    st = go.State(alpha=np.random.default_rng(n_template).normal(0, 0.2, mo.rank), euler=EULER, center=np.array(CENTER),
                  translation=np.array(TRANSLATION), scale=1.0, sigma2=2.0, fit=np.zeros((mo.M, 3)), iteration=1)
    st.fit = go.model_instance_shape_pose_scale(mo, st)
    return mo, sc, tv, tt, st


@pytest.mark.parametrize("reject", [0, 1])
@pytest.mark.parametrize("n_template", [16, 17])
def test_restatement_agrees_with_the_landmark_route_of_the_oracle(n_template, reject):
    mo, cells, tv, tt, st = grid_case(n_template)
    ratio = 100.0
    cp, w, win, _ = pp.correspondence(st.fit, cells, tv, tt)
    assert 0 < w.sum() < w.shape[0]                                                         # the open target rejects some
    nrm = pp.unit_normals(tv, tt, np.float64)[win]
    obs, L = pp.planes(cp, w, nrm, st.sigma2, ratio, reject)
    pids = np.flatnonzero(w == 1.0) if reject else np.arange(mo.M)
    assert np.array_equal(obs[pids], cp[pids]) and (not reject or (not obs[w == 0].any() and not L[w == 0].any()))
    covs = pp.covariances(nrm, st.sigma2, ratio)
    mesh_o, a_o, _ = go.compute_posterior_mean(mo, st, *pp.NONE_ISO, landmarks=go.Landmarks(pids, cp[pids], covs[pids]))
    R = st.rotation()
    W, v = pr.posed_terms(mo, R, st.center, st.translation, obs, L)
    G, rhs = pr.system(pr.model_basis(mo), W, v)
    a, mesh = pr.posterior(mo, R, st.center, st.translation, G, rhs)
    print(f"{n_template}^2 vertices, reject {reject}: rel(mesh) {rel(mesh, mesh_o):.3e}, rel(a) {rel(a, a_o):.3e}")
    assert rel(mesh, mesh_o) < 1e-5 and rel(a, a_o) < 1e-5 and rel(mesh, st.fit) > 1e-4
    # the whole update: the oracle's route as the GPU tests call it commits, moves the fit and steps sigma2
    nxt, _ = pp.oracle_update(mo, cells, tv, tt, st, ratio, reject, (2.0, 0.5, 10))
    assert nxt.status == 0 and nxt.iteration == 2 and nxt.sigma2 == 2.0 - 0.15 and rel(nxt.fit, st.fit) > 1e-4


def test_sigma2_recursion_is_icps():
    for initial, end, iters in ((100.0, 1.0, 100), (2.0, 0.5, 7), (1.0, 1.0, 3), (0.3, 0.1, 1)):
        s = t = initial
        for _ in range(iters + 3):                                                          # (runs into the floor)
            s, t = pp.schedule(s, initial, end, iters), go.icp_update_sigma2(t, initial, end, iters)
            assert s == t
        assert s == end


def test_triangle_quality_the_gpu_bound_relies_on():
    worst = {}
    for name, (v, t) in (("grid 17", grid_mesh(17, 40.0, 6.0, 3)), ("grid 24", grid_mesh(24, 40.0, 6.0, 1))):
        worst[name] = float(pp.kappa(v, t).max())
        assert worst[name] <= 1.5, worst
    _, _, target, tcells = femur()
    worst["femur"] = float(pp.kappa(target, tcells).max())
    print("largest kappa_t:", worst)
    assert target.shape[0] > 0 and tcells.shape[0] == 3240 and worst["femur"] <= 22.0
    assert np.isinf(pp.kappa(np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]), np.array([[0, 1, 2]]))[0])
    assert not pp.unit_normals(np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]), np.array([[0, 1, 2]])).any()


def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert re.search(r"typedef\s+struct\s+gingr_plane_params\s*\{\s*double\s+tangent_over_normal;\s*int32_t\s+reject;\s*\}", text)
    assert [n for n, _ in _native.PlaneParams._fields_] == ["tangent_over_normal", "reject"]
    assert ctypes.sizeof(_native.PlaneParams) == 16


def test_configuration_and_class_are_part_of_the_package():
    import gingr_amd as ga
    import gingr_amd.api as api
    from gingr_amd.registration import GingrAlgorithm, PointToPlaneIcpRegistration
    assert ga.PointToPlaneIcpRegistration is api.PointToPlaneIcpRegistration is PointToPlaneIcpRegistration
    assert issubclass(PointToPlaneIcpRegistration, GingrAlgorithm)
    cfg = ga.PointToPlaneConfiguration(maxIterations=10, initialSigma=2.0, endSigma=0.5)
    assert cfg.tangentOverNormal == 100.0 and cfg.reject is False and cfg.sigmaStep == 0.15
    assert [f.name for f in dataclasses.fields(cfg)][:5] == ["maxIterations", "initialSigma", "endSigma", "tangentOverNormal", "reject"]
    assert ga.PointToPlaneRegistrationState is api.PointToPlaneRegistrationState
