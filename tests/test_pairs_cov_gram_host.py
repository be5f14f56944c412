"""CPU tests of the dense covariance pairs (gingr_fitter_set_pairs_cov_dense): the numpy restatement
(tests/pairs_cov_gram_restatement.py) against the oracle's two routes, the slab plan of the 3 x 3-weighted Gram pass
(gingr_amd/csrc/gram_cov_plan.h) compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone driver
(tests/c/gram_cov_plan_driver.cpp), normalTangentCovariances, and the two entries in the header, the library and the loader.

Bounds of the restatement against the oracle: rel < 1e-5 on the posterior mean mesh, the bound tests/test_gpu_template_pairs.py holds
its covariance-pair test to (test_covariance_pairs), and the same on the coefficients; the oracle's two routes (compute_posterior_mean
with the pairs as landmarks, PDM.posterior_model on the posed model) are first checked against each other within it."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import pairs_cov_gram_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_fitter_set_pairs_cov_dense", "gingr_fitter_get_pair_precisions"]
EULER, CENTER, TRANSLATION = (0.3, -0.2, 0.1), (4.0, -3.0, 2.0), (1.0, -2.0, 0.5)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def case(layout, seed=0):
    rng = np.random.default_rng(seed)
    M = 120
    ref = rng.normal(0, 30, (M, 3))
    mo = go.build_gaussian_gpmm(ref, 40.0, 20.0, rel_tol=1e-9, max_rank=20)
    if layout == "one-per-vertex":
        pids = rng.permutation(M)
    else:  # repeated, unordered, a third of the vertices without pairs, one vertex with three pairs
        seen = rng.permutation(M)[: 2 * M // 3]
        pids = np.concatenate([seen, rng.choice(seen, 30), [seen[0], seen[0]]])
        pids = pids[rng.permutation(pids.shape[0])]
    K = pids.shape[0]
    truth = mo.instance(rng.normal(0, 0.6, mo.rank)) @ go.euler_to_rot(0.05, -0.04, 0.03).T + np.array([2.0, -1.0, 1.5])
    pts = truth[pids] + rng.normal(0, 0.5, (K, 3))
    covs = pr.normal_tangent(rng.normal(0, 1, (K, 3)), 10.0 ** rng.uniform(-2, 0, K), 10.0 ** rng.uniform(0, 2, K))
    st = go.State(alpha=rng.normal(0, 0.2, mo.rank), euler=EULER, center=np.array(CENTER), translation=np.array(TRANSLATION), scale=1.0,
                  sigma2=1.0, fit=np.zeros((M, 3)), iteration=1)
    st.fit = go.model_instance_shape_pose_scale(mo, st)
    return mo, st, pids.astype(np.int64), pts, covs


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("layout", ["one-per-vertex", "repeated"])
def test_restatement_agrees_with_both_routes_of_the_oracle(layout):
    mo, st, pids, pts, covs = case(layout)
    none = (np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0))
    mesh_a, a_a, posed = go.compute_posterior_mean(mo, st, *none, landmarks=go.Landmarks(pids, pts, covs))
    post = posed.posterior_model(pids, pts, covs)
    mesh_b = post.ref + post.mean
    a_b = np.linalg.lstsq(posed.U * np.sqrt(posed.lam)[None, :], (mesh_b - posed.ref - posed.mean).reshape(-1), rcond=None)[0]
    print(f"{layout}: the oracle's routes, rel(mesh) {rel(mesh_b, mesh_a):.3e}, rel(a) {rel(a_b, a_a):.3e}")
    assert rel(mesh_b, mesh_a) < 1e-5 and rel(a_b, a_a) < 1e-5
    R = st.rotation()
    obs, L, n = pr.consolidate(mo.M, pids, pts, covs)
    assert n.max() == (1 if layout == "one-per-vertex" else n.max()) and (layout == "one-per-vertex" or (n.max() >= 3 and (n == 0).any()))
    W, v = pr.posed_terms(mo, R, st.center, st.translation, obs, L)
    G, rhs = pr.system(pr.model_basis(mo), W, v)
    a, mesh = pr.posterior(mo, R, st.center, st.translation, G, rhs)
    print(f"{layout}: restatement against the oracle, rel(mesh) {rel(mesh, mesh_a):.3e}, rel(a) {rel(a, a_a):.3e}")
    assert rel(mesh, mesh_a) < 1e-5 and rel(a, a_a) < 1e-5
    assert rel(mesh, mesh_b) < 1e-5 and rel(a, a_b) < 1e-5
    assert rel(mesh, st.fit) > 1e-4                                                          # (the observations say something)


def test_consolidation_keeps_a_single_pair_and_leaves_the_rest_zero():
    mo, st, pids, pts, covs = case("repeated", seed=3)
    obs, L, n = pr.consolidate(mo.M, pids, pts, covs)
    one = np.flatnonzero(n == 1)
    where = np.array([np.flatnonzero(pids == i)[0] for i in one])
    assert one.size > 10 and np.array_equal(obs[one], pts[where])
    assert not obs[n == 0].any() and not L[n == 0].any()
    # three pairs on one vertex: the precision-weighted mean solves Lambda x = sum Sigma^-1 x_k
    i = int(np.argmax(n))
    ks = np.flatnonzero(pids == i)
    b = sum(np.linalg.inv(covs[k]) @ pts[k] for k in ks)
    assert n[i] >= 3 and np.allclose(L[i] @ obs[i], b, rtol=1e-9, atol=0)
    # the extended-precision run of the same definition agrees to double rounding, conditioning included
    obs_l, L_l, _ = pr.consolidate(mo.M, pids, pts, covs, dtype=np.longdouble)
    assert rel(pr.prec6(L), pr.prec6(L_l).astype(np.float64)) < 1e-12


# ------------------------------------------------------------------------------------------------------------ the planner
PLAN_CASES = sorted({(M, pr.padded(r)) for r, M in pr.GPU_SHAPES} | {(1, rp) for rp in (16, 112, 128, 512)} |
                    {(10 ** 6, rp) for rp in (16, 112, 128, 512)} | {(50000, 112), (50000, 256)})


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("gram_cov_plan") / "gram_cov_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "gram_cov_plan_driver.cpp"),
                           "-o", str(exe)])
    rows = np.ascontiguousarray(PLAN_CASES, dtype=np.int64)
    flat = np.frombuffer(subprocess.run([str(exe)], input=rows.tobytes(), capture_output=True, check=True).stdout, dtype=np.int64)
    out, at = {}, 0
    for c in PLAN_CASES:
        head = [int(x) for x in flat[at:at + 10]]
        slabs = flat[at + 10:at + 10 + 2 * head[2]].reshape(head[2], 2)
        out[c] = (head, slabs)
        at += 10 + 2 * head[2]
    assert at == flat.size
    return out


def test_slabs_tile_the_vertices_exactly(plans):
    for (M, rp), (head, slabs) in plans.items():
        nbp, npatch, nslabs, vps = head[:4]
        assert (nbp, npatch, nslabs, vps) == pr.plan(M, rp), (M, rp)                        # the restatement's planner is this one
        assert nbp == -(-rp // 64) and npatch == nbp * (nbp + 1) // 2, (M, rp)
        assert nslabs >= 1 and vps % 16 == 0 and int(slabs[0, 0]) == 0 and int(slabs[-1, 1]) == M, (M, rp)
        assert np.array_equal(slabs[1:, 0], slabs[:-1, 1]) and (slabs[:, 1] > slabs[:, 0]).all(), (M, rp)   # no gap, no overlap, none empty
        assert (slabs[:-1, 1] - slabs[:-1, 0] == vps).all() and int(slabs[-1, 1] - slabs[-1, 0]) <= vps, (M, rp)


def test_workspace_covers_every_partial_and_the_reducer_limit_holds(plans):
    for (M, rp), (head, _) in plans.items():
        _, npatch, nslabs, _, stride, partial, factor, ws, max_slabs, instance = head
        assert stride == rp * rp + rp and partial == nslabs * stride and factor == 9 * M and ws == partial + factor, (M, rp)
        assert nslabs <= max_slabs == pr.MAX_SLABS and nslabs * npatch <= max(pr.WANT_WORKGROUPS, npatch), (M, rp)
        assert instance == 0
    assert plans[(10 ** 6, 512)][0][7] * 8 < 1 << 28 and plans[(10 ** 6, 112)][0][7] * 8 < 1 << 28     # below 256 MiB at a million vertices
    assert plans[(65, 16)][0][2] == 2 and plans[(64, 16)][0][2] == 1 and plans[(63, 16)][0][2] == 1    # 65: the first size with two slabs


# ------------------------------------------------------------------------------------------------------------ the helper
def test_normal_tangent_covariances():
    from gingr_amd.registration import normalTangentCovariances
    import gingr_amd.api as api
    assert api.normalTangentCovariances is normalTangentCovariances
    rng = np.random.default_rng(1)
    n = rng.normal(0, 3, (40, 3))
    n[7] = 0.0
    vn, vt = 10.0 ** rng.uniform(-3, 0, 40), 10.0 ** rng.uniform(0, 3, 40)
    C = normalTangentCovariances(n, vn, vt)
    assert C.shape == (40, 3, 3) and np.array_equal(C, np.swapaxes(C, 1, 2))
    assert np.allclose(C, pr.normal_tangent(n, vn, vt), rtol=1e-14, atol=0)
    assert np.array_equal(C[7], vt[7] * np.eye(3))                                           # a zero normal: isotropic
    for k in (0, 1, 39):
        w, V = np.linalg.eigh(C[k])
        assert np.allclose(w, [vn[k], vt[k], vt[k]], rtol=1e-10)                              # eigenvalues: varNormal once, varTangent twice
        assert abs(abs(V[:, 0] @ n[k]) / np.linalg.norm(n[k]) - 1.0) < 1e-10                 # eigenvector of varNormal: the normal
    # scalars and (K,) arrays broadcast; the normals' length does not matter
    assert np.array_equal(normalTangentCovariances(n, 0.01, 100.0), normalTangentCovariances(n, np.full(40, 0.01), np.full(40, 100.0)))
    assert np.allclose(normalTangentCovariances(5.0 * n, vn, 2.0), normalTangentCovariances(n, vn, np.full(40, 2.0)), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        normalTangentCovariances(np.zeros(3), 1.0, 1.0)


def test_covariance_pass_argument():
    import inspect
    from gingr_amd.registration import TemplateRegistration
    assert inspect.signature(TemplateRegistration.__init__).parameters["covariancePass"].default == "landmark"


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert _native.SIGNATURES["gingr_fitter_set_pairs_cov_dense"] == _native.SIGNATURES["gingr_fitter_set_pairs_cov"]
    assert _native.SIGNATURES["gingr_fitter_get_pair_precisions"] == _native.SIGNATURES["gingr_fitter_get_pair_observations"]
