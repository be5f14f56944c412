"""CPU side of the Bayesian coherent point drift (gingr_amd/csrc/bcpd.hip): the two routes of its numpy restatement agree on the inputs
the GPU tests use; gingr_amd/csrc/bcpd_math.h, compiled for the host with the address and undefined-behaviour sanitizers into a
stand-alone driver (tests/c/bcpd_math_driver.cpp), gives scipy's digamma and numpy's similarity transform; the restatement's helpers
for the edge tests (chunk planner, blocked assignment, crafted inputs) and the guards those tests rely on; and the C ABI declares and
exports the five gingr_bcpd_* functions."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import digamma

from tests import bcpd_edge_cases as ec
from tests import bcpd_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_bcpd_create", "gingr_bcpd_destroy", "gingr_bcpd_iterate", "gingr_bcpd_get", "gingr_bcpd_set"]


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("g,beta,cut,w", [(6, 1.5, False, 0.1), (7, 1.5, False, 0.1), (7, 1.2, False, 0.1), (7, 1.5, True, 0.1),
                                          (6, 1.5, False, 0.0)])
def test_the_two_routes_agree(g, beta, cut, w):
    y, x = br.grid_case(g, cut=cut)
    p = br.Problem(y, x, w=w, beta=beta, **br.PARAMS)
    assert np.linalg.cond(p.G) <= 1e8                      # a condition on the inputs: the literal route inverts G
    a, b = p.run(40, "woodbury"), p.run(40, "literal")
    for i in range(1, 41):
        assert br.rel(a[i].yhat, b[i].yhat) < 1e-9 and abs(a[i].sigma2 - b[i].sigma2) < 1e-9 * b[i].sigma2, i
        assert np.abs(a[i].sig - b[i].sig).max() < 1e-9 * np.diag(p.G).max() / p.lam, i
    assert 0.7 < a[40].s < 1.1                             # (gamma = 1, lambda = 2 would collapse to s -> 0: the model, not a defect)


def test_full_overlap_runs_reach_rows_without_counterpart():
    """the nu_m -> 0 cases of the GPU tests are what they are said to be"""
    for g, bound in [(6, 1e-300), (7, 1e-8)]:
        y, x = br.grid_case(g)
        p = br.Problem(y, x, w=0.1, beta=1.5, **br.PARAMS)
        assert p.run(40, keep=(40,))[40].nu.min() <= bound


# ---------------------------------------------------------------------------------------------------------- bcpd_math.h
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("bcpd_math") / "bcpd_math_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "bcpd_math_driver.cpp"), "-o", str(exe)])
    return str(exe)


def run(driver, mode, count, payload):
    raw = np.concatenate([[mode, count], np.asarray(payload, float).ravel()]).astype(np.float64).tobytes()
    return np.frombuffer(subprocess.run([driver], input=raw, capture_output=True, check=True).stdout, dtype=np.float64)


def test_digamma_against_scipy(driver):
    rng = np.random.default_rng(0)
    root = 1.4616321449683623
    x = np.concatenate([np.logspace(-3, 7, 4001), rng.uniform(1e-3, 12.0, 4000), root + np.linspace(-1e-2, 1e-2, 401),
                        [1.0, 2.0, 5.999999999999999, 6.0, 6.000000000000001, root]])
    got, want = run(driver, 0, x.size, x), digamma(x)
    err = np.abs(got - want)
    ok = (err <= 1e-13 * np.abs(want)) | (err <= 1e-15)
    assert ok.all(), (x[~ok][:5], got[~ok][:5], want[~ok][:5])
    assert np.isnan(run(driver, 0, 2, [0.0, -1.0])).all() and run(driver, 0, 1, [np.inf])[0] == np.inf


def test_alpha_update(driver):
    nu = np.array([0.0, 1e-12, 0.3, 1.0, 7.5, 300.0])
    M, Nhat, kappa = 6.0, nu.sum(), 1.0
    got = run(driver, 3, nu.size, np.concatenate([[kappa, digamma(kappa * M + Nhat), M], nu]))
    assert np.allclose(got, np.exp(digamma(kappa + nu) - digamma(kappa * M + Nhat)), rtol=1e-13, atol=0)
    assert np.array_equal(run(driver, 3, nu.size, np.concatenate([[np.inf, 0.0, M], nu])), np.full(nu.size, 1.0 / M))


def similarity_cases():
    rng = np.random.default_rng(1)
    out = []
    for kind in ["random"] * 6 + ["rank2"] * 4 + ["reflected"] * 4:
        S = rng.normal(0, 1, (3, 3))
        if kind == "rank2":
            U, d, Vt = np.linalg.svd(S)
            S = U @ np.diag([d[0], d[1], 0.0]) @ Vt
        elif kind == "reflected":
            if np.linalg.det(S) > 0:
                S = S @ np.diag([1.0, 1.0, -1.0])
            assert np.linalg.det(S) < 0
        out.append((kind, S, float(rng.uniform(0.5, 4.0)), rng.normal(0, 3, 3), rng.normal(0, 3, 3)))
    return out


def test_similarity_finish_against_numpy(driver):
    cases = similarity_cases()
    payload, want = [], []
    for kind, S, tr, xbar, ubar in cases:
        Phi, _, Psit = np.linalg.svd(S)
        if kind == "rank2":
            Phi = Phi @ np.diag([1.0, 1.0, -1.0])            # the last column of a rank-2 matrix's Phi is free up to sign
        payload.append(np.concatenate([S.ravel(), Phi.ravel(), Psit.T.ravel(), [tr], xbar, ubar]))
        U, _, Vt = np.linalg.svd(S)
        R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        s = np.trace(R.T @ S) / tr
        want.append(np.concatenate([[s], R.ravel(), xbar - s * R @ ubar]))
    got = run(driver, 1, len(cases), np.concatenate(payload)).reshape(len(cases), 13)
    for (kind, S, *_), g, w in zip(cases, got, want):
        assert np.abs(g - w).max() < 1e-13 * max(1.0, np.abs(w).max()), kind
        R = g[1:10].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1.0) < 1e-13 and np.abs(R @ R.T - np.eye(3)).max() < 1e-13, kind


def test_chunk_planner_covers_the_streamed_cloud(driver):
    sizes = [(1, 1), (1, 3), (65, 1), (216, 194), (343, 308), (1622, 1622), (5000, 5000), (20000, 20000), (32768, 100000), (3, 10 ** 7)]
    got = run(driver, 2, len(sizes), np.array(sizes, float)).reshape(-1, 2)
    for (owners, streamed), (count, length) in zip(sizes, got):
        assert length % 256 == 0 and 1 <= count <= 256
        assert count * length >= streamed > (count - 1) * length        # every chunk holds at least one point


def edge_shapes():
    out = []
    for M, N in list(ec.SIZE_EDGES) + list(ec.MULTI_TILE):
        out += [(N, M), (M, N)]                                          # column pass, row pass
    return out


def test_plan_chunks_restates_the_planner(driver):
    rng = np.random.default_rng(5)
    sizes = edge_shapes() + [(int(o), int(s)) for o, s in zip(rng.integers(1, 40000, 200), rng.integers(1, 300000, 200))]
    sizes += [(int(o), int(s)) for o, s in zip(rng.integers(1, 600, 200), rng.integers(1, 2000, 200))]      # around the tile edges
    got = run(driver, 2, len(sizes), np.array(sizes, float)).reshape(-1, 2)
    for (owners, streamed), (count, length) in zip(sizes, got):
        assert br.plan_chunks(owners, streamed) == (int(count), int(length)), (owners, streamed)


# ------------------------------------------------------------------------------------------- helpers of the edge tests
@pytest.mark.parametrize("g", [6, 7])
def test_blocked_assignment_equals_the_dense_one(g):
    """the summation order differs (slabs of columns), so 1e-13 relative, not bits"""
    y, x = br.grid_case(g)
    p = br.Problem(y, x, w=0.1, beta=1.5, **br.PARAMS)
    assert p.M * p.N <= br.DENSE_LIMIT                                   # the existing cases keep the dense arithmetic
    for it, st in p.run(10, keep=(0, 10)).items():
        dense = p.assignment(st)
        for pairs in (50 * p.M, 97 * p.M, br.SLAB_PAIRS):                # ragged last slab; 97 divides neither N; one slab
            blocked = p.assignment_blocked(st, pairs=pairs)
            assert len(p.slabs(pairs)) == -(-p.N // (pairs // p.M))
            for name, a, b in zip(("nu", "nu_prime", "PX", "xPx"), blocked, dense):
                assert br.rel(a, b) < 1e-13, (g, it, pairs, name)
                assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-13 * np.abs(b).max(), (g, it, pairs, name)


def test_blocked_route_is_taken_past_the_limit_and_agrees_with_the_dense_one(monkeypatch):
    y, x = br.cloud_case(40, 1000, seed=3)
    p = br.Problem(y, x, w=0.1, beta=1.5, **br.PARAMS)
    st = br.crafted_state(p, seed=4)
    dense, dense0 = p.iterate(st), p.initial()
    monkeypatch.setattr(br, "DENSE_LIMIT", 1000)
    monkeypatch.setattr(br, "SLAB_PAIRS", 40 * 300)                       # four slabs, the last ragged
    monkeypatch.setattr(p, "assignment", None)                           # the dense route is not available
    blocked = p.iterate(st)
    for k in ("yhat", "vhat", "nu", "nu_prime", "PX", "alpha", "sig", "sigma2", "s", "R", "t"):
        assert br.rel(getattr(blocked, k), getattr(dense, k)) < 1e-12, k
    assert abs(p.initial().sigma2 - dense0.sigma2) < 1e-13 * dense0.sigma2


def test_crafted_inputs_are_what_they_are_said_to_be():
    R = br.pose_rotation()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    assert np.arccos((np.trace(R) - 1.0) / 2.0) > 1.0 and np.abs(br.POSE_AXIS).min() > 0.3 and br.POSE_S != 1.0 and np.abs(br.POSE_T).min() >= 3.0
    for w in (0.0, 0.1):
        p = ec.cloud_problem(63, 300, w)
        st = ec.cloud_state(63, 300, w, "crafted")
        assert abs(st.alpha.sum() - 1.0) < 1e-14 and st.alpha.min() > 0.0
        assert (st.sig > 0.0).all() and (st.sig < np.diag(p.G) / p.lam).all()
        a = (1.0 - w) * st.alpha * np.exp(-1.5 * st.s ** 2 * st.sig / st.sigma2)
        d2 = ((p.x[None, :, :] - st.yhat[:, None, :]) ** 2).sum(-1)
        den = (a[:, None] * np.exp(-d2 / (2.0 * st.sigma2))).sum(0)
        assert den.min() > 1e-12                                         # no column vanishes: w = 0 stays finite
        assert np.isfinite(ec.cloud_reference(63, 300, w, "crafted").yhat).all()


def test_guards_of_the_edge_tests_hold():
    """every guard tests/test_gpu_bcpd_edges.py asserts before it uses the device, from the restatement alone"""
    for M, N in ec.SIZE_EDGES:
        ec.size_guard(M, N)
    assert ec.chunks(576, 700) == {"col": (3, 256), "row": (3, 256)} and ec.chunks(1025, 300)["col"] == (5, 256)
    for M, N in ec.MULTI_TILE:
        ec.multi_tile_guard(M, N)
    assert br.plan_chunks(64, 65536)[1] == br.TILE                      # one point fewer: one-tile chunks
    assert br.plan_chunks(130816, 513) == (3, 256)                      # one target point fewer: the column pass takes three one-tile chunks
    on = [ec.clamp_guard(which) for which in ec.CLAMP_CASES]
    assert on[0] > br.CLAMP_AT and on[1] > br.CLAMP_AT and on[2] < br.CLAMP_AT
    for name in ec.PARAMETER_CASES:
        ec.parameter_guard(name)
    p, states, refs = ec.offset_case()
    assert np.abs(p.y).min() > 0.9 * ec.OFFSET and all(np.isfinite(r.sigma2) for r in refs.values())


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_abi():
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
    from gingr_amd import _native
    for name in FUNCTIONS:
        assert name in _native.SIGNATURES, name
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
