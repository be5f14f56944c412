"""CPU pins of the sparse inverse-Laplacian model build (gingr_model_from_laplacian).

1. tests/lap_spectral_restatement.py -- the iteration restated in numpy, same steps in the same order -- against numpy.linalg.eigh on
   the cases of the fixture table, at the bounds the device tests use (variances 1e-8 relative in norm, |U^T U - I| < 1e-9, covariance
   on 300 random rows 1e-8 of its largest entry), and its count of block products against the default budget.
2. gingr_amd/csrc/lap_spectral_plan.h compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone
   driver (tests/c/lap_spectral_plan_driver.cpp): edge lists, block widths, filter plans and recurrence coefficients are those of the
   restatement.
3. The C ABI, the ctypes binding and the Python entry points name the new call."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lap_spectral_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

_cache = {}


def mesh(name):
    if name not in _cache:
        v, c = {"femur": rs.femur_full, "small": rs.femur_small, "tetra": rs.tetrahedron,
                "doubled": lambda: rs.doubled_with_isolated(*rs.femur_small())}[name]()
        _cache[name] = (v, c, rs.laplacian(v.shape[0], c))
    return _cache[name]


def check(got, want):
    assert got.rank == want.rank
    assert np.linalg.norm(got.lam - want.lam) < 1e-8 * np.linalg.norm(want.lam)
    assert np.abs(got.U.T @ got.U - np.eye(got.rank)).max() < 1e-9
    rows = np.random.default_rng(0).permutation(got.U.shape[0])[:300]
    A, B = got.U[rows] * np.sqrt(got.lam), want.U[rows] * np.sqrt(want.lam)
    Cw = B @ B.T
    assert np.abs(A @ A.T - Cw).max() < 1e-8 * np.abs(Cw).max()


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
def test_laplacian_is_the_oracles():
    from oracle import gingr_oracle as go
    for name in ("small", "doubled", "tetra"):
        v, c, L = mesh(name)
        assert np.array_equal(L, go.graph_laplacian(v.shape[0], c))


@pytest.mark.parametrize("name,k,gap", [("femur", 4, 0.43), ("femur", 34, 0.053), ("femur", 170, 0.011), ("small", 8, 0.148), ("small", 33, 0.073)])
def test_restatement_against_eigh(name, k, gap):
    L = mesh(name)[2]
    theta, V, info = rs.solve(L, k)
    want, mu = rs.eigh_model(L, k, 30.0)
    assert info.converged and info.n_components == 1 and info.n_dropped == 1 and info.max_residual <= 1e-10
    assert abs(info.cut_gap - gap) < 0.1 * gap and abs((mu[k + 1] - mu[k]) / mu[k] - gap) < 0.05 * gap
    assert info.total_degree <= rs.DEFAULT_MAX_DEGREE // 4          # the default budget keeps its margin of four
    check(rs.expand(theta, V, 30.0), want)
    assert np.all(V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0)


def test_restatement_components_and_small_inputs():
    L = mesh("doubled")[2]
    theta, V, info = rs.solve(L, 8)
    assert info.n_components == 3 and info.n_dropped == 3 and abs(info.cut_gap - 0.195) < 0.0195
    check(rs.expand(theta, V, 30.0), rs.eigh_model(L, 8, 30.0)[0])
    lone = (L.shape[0] - 1) // 2
    assert not V[lone].any()
    theta7, V7, info7 = rs.solve(L, 7)                               # a cut inside a double eigenvalue
    assert info7.converged and info7.cut_gap < 1e-6 and np.allclose(theta7, np.linalg.eigvalsh(L)[3:10], rtol=1e-9)
    Lt = mesh("tetra")[2]
    theta, V, info = rs.solve(Lt, 3)
    assert np.allclose(theta, 4.0, rtol=1e-12) and info.cut_gap == math.inf and info.total_degree == 2
    assert np.allclose(V @ V.T * (30.0 / 4.0), 30.0 * np.linalg.pinv(Lt), atol=1e-12)
    assert rs.solve(Lt, 1)[0].shape == (1,)
    for k in (4, 0, 171):
        with pytest.raises(rs.LaplacianError):
            rs.solve(Lt, k)


def test_restatement_drops_what_lies_below_the_cutoff():
    """a band of 2 x 1 200 vertices: mu_1 = 8.6e-6 is dropped with the null vector, the model starts at mu_2 = 3.4e-5"""
    v, c = rs.strip(1200)
    L = rs.laplacian(v.shape[0], c)
    mu = np.linalg.eigvalsh(L)
    assert mu[1] <= rs.CUTOFF < mu[2]
    theta, V, info = rs.solve(L, 3)
    assert info.converged and info.n_components == 1 and info.n_dropped == 2 and info.total_degree <= rs.DEFAULT_MAX_DEGREE // 4
    assert np.linalg.norm(theta - mu[2:5]) < 1e-8 * np.linalg.norm(mu[2:5])
    assert abs(info.cut_gap - (mu[5] - mu[4]) / mu[4]) < 0.1 * (mu[5] - mu[4]) / mu[4]
    assert np.abs(V.T @ V - np.eye(3)).max() < 1e-9
    assert (np.linalg.norm(L @ V - V * theta[None, :], axis=0) / (2.0 * np.diag(L).max())).max() <= 1.01e-10


def test_restatement_budget():
    L = mesh("small")[2]
    with pytest.raises(rs.NotConverged) as e:
        rs.solve(L, 8, max_degree=1)
    assert e.value.info.converged == 0 and e.value.info.total_degree == 0
    with pytest.raises(rs.NotConverged) as e:
        rs.solve(L, 8, max_degree=40)
    assert 0 < e.value.info.total_degree <= 40 and e.value.info.max_residual > 1e-10


def test_filter_is_scaled_at_zero_and_bounded_on_its_interval():
    """the recurrence evaluates p_d with p_d(0) = 1 and |p_d| <= 1 / T_d(c / e) on [a, bound]"""
    f = rs.filter_plan(2.25, 20.0, 4000)
    x = np.concatenate([[0.0], np.linspace(f.a, f.bound, 400)])
    prev, cur = None, np.ones_like(x)
    for alpha, beta, gamma in rs.recurrence_steps(f):
        prev, cur = cur, alpha * x * cur + beta * cur + (gamma * prev if prev is not None else 0.0)
    assert abs(cur[0] - 1.0) < 1e-12
    assert np.abs(cur[1:]).max() <= (1.0 + 1e-9) / rs.filter_spread(f, f.degree)
    assert rs.filter_spread(f, f.degree) <= rs.SPREAD_BOUND < rs.filter_spread(f, f.degree + 1)


# ---------------------------------------------------------------------------------------------------------------- 2. the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("lap_plan") / "lap_spectral_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "lap_spectral_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def ask(driver, text):
    return subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def edges(driver, n, cells):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    out = ask(driver, f"edges {n} {cells.shape[0]} " + " ".join(str(int(x)) for x in cells.ravel()) + "\n")
    status, bad, ne = (int(x) for x in out[0].split())
    e = np.array([[int(x) for x in line.split()] for line in out[1:1 + ne]], dtype=np.int32).reshape(-1, 2)
    return status, bad, e


def test_plan_edges_from_cells(driver):
    for name in ("small", "doubled", "tetra"):
        v, c, _ = mesh(name)
        status, bad, e = edges(driver, v.shape[0], c)
        assert status == 0 and bad == -1 and np.array_equal(e, rs.edges_from_cells(v.shape[0], c))
    # duplicate triangles, triangles in both orientations, shared edges, an unreferenced vertex, a cell that names a vertex twice
    cells = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 2, 3], [5, 5, 3]]
    status, bad, e = edges(driver, 7, cells)
    assert status == 0 and np.array_equal(e, [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [3, 5]])
    assert np.array_equal(e, rs.edges_from_cells(7, cells))
    assert edges(driver, 3, [[0, 1, 2], [0, 1, 3]])[:2] == (1, 1)      # an index == n
    assert edges(driver, 3, [[0, -1, 2]])[:2] == (1, 0)                # a negative index
    assert edges(driver, 3, np.zeros((0, 3)))[0] == 3                  # no cells


@pytest.mark.parametrize("k,dim,want", [(1, 1621, (16, 16)), (8, 1621, (16, 16)), (9, 1621, (32, 32)), (13, 220, (32, 32)), (14, 220, (32, 32)),
                                        (170, 1621, (192, 192)), (170, 180, (192, 180)), (3, 3, (16, 3)), (1, 3, (16, 3))])
def test_plan_block_widths(driver, k, dim, want):
    got = tuple(int(x) for x in ask(driver, f"block {k} {dim}\n")[0].split())
    assert got == want == rs.block_plan(k, dim)
    assert got[0] % 16 == 0 and got[0] <= 192 and (got[1] == dim or got[1] >= k + rs.MIN_GUARD)


@pytest.mark.parametrize("theta,bound,budget", [(2.25, 20.0, 4000), (7.9, 22.0, 4000), (0.02, 24.0, 4000), (0.02, 24.0, 37), (19.99, 20.0, 4000),
                                                (6.0, 6.0, 5), (1e-300, 20.0, 4000), (2.25, 20.0, 1)])
def test_plan_filter_and_recurrence(driver, theta, bound, budget):
    out = ask(driver, f"filter {theta!r} {bound!r} {budget}\n")
    head = out[0].split()
    a, c, e, sigma1, spread, spread_next = (float(head[i]) for i in (0, 1, 2, 3, 5, 6))
    degree = int(head[4])
    f = rs.filter_plan(theta, bound, budget)
    assert (a, c, e, sigma1, degree) == (f.a, f.c, f.e, f.sigma1, f.degree)
    # the degree rule at its bounds: at least 1, within the budget and the step limit, and the largest whose spread stays below the bound
    assert 1 <= degree <= min(budget, rs.MAX_STEP_DEGREE) and a <= 0.95 * bound
    assert degree == 1 or spread <= rs.SPREAD_BOUND
    if degree < min(budget, rs.MAX_STEP_DEGREE):
        assert spread_next > rs.SPREAD_BOUND
    steps = np.array([[float(x) for x in line.split()] for line in out[1:1 + degree]])
    want = np.array(rs.recurrence_steps(f))
    assert steps.shape == want.shape and np.allclose(steps, want, rtol=1e-14, atol=0.0)


def test_plan_stop_rule(driver):
    assert ask(driver, "stop 1e-10 3 1e-11 1e-10 9e-11\n")[0] == "1"
    assert ask(driver, "stop 1e-10 3 1e-11 1.1e-10 9e-11\n")[0] == "0"
    assert ask(driver, "stop 1e-10 2 1e-11 nan\n")[0] == "0"
    assert ask(driver, "stop 1e-10 0\n")[0] == "1"
    assert ask(driver, "dropped 3 1e-6 1e-5 2e-5\n")[0] == "2"
    assert ask(driver, "dropped 2 0.5 0.6\n")[0] == "0"


# ---------------------------------------------------------------------------------------------------------------- 3. the interface
def test_the_call_is_declared_everywhere():
    from gingr_amd import _native as nat
    import gingr_amd as ga
    from gingr_amd import simple as sp
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    assert re.search(r"int gingr_model_from_laplacian\(", header) and "gingr_laplacian_info" in header
    res, args = nat.SIGNATURES["gingr_model_from_laplacian"]
    assert len(args) == 11
    fields = [f[0] for f in nat.LaplacianInfo._fields_]
    body = re.sub(r"/\*.*?\*/", "", header.split("typedef struct gingr_laplacian_info {")[1].split("}")[0], flags=re.S)
    assert fields == re.findall(r"(\w+);", body)
    assert hasattr(ga.GPMMTriangleMesh3D, "InverseLaplacianSpectral") and sp.InvLapSpectralKernel(30.0, 102).printpars == "30.0_102"
    make = open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()
    assert "lap_spectral.hip" in make and "lap_spectral_plan.h" in make
    plan = open(os.path.join(ROOT, "gingr_amd", "csrc", "lap_spectral_plan.h")).read()
    assert f"kLapDefaultMaxDegree = {rs.DEFAULT_MAX_DEGREE};" in plan
