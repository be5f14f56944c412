"""CPU side of the model metrics (gingr_amd/csrc/model_metrics.hip): the longdouble restatement (tests/model_metrics_restatement.py)
against hand-worked cases -- the nested-factor shortcut against the direct solve of every leading block, distances, the specificity
minimum with its tie rule, compactness against a hand sum -- the conditioning of the models the GPU tests rely on, the planner
(gingr_amd/csrc/model_metrics_plan.h) compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone
driver (tests/c/model_metrics_plan_driver.cpp), and the three entries in the header, the loader and the Python layer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import model_metrics_restatement as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_model_instances", "gingr_model_generalization", "gingr_model_specificity"]
PLAN_M = [1, 15, 16, 17, 127, 128, 129, 2049, 50000]
PLAN_COLS = [1, 63, 64, 65, 512, 513]


# ------------------------------------------------------------------------------------------------------ the restatement
def test_nested_factor_equals_the_direct_solve_of_every_leading_block():
    """3 x 3 by hand: B = [[4, 2, 0], [2, 5, 3], [0, 3, 6]] has L = [[2, 0, 0], [1, 2, 0], [0, 1.5, sqrt(3.75)]]; the leading blocks of L
    and of L^-T are the factors of the leading blocks of B."""
    B = np.array([[4, 2, 0], [2, 5, 3], [0, 3, 6]], dtype=mm.LD)
    L = mm.cholesky(B)
    assert np.allclose(np.asarray(L, dtype=float), [[2, 0, 0], [1, 2, 0], [0, 1.5, np.sqrt(3.75)]], atol=1e-15)
    W = mm.solve_lower(L, np.eye(3, dtype=mm.LD)).T
    rhs = np.array([1.0, -2.0, 0.5], dtype=mm.LD)
    for k in (1, 2, 3):
        direct = mm.solve_spd(B[:k, :k], rhs[:k])
        nested = W[:k, :k] @ (W[:k, :k].T @ rhs[:k])
        assert float(np.abs(direct - nested).max()) < 1e-17
    assert float(abs(mm.solve_spd(B[:1, :1], rhs[:1])[0] - mm.LD(0.25))) < 1e-18            # 1 / 4
    assert float(np.abs(mm.solve_spd(B[:2, :2], rhs[:2]) - np.array([9, -10], dtype=mm.LD) / 16).max()) < 1e-18   # [[5,-2],[-2,4]]/16 rhs


@pytest.mark.parametrize("M,r", [(4, 3), (17, 9), (40, 33)])
def test_nested_projection_equals_direct_projection(M, r):
    mo = mm.random_model(M, r, 7 + M)
    rng = np.random.default_rng(M)
    X = mo.ref + mo.mean + rng.normal(0, 2.0, (5, M, 3))
    ranks = sorted({1, max(1, r // 2), r})
    cd, ad, xd = mm.project_direct(mo, X, ranks)
    cn, an, xn = mm.project_nested(mo, X, ranks)
    cond = mm.condition(mo.Q)
    scale = float(np.abs(cd).max())
    assert float(np.abs(cd - cn).max()) <= 64 * r * r * 2.0 ** -64 * cond * scale
    assert float(np.abs(ad - an).max()) < 1e-15 and float(np.abs(xd - xn).max()) < 1e-15
    for q, k in enumerate(ranks):
        assert not np.any(np.asarray(cd[q, :, k:], dtype=float)) and not np.any(np.asarray(cn[q, :, k:], dtype=float))


def test_projection_by_hand():
    """one point, one basis function along x of length 2 (variance 4): Q = (2, 0, 0)^T, S = 4, alpha = (2 dx / eps) / (4 / eps + 1)"""
    mo = mm.Model(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.array([[1.0], [0.0], [0.0]]), np.array([4.0]))
    x = np.array([[[4.0, 3.0, 0.0]]])
    coef, avg, mx = mm.project_direct(mo, x, [1])
    alpha = (2 * 3.0 / 1e-5) / (4 / 1e-5 + 1)
    assert abs(float(coef[0, 0, 0]) - alpha) < 1e-15
    want = np.hypot(3.0 - 2 * alpha, 3.0)    # the residual along x (the ridge's bias) and the 3 along y the model cannot reach
    assert abs(float(avg[0, 0]) - want) < 1e-15 and abs(float(mx[0, 0]) - want) < 1e-15


def test_instance_of_the_model_comes_back_at_the_ridge_bias():
    mo = mm.random_model(30, 6, 3)
    a = np.array([[1.0, -0.5, 0.25, 2.0, 0.0, -1.0]])
    x = np.asarray(mm.instances(mo, a), dtype=np.float64)
    coef, avg, _ = mm.project_direct(mo, x, [6])
    assert 1e-9 < float(avg[0, 0]) < 1e-4 and float(np.abs(coef[0, 0] - a[0]).max()) < 1e-4


def test_specificity_minimum_and_tie_rule():
    mo = mm.Model(np.zeros((2, 3)), np.zeros((2, 3)), np.eye(6)[:, :2], np.array([1.0, 1.0]))
    # samples: alpha = (3, 4) moves vertex 0 to (3, 4, 0); training shapes: zero, zero again, and the sample itself
    train = np.zeros((3, 2, 3))
    train[2, 0] = [3.0, 4.0, 0.0]
    means, mn, am = mm.specificity(mo, train, np.array([[3.0, 4.0], [0.0, 0.0]]), [1, 2])
    assert np.allclose(np.asarray(means[1, 0], dtype=float), [2.5, 2.5, 0.0])      # (5 + 0) / 2
    assert np.allclose(np.asarray(means[0, 0], dtype=float), [1.5, 1.5, 2.0])      # rank 1: the sample is (3, 0, 0)
    assert am.tolist() == [[0, 0], [2, 0]] and np.allclose(np.asarray(mn, dtype=float), [[1.5, 0.0], [0.0, 0.0]])


def test_compactness_against_a_hand_sum():
    import gingr_amd as ga
    var = np.array([8.0, 4.0, 2.0, 1.0, 1.0])
    host = ga.PointDistributionModel(np.zeros((2, 3)), np.zeros((2, 3)), np.eye(6)[:, :5], var)
    got = ga.ModelMetrics.compactness(host)
    assert np.array_equal(got, np.array([8.0, 12.0, 14.0, 15.0, 16.0]) / 16.0)
    assert np.array_equal(ga.ModelMetrics.compactness(host, ranks=[1, 5]), [0.5, 1.0])
    assert np.allclose(np.asarray(mm.compactness(var), dtype=float), got)


def test_bounds_refuse_a_wrong_result():
    """one vertex left out of a mean, or one coefficient more than k, lies far outside the bound"""
    mo = mm.random_model(130, 17, 5)
    rng = np.random.default_rng(1)
    X = mo.ref + mo.mean + rng.normal(0, 2.0, (3, 130, 3))
    coef, avg, mx = mm.project_direct(mo, X, [5, 17])
    b = mm.projection_bounds(mo, X, [5, 17])
    D = mm.centred(mo, X)
    dist = mm.vertex_distances(coef[0] @ np.asarray(mo.Q, dtype=mm.LD).T, D)
    assert float(np.abs(dist[:, :-1].sum(axis=1) / 130 - avg[0]).min()) > 1e6 * b["avg"].max()
    c6, _, _ = mm.project_direct(mo, X, [6])
    assert float(np.abs(c6[0] - coef[0]).max()) > 1e6 * b["coef"].max()
    assert b["avg"].max() < 1e-8 and b["coef"].max() < 1e-8


def test_models_of_the_gpu_tests_are_well_conditioned():
    """variances within [0.25, 64]: cond(S / eps + I) stays moderate, so that the single-call route of the GPU tests is itself inside the
    bounds (tests/test_gpu_model_metrics.py builds its uploaded models with random_model at these sizes)"""
    for M, r, seed in [(130, 17, 11), (130, 48, 12), (257, 35, 13), (40, 20, 14)]:
        cond = mm.condition(mm.random_model(M, r, seed).Q)
        print(f"M={M} r={r}: cond_inf(S / eps + I) = {cond:.1f}")
        assert cond < 2e4, (M, r, cond)


# ---------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("model_metrics_plan") / "model_metrics_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "model_metrics_plan_driver.cpp"),
                           "-o", str(exe)])

    def run(*case):
        out = subprocess.run([str(exe)] + [str(c) for c in case], capture_output=True, check=True, text=True).stdout.split("\n")
        return [[int(v) for v in line.split()] for line in out if line.strip()]
    return run


def check_slabs(rows, M, vps, slabs, granule):
    assert len(rows) == slabs >= 1 and vps % granule == 0
    assert rows[0][0] == 0 and rows[-1][1] == M
    for s, (b, e) in enumerate(rows):
        assert b == s * vps and b < e <= b + vps, "an empty or overlong slab"
        assert s == 0 or rows[s - 1][1] == b


@pytest.mark.parametrize("n", PLAN_COLS + [1024, 1025])
def test_column_blocks_cover_every_column_once(plan_driver, n):
    rows = plan_driver("blocks", n)
    count, blocks = rows[0][0], rows[1:]
    assert count == len(blocks) == -(-n // 512)
    at = 0
    for begin, length, padded in blocks:
        assert begin == at and 1 <= length <= 512 and padded % 16 == 0 and length <= padded < length + 16
        at += length
    assert at == n


@pytest.mark.parametrize("M", PLAN_M)
@pytest.mark.parametrize("cols", PLAN_COLS + [8192])
def test_measure_plan(plan_driver, M, cols):
    head, rows = plan_driver("measure", M, cols)[0], plan_driver("measure", M, cols)[1:]
    pc, chunks, vps, slabs, partial = head
    assert pc % 16 == 0 and cols <= pc < cols + 16 and chunks == -(-pc // 64) and partial == slabs * 2 * pc
    check_slabs(rows, M, vps, slabs, 128)
    assert slabs * chunks <= max(1024 + chunks, chunks)


def test_measure_plan_never_leaves_an_empty_last_slab(plan_driver):
    """M = 1 300 with 128 chunks: 8 slabs wanted, 163 vertices each, rounded up to 256 -- the vertices fill 6 such slabs, and slabs 7 and
    8 would be empty: the count is taken again from the slab length, so that the last slab always holds vertices"""
    rows = plan_driver("measure", 1300, 8192)
    assert rows[0][2] == 256 and rows[0][3] == 6 and rows[-1] == [1280, 1300]
    for M, cols in [(1300, 8192), (1025, 64), (2049, 1024), (129, 64), (50000, 8192), (640, 64)]:
        rows = plan_driver("measure", M, cols)
        check_slabs(rows[1:], M, rows[0][2], rows[0][3], 128)
        assert rows[-1][0] < M
    rows = plan_driver("pair", 100, 512, 512)   # 100 vertices in slabs of 32: the last one holds 4
    assert rows[0][4] == 32 and rows[0][5] == 4 and rows[-1] == [96, 100]


@pytest.mark.parametrize("M", PLAN_M)
@pytest.mark.parametrize("S,T", [(1, 1), (63, 15), (64, 17), (65, 512), (512, 512), (512, 1)])
def test_pair_plan(plan_driver, M, S, T):
    rows = plan_driver("pair", M, S, T)
    sp, tp, ts, tt, vps, slabs, partial = rows[0]
    assert sp % 16 == 0 and S <= sp < S + 16 and tp % 16 == 0 and T <= tp < T + 16
    assert ts == -(-sp // 64) and tt == -(-tp // 64) and partial == slabs * sp * tp <= 1 << 24
    check_slabs(rows[1:], M, vps, slabs, 32)


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entries_are_declared_bound_and_exported():
    import ctypes
    from gingr_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in FUNCTIONS:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name


def test_python_layer_names():
    import gingr_amd as ga
    from gingr_amd import api, metrics
    assert api.ModelMetrics is metrics.ModelMetrics is ga.ModelMetrics
    for name in ("generalization", "specificity", "compactness"):
        assert callable(getattr(ga.ModelMetrics, name))
    assert callable(ga.DeviceModel.instances) and callable(ga.DeviceModel.project)
    res = metrics.GeneralizationResult(np.array([1, 2]), np.array([[1.0, 3.0], [0.5, 1.5]]), np.zeros((2, 2)), np.zeros((2, 2, 2)))
    assert np.array_equal(res.curve(), [2.0, 1.0])
    spec = metrics.SpecificityResult(np.array([2]), np.array([[1.0, 2.0, 6.0]]), np.zeros((1, 3), dtype=np.int64), np.zeros((3, 2)))
    assert np.array_equal(spec.curve(), [3.0])
