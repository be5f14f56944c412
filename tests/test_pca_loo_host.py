"""CPU side of the leave-one-out generalization (gingr_amd/csrc/pca_leave_one_out.hip): the two routes of tests/pca_loo_restatement.py
against each other on every data set of the GPU tests (the measured spread is what the GPU tolerance is built on) and against
hand-worked cases, the bookkeeping header (gingr_amd/csrc/pca_loo_plan.h) compiled for the host with the address and
undefined-behaviour sanitizers into a stand-alone driver (tests/c/pca_loo_plan_driver.cpp), and the entry in the header, the loader
and the Python layer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import pca_loo_restatement as lr
from tests import pca_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
DATA = [(M, n, None, ranks) for M, n, ranks in lr.CASES] + [(M, n, r, ranks) for M, n, r, ranks in lr.LOW_RANK]


# ------------------------------------------------------------------------------------------------------------ the two routes
@pytest.mark.parametrize("M,n,r,ranks", DATA, ids=[f"M{M}-n{n}" + (f"-r{r}" if r else "") for M, n, r, _ in DATA])
def test_route_spread_direct_against_gram(M, n, r, ranks):
    ref, X = pr.dataset(M, n) if r is None else pr.low_rank_dataset(M, n, r)
    a1, m1, f1 = lr.loo_direct(X, ranks)
    a2, m2, f2 = lr.loo_gram(X, ranks)
    spread = max(float(np.abs(a1 - a2).max()), float(np.abs(m1 - m2).max())) / lr.scale_of(ref, X)
    print(f"M={M} n={n} r={r}: fold ranks {f1.min()}..{f1.max()}, route spread {spread:.2e} of max |shape - ref|")
    assert np.array_equal(f1, f2), (f1, f2)
    assert spread <= lr.LOO_ROUTE_SPREAD
    assert np.all(a1 <= m1 + 1e-12) and np.all(m1 > 0)


def test_by_hand_three_shapes_of_one_point():
    """x0 = (0, 0, 0), x1 = (2, 0, 0), x2 = (1, 3, 0).  Fold 2: mean (1, 0, 0), one component along x of variance 2; x2 - mean = (0, 3, 0) has
    nothing along it: distance 3.  Fold 0: x1 - x2 = (1, -3, 0), variance 10 / 2 = 5, mean (1.5, 1.5, 0); d = x0 - mean = (-1.5, -1.5, 0) has
    3 / sqrt(10) along the component and 3.6 = 4.5 - 0.9 in squares across it; the ridge leaves eps / (5 + eps) of the former."""
    X = np.array([[[0.0, 0.0, 0.0]], [[2.0, 0.0, 0.0]], [[1.0, 3.0, 0.0]]])
    along = 3.0 / np.sqrt(10.0) * 1e-5 / (5.0 + 1e-5)
    want0 = np.sqrt(3.6 + along * along)
    for route in (lr.loo_direct, lr.loo_gram):
        avg, mx, rank = route(X, [1])
        assert rank.tolist() == [1, 1, 1]
        assert abs(avg[0, 2] - 3.0) < 1e-14 and abs(mx[0, 2] - 3.0) < 1e-14
        assert abs(avg[0, 0] - want0) < 1e-14 and abs(mx[0, 0] - want0) < 1e-14
        assert abs(avg[0, 1] - want0) < 1e-14           # the mirror image of fold 0 in the line x = 1


def test_fold_of_rank_zero():
    """three identical shapes and one different: the fold without the different one has no variance, its projection is its mean"""
    y = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 6.0]])
    z = y + np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 12.0]])
    X = np.stack([y, y, z, y])
    for route in (lr.loo_direct, lr.loo_gram):
        avg, mx, rank = route(X, [1, 2])
        assert rank.tolist() == [1, 1, 0, 1]
        assert np.allclose(avg[:, 2], 8.5, atol=1e-14) and np.allclose(mx[:, 2], 12.0, atol=1e-14)   # (5 + 12) / 2
        # the other folds: the one component points from y to z; y lies on it: only the ridge's bias is left
        assert np.all(avg[:, [0, 1, 3]] < 1e-4)
    assert lr.fold_is_rank0(np.stack([y, y, y])) and not lr.fold_is_rank0(np.stack([y, y, z]))


def test_weights_sum_rule():
    """the kept eigenvectors of a centred Gram matrix are orthogonal to the vector of ones, so the weights of the shapes that stay sum
    to zero -- the fold's mean takes no part in the projection -- and the left-out shape keeps exactly -(1 + a), a = 1 / (n - 1)"""
    ref, X = pr.dataset(37, 5)
    D = (X - X.mean(axis=0)).reshape(5, -1)
    for i in range(5):
        w, rank = lr.fold_weights(D @ D.T, i, [1, 2, 3], 1e-10)
        assert rank == 3 and np.allclose(w.sum(axis=1), -1.25, atol=1e-10) and np.allclose(w[:, i], -1.25, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("pca_loo_plan") / "pca_loo_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "pca_loo_plan_driver.cpp"),
                           "-o", str(exe)])

    def run(*case):
        out = subprocess.run([str(exe)] + [str(c) for c in case], capture_output=True, check=True, text=True).stdout.split("\n")
        return [[int(v) for v in line.split()] for line in out if line.strip()]
    return run


def test_rank_rules(plan_driver):
    assert plan_driver("ranks", 8, 1, 2, 3, 6, "end") == [[0, 3]]
    assert plan_driver("ranks", 8, "end") == [[1, 0]]
    assert plan_driver("ranks", 40, *range(1, 18), "end") == [[1, 0]]
    assert plan_driver("ranks", 40, *range(1, 17), "end") == [[0, 15]]
    assert plan_driver("ranks", 8, 0, "end") == [[2, 0]]
    assert plan_driver("ranks", 8, 1, 7, "end") == [[2, 1]]
    assert plan_driver("ranks", 3, 1, "end") == [[0, 0]]
    assert plan_driver("ranks", 3, 2, "end") == [[2, 0]]
    assert plan_driver("ranks", 8, 2, 2, "end") == [[3, 1]] and plan_driver("ranks", 8, 3, 2, "end") == [[3, 1]]


@pytest.mark.parametrize("n,i", [(3, 0), (3, 1), (3, 2), (17, 0), (17, 8), (17, 16), (512, 511)])
def test_fold_maps(plan_driver, n, i):
    rows = plan_driver("maps", n, i)
    assert len(rows) == n - 1
    assert [s for _, s, _ in rows] == [j for j in range(n) if j != i]
    assert all(r == back for r, _, back in rows)


@pytest.mark.parametrize("n", [3, 4, 16, 17, 100, 193, 194, 300, 512])
def test_fold_batches_cover_every_fold_once(plan_driver, n):
    work = 192 * (n - 1) + 192 if n - 1 <= 192 else 0
    rows = plan_driver("batches", n, work)
    per, count, padded, nbytes = rows[0]
    assert padded % 16 == 0 and n <= padded < n + 16
    assert nbytes == (2 * (n - 1) ** 2 + 2 * (n - 1) + work) * 8
    assert min(3, n) <= per <= n and len(rows) - 1 == count == -(-n // per)
    assert per == n or per * nbytes <= 256 << 20 or per == 3
    at = 0
    for begin, length in rows[1:]:
        assert begin == at and 1 <= length <= per
        at += length
    assert at == n
    if n <= 193:
        assert count == 1      # the folds of a call on the register kernel: one launch


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entry_is_declared_bound_and_exported():
    import ctypes
    from gingr_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    name = "gingr_pca_leave_one_out"
    assert re.search(rf"\bint {name}\s*\(", header)
    assert name in _native.SIGNATURES and hasattr(lib, name)
    assert len(_native.SIGNATURES[name][1]) == 10
    common = open(os.path.join(ROOT, "gingr_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define GINGR_TIMERS (\d+)", common).group(1)) >= 23      # hook 22: the batched decomposition


def test_python_layer_names():
    import gingr_amd as ga
    from gingr_amd import api, metrics
    assert callable(ga.ModelMetrics.generalizationLeaveOneOut)
    assert api.LeaveOneOutResult is metrics.LeaveOneOutResult
    res = metrics.LeaveOneOutResult(np.array([1, 2]), np.array([[1.0, 3.0], [0.5, 1.5]]), np.zeros((2, 2)), np.array([2, 2]))
    assert np.array_equal(res.curve(), [2.0, 1.0])
    with pytest.raises(ValueError):
        ga.ModelMetrics.generalizationLeaveOneOut(None, np.zeros((4, 7)))
