"""CPU tests of the k-nearest-neighbour normals (gingr_cloud_knn / gingr_cloud_normals) and of point-to-plane ICP against a point cloud:
the numpy restatement (tests/cloud_normals_restatement.py) against scipy's k-d tree and numpy's eigh, the grid plan
(gingr_amd/csrc/cloud_knn_plan.h) and the 3 x 3 symmetric eigen-solver (gingr_amd/csrc/sym_eig3.h) compiled for the host with the
address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/cloud_knn_plan_driver.cpp), and the new entries in the
header, the library and the loader."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cloud_normals_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_cloud_knn", "gingr_cloud_normals", "gingr_fitter_set_target_normals", "gingr_fitter_estimate_target_normals",
             "gingr_fitter_get_target_normals", "gingr_fitter_set_pairs_plane_cloud_async", "gingr_fitter_update_plane_cloud_async"]


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N, k", [(200, 3), (500, 16), (300, 64)])
def test_lists_are_the_kd_trees_on_clouds_without_ties(N, k):
    from scipy.spatial import cKDTree
    x = np.random.default_rng(N + k).uniform(-1, 1, (N, 3))
    idx, d2 = cr.knn(x, k)
    dist, tree = cKDTree(x).query(x, k)
    assert (np.diff(d2, axis=1) > 0).all()                                   # no ties: the lists are sets with one order
    assert np.array_equal(np.sort(idx, axis=1), np.sort(tree, axis=1))
    assert np.array_equal(idx[:, 0], np.arange(N)) and not d2[:, 0].any()    # the point itself comes first
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-14, atol=0)


def test_ties_go_to_the_lowest_index():
    g = np.arange(4.0)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    x = np.concatenate([x, x[:5]])                                           # duplicates of the first five points
    idx, d2 = cr.knn(x, 8)
    for j in range(x.shape[0]):
        key = list(zip(d2[j], idx[j]))
        assert key == sorted(key)
        row = cr.d2_matrix_row(x, j)
        rest = np.setdiff1d(np.arange(x.shape[0]), idx[j])
        assert (row[rest] >= d2[j, -1]).all() and (rest[row[rest] == d2[j, -1]] > idx[j, -1]).all()
    assert idx[64, 0] == 0 and idx[0, 0] == 0 and idx[0, 1] == 64            # a duplicate: the lower index first


def test_normals_agree_with_numpy_eigh_and_the_rules_hold():
    rng = np.random.default_rng(5)
    u = rng.normal(0, 1, (400, 3))
    x = u / np.linalg.norm(u, axis=1)[:, None] * np.array([3.0, 2.0, 1.0])   # an ellipsoid
    n, var, lam, idx = cr.normals(x, 12)
    w, V = np.linalg.eigh(cr.moments(x, idx))
    assert np.allclose(lam, w, rtol=1e-10, atol=1e-14)
    assert (np.abs((n * V[:, :, 0]).sum(1)) > 1 - 1e-10).all()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, rtol=1e-14)
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)
    assert (lead > 0).all() and (var >= 0).all() and (var < 0.1).all()
    # with the viewpoint at the centre every normal points inward; the longdouble run agrees to double rounding
    inward = cr.normals(x, 12, viewpoint=np.zeros(3), idx=idx)[0]
    assert ((inward * x).sum(1) < 0).all() and np.array_equal(np.abs(inward), np.abs(n))
    n_ld = cr.normals(x, 12, dtype=np.longdouble, idx=idx)[0]
    assert np.abs(n_ld.astype(np.float64) - n).max() < 1e-12
    # translation changes nothing but rounding: the differences are taken first
    moved = cr.normals(x + 1e6, 12)[0]
    assert np.abs(moved - n).max() < 1e-6


def test_degenerate_neighbourhoods_give_the_zero_normal():
    line = np.stack([np.arange(20.0), np.zeros(20), np.zeros(20)], 1)
    n, var, lam, _ = cr.normals(line, 5)
    assert not n.any() and np.isfinite(var).all() and not var.any()
    same = np.ones((10, 3)) * 2.5
    n, var, _, _ = cr.normals(same, 4)
    assert not n.any() and not var.any()
    g = np.arange(6.0)
    sheet = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    sheet = np.concatenate([sheet, np.zeros((36, 1))], 1)
    n, var, _, _ = cr.normals(sheet, 9)
    assert np.array_equal(n, np.broadcast_to([0.0, 0.0, 1.0], n.shape)) and not var.any()


# ------------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("cloud_knn_plan") / "cloud_knn_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "cloud_knn_plan_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, check=True, text=True).stdout
    assert "FAIL" not in out, out
    plans, eigs = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "plan":
            plans[f[1]] = dict(N=int(f[2]), k=int(f[3]), dims=int(f[4]), h=float(f[5]), g=tuple(int(v) for v in f[6:9]), lanes=int(f[9]))
        else:
            eigs[f[1]] = dict(lam=np.array(f[2:5], dtype=float), n=np.array(f[5:8], dtype=float), var=float(f[8]), res=float(f[9]),
                              orth=float(f[10]))
    return plans, eigs


EXTENTS = {"three": (1.0, 2.0, 0.5), "thousand": (40.0, 40.0, 400.0), "million": (1.0, 1.0, 1.0), "million64": (1.0, 1.0, 1.0),
           "flat": (10.0, 7.0, 0.0), "line": (0.0, 7.0, 0.0), "onecell": (0.0, 0.0, 0.0), "sliver": (1e6, 1e-2, 1.0)}


def test_grid_sizing(driver):
    plans, _ = driver
    assert set(plans) == set(EXTENTS)
    for name, p in plans.items():
        e, g, h, N, k = EXTENTS[name], p["g"], p["h"], p["N"], p["k"]
        assert h > 0 and np.isfinite(h), name
        assert all(1 <= g[d] <= 1024 and g[d] == int(np.floor(e[d] / h)) + 1 for d in range(3)), (name, p)
        assert g[0] * g[1] * g[2] <= min(8 * N + 4096, 2 ** 30), (name, p)
        assert p["dims"] == sum(1 for d in range(3) if e[d] > 1e-9 * max(e)) if max(e) > 0 else p["dims"] == 0, name
        assert p["lanes"] == (16 if k <= 16 else 32 if k <= 32 else 64) and p["lanes"] >= k
    assert max(plans["three"]["g"]) <= 3                                      # three points: a block of two cells' half-width is the whole grid
    assert plans["onecell"]["g"] == (1, 1, 1) and plans["onecell"]["h"] == 1.0
    assert plans["flat"]["g"][2] == 1 and plans["flat"]["g"][0] > 10           # one cell thick
    assert plans["line"]["g"][0] == 1 and plans["line"]["g"][2] == 1 and plans["line"]["g"][1] > 100
    # the rule itself (cloud_knn_plan.h): the smaller of the volume and the surface radius that holds 2 k points
    for name in ("thousand", "million", "million64"):
        e, p = EXTENTS[name], plans[name]
        want = 2.0 * p["k"] / p["N"]
        hv = np.cbrt(want * e[0] * e[1] * e[2] * 3 / (4 * np.pi))
        hs = np.sqrt(want * 2 * (e[0] * e[1] + e[0] * e[2] + e[1] * e[2]) / np.pi)
        assert abs(p["h"] / min(hv, hs) - 1) < 1e-12, (name, p["h"], hv, hs)
    e, p = EXTENTS["flat"], plans["flat"]
    assert abs(p["h"] / np.sqrt(2.0 * p["k"] / p["N"] * e[0] * e[1] / np.pi) - 1) < 1e-12
    assert plans["sliver"]["g"][0] <= 1024 and plans["sliver"]["h"] >= 1e6 / 1024   # coarsened to fit the axis limit


def test_eigen_routine_against_closed_forms(driver):
    _, e = driver
    for name, c in e.items():
        assert c["res"] < 8 * 2.0 ** -52 and c["orth"] < 8 * 2.0 ** -52, (name, c)
    assert np.array_equal(e["diag"]["lam"], [1.0, 2.0, 3.0]) and np.array_equal(e["diag"]["n"], [0.0, 1.0, 0.0])
    assert e["diag"]["var"] == 1.0 / 6.0
    assert np.array_equal(e["repeated_low"]["lam"], [2.0, 2.0, 5.0]) and not e["repeated_low"]["n"].any()      # lam0 = lam1: no normal
    assert np.array_equal(e["repeated_high"]["lam"], [1.0, 4.0, 4.0]) and np.array_equal(e["repeated_high"]["n"], [1.0, 0.0, 0.0])
    assert not e["zero"]["lam"].any() and not e["zero"]["n"].any() and e["zero"]["var"] == 0.0
    assert not e["isotropic"]["n"].any() and e["isotropic"]["var"] == 1.0 / 3.0
    r1 = e["rank_one"]
    assert abs(r1["lam"][2] - 9.0) < 1e-14 and np.abs(r1["lam"][:2]).max() < 1e-14 and not r1["n"].any()          # a line: no normal
    pl = e["plane111"]
    assert np.allclose(pl["lam"], [0.0, 1.0, 4.0], atol=1e-14) and np.allclose(pl["n"], np.ones(3) / np.sqrt(3.0), atol=1e-14)
    assert abs(pl["var"]) < 1e-15
    w, V = np.linalg.eigh(np.array([[4.0, 1.0, -2.0], [1.0, 3.0, 0.5], [-2.0, 0.5, 6.0]]))
    for name, scale in (("general", 1.0), ("tiny", 1e-300), ("huge", 1e300)):
        c = e[name]
        assert np.allclose(c["lam"], w * scale, rtol=1e-13, atol=0), name
        assert abs(abs(c["n"] @ V[:, 0]) - 1) < 1e-13 and c["n"][np.argmax(np.abs(c["n"]))] > 0, name
        assert abs(c["var"] - w[0] / w.sum()) < 1e-14, name


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert ctypes.sizeof(_native.CloudKnnInfo) == 24 and ctypes.sizeof(_native.PlaneCloudParams) == 16
    srcs = open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()
    assert " cloud_knn.hip" in srcs and "cloud_knn_plan.h" in srcs and "sym_eig3.h" in srcs


def test_configuration_and_keywords():
    import inspect
    import gingr_amd as ga
    assert ga.PointToPlaneConfiguration().maxDistance is None
    assert ga.PointToPlaneConfiguration(100, 100.0, 1.0, 100.0, False, 1e-10).maxIterations == 100       # positional order unchanged
    sig = inspect.signature(ga.PointToPlaneIcpRegistration.createInitialState).parameters
    assert sig["targetNormals"].default is None and sig["targetNeighbours"].default == 16
    assert inspect.signature(ga.Context.cloud_normals).parameters["k"].default == 16
