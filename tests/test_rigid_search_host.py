"""CPU tests of the global rigid pre-alignment: the plan header (gingr_amd/csrc/rigid_search_plan.h) through a stand-alone C++ driver
built with the address and undefined-behaviour sanitizers (tests/c/rigid_search_plan_driver.cpp), the numpy restatement
(tests/rigid_search_restatement.py) against itself in extended precision and on the recovery inputs, and the C ABI / Python surface.

Recovery of the restatement itself (float64, k-d tree), re-measured with this file: over seeds 0..7 the rotation after 50 refining
iterations lies at most 1.02 degrees (plain, overlap 1) and 0.82 degrees (72 clutter points, overlap 0.85) from R_true R_base; the bound
of 3 degrees is about twice the prototype's 1.45, the spread of ICP's own fixed points."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import rigid_search_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_rotation_samples", "gingr_rigid_search"]
EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------------ the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("rigid_search_plan") / "rigid_search_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "rigid_search_plan_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, check=True, text=True).stdout
    assert "FAIL" not in out and "ok 0" in out, out
    return out


def test_spiral_equals_the_restatement(driver):
    quats, rots = {}, {}
    for line in driver.splitlines():
        w = line.split()
        if w[0] == "quat":
            quats[(int(w[1]), int(w[2]))] = [float.fromhex(v) for v in w[3:]]
        elif w[0] == "rot":
            rots[(int(w[1]), int(w[2]))] = [float.fromhex(v) for v in w[3:]]
    for n in (1, 2, 7, 64, 1000):
        q = np.array([quats[(n, i)] for i in range(n)])
        R = np.array([rots[(n, i)] for i in range(n)]).reshape(n, 3, 3)
        want_q = rs.spiral_quaternions(n, np.longdouble)
        # the angle 2 pi s / phi reaches 2 pi n / sqrt 2: its rounding (eps / 2 relative) moves sine and cosine by that much, absolutely
        tol = 4 * EPS * max(1.0, 2 * math.pi * n / math.sqrt(2.0))
        assert np.abs(q - want_q.astype(np.float64)).max() <= tol, n
        assert np.abs(R - rs.rotation_samples(n, np.longdouble).astype(np.float64)).max() <= 8 * tol, n
        assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-14
        assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() <= 1e-14            # unit quaternions: orthonormal,
        assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14                                   # determinant +1
    # evenly spread: 64 disjoint balls of SO(3) (volume 8 pi^2, a ball of radius a: 4 pi (a - sin a)) have a radius below 49 degrees, so
    # no arrangement separates 64 rotations by 98 degrees; random ones come as close as ~10.  The spiral: all above 30, every nearest below 60
    R = np.array([rots[(64, i)] for i in range(64)]).reshape(64, 3, 3)
    ang = np.array([[rs.angle_deg(a, b) if i != j else 1e9 for j, b in enumerate(R)] for i, a in enumerate(R)])
    assert ang.min() > 30.0 and ang.min(1).max() < 60.0


def test_keep_is_the_ceiling_of_the_product(driver):
    rows = [(int(m), float.fromhex(r), int(k)) for m, r, k in re.findall(r"keep (\d+) (\S+) (\d+)", driver)]
    assert len(rows) > 100
    for M, rho, keep in rows:
        assert keep == min(M, max(1, math.ceil(rho * M))) == rs.keep_count(M, rho), (M, rho)
    table = {(M, rho): k for M, rho, k in rows}
    assert table[(10, 0.5)] == 5 and table[(10, float(np.nextafter(0.5, 2.0)))] == 6 and table[(10, float(np.nextafter(0.5, 0.0)))] == 5
    assert table[(478, 0.85)] == 407 and table[(406, 1.0)] == 406 and table[(1000, 1e-300)] == 1
    for M in (2, 3, 255, 256, 257, 1000):                                                   # the overlaps of the trimming tests
        assert table[(M, (M - 1) / M)] == M - 1 and table[(M, 1 / M)] == 1 and table[(M, 0.5)] == math.ceil(M / 2)


def test_slabs_depend_on_sizes_only_and_cover_every_pose(driver):
    slabs = {(int(m), int(n)): int(p) for m, n, p in re.findall(r"slab (\d+) (\d+) (\d+)", driver)}
    assert len(slabs) == 9 * 6                                                               # (the driver checks the cover for 7 values of S each)
    assert all(1 <= p <= 64 for p in slabs.values())
    assert slabs[(406, 1622)] == 64 and slabs[(1000, 5000)] == 64 and slabs[(2000, 1622)] == 64      # 64 starts: one slab
    assert slabs[(4097, 1622)] == 63 and slabs[(300000, 1622)] == 1 and slabs[(2147483647, 2147483647)] == 1
    assert slabs[(2000, 1000000)] == 8                                                       # a large target: the tile scan's work bounds the slab
    src = open(os.path.join(ROOT, "gingr_amd", "csrc", "rigid_search_plan.h")).read()
    assert re.search(r"inline int64_t slab_poses\(int64_t M, int64_t N\)", src)              # no S in the signature
    blocks = {int(m): int(b) for m, b in re.findall(r"blocks (\d+) (\d+)", driver)}
    assert [blocks[m] for m in (1, 255, 256, 257, 1000, 8192, 8193)] == [1, 1, 1, 2, 4, 32, 32]


# ------------------------------------------------------------------------------------------------------ the restatement
def cloud_case(M, N, S, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 30.0, (M, 3)) + [200.0, -50.0, 10.0]
    Y = rng.normal(0, 30.0, (N, 3)) + [-40.0, 300.0, 80.0]
    R0 = np.stack([rs.random_rotation(rng) for _ in range(S)])
    return X, Y, R0


def spread(X, Y, R0, K, rho):
    """(float64 result, longdouble result, spread of rotations, translations, scores): brute-force search in both"""
    a = rs.search(X, Y, R0, K, rho, np.float64, brute=True)
    b = rs.search(X, Y, R0, K, rho, np.longdouble, brute=True)
    return a, b, (float(np.abs(a["rotations"] - b["rotations"]).max()), float(np.abs(a["translations"] - b["translations"]).max()),
                  float(np.abs(a["scores"] - b["scores"]).max()))


@pytest.mark.parametrize("M,N,S,rho", [(257, 500, 5, 1.0), (1000, 700, 3, 0.5), (255, 7, 4, 1.0)])
def test_float64_against_longdouble(M, N, S, rho):
    X, Y, R0 = cloud_case(M, N, S)
    a, b, (sr, st, ss) = spread(X, Y, R0, 1, rho)
    scale = max(np.abs(X).max(), np.abs(Y).max())
    print(f"M {M} N {N} rho {rho}: spread rotation {sr:.3g} translation {st:.3g} ({st / scale:.3g} of the scale) score {ss:.3g}")
    assert np.array_equal(a["kept"], b["kept"]) and a["best"] == b["best"]
    # one well-posed iteration: float64 carries the result to a few thousand units of rounding of the coordinates' scale
    assert sr <= 4096 * EPS and st <= 4096 * EPS * scale and ss <= 4096 * EPS * scale
    # k-d tree and argmin over all pairs: the same matches, so the same bits
    c = rs.search(X, Y, R0, 1, rho)
    assert np.array_equal(c["rotations"], a["rotations"]) and np.array_equal(c["scores"], a["scores"]) and np.array_equal(c["kept"], a["kept"])


def test_ties_stay_and_rho_one_keeps_everything():
    d2 = np.array([4.0, 1.0, 1.0, 9.0, 1.0, 0.5])
    assert rs.kept_mask(d2, 1).sum() == 1 and rs.kept_mask(d2, 2).sum() == 4 and rs.kept_mask(d2, 4).sum() == 4
    assert rs.kept_mask(d2, 5).sum() == 5 and rs.kept_mask(d2, 6).all()
    Y = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    j, _ = rs.nearest_brute(np.array([[0.9, 0, 0], [0.1, 0, 0]]), Y)
    assert j.tolist() == [1, 0]                                                              # the lowest index on ties
    from scipy.spatial import cKDTree
    j2, _ = rs.nearest(np.array([[0.9, 0, 0], [0.1, 0, 0]]), Y, cKDTree(Y))
    assert j2.tolist() == [1, 0]


def test_step_is_exact_on_a_rigid_copy_and_proper_on_a_reflection():
    rng = np.random.default_rng(2)
    p = rng.normal(0, 10, (50, 3))
    R = rs.random_rotation(rng)
    t = np.array([5.0, -3.0, 2.0])
    dR, dt = rs.step(p, p @ R.T + t, np.array([1.0, 2.0, 3.0]))
    assert np.abs(dR - R).max() < 1e-13 and np.abs(dt - t).max() < 1e-12
    dR, _ = rs.step(p, p * [1.0, 1.0, -1.0], np.zeros(3))                                    # a mirror image: still a rotation
    assert abs(np.linalg.det(dR) - 1.0) < 1e-13 and np.abs(dR @ dR.T - np.eye(3)).max() < 1e-13


@pytest.fixture(scope="module")
def bases():
    femur, tgt = rs.femur_pair()
    out = {}
    for clutter, rho in ((False, 1.0), (True, 0.85)):
        tpl = rs.recovery_case(0, clutter)[0]
        out[clutter] = rs.icp_from(tpl, tgt, np.eye(3), np.zeros(3), 50, rho)[0]
    return out


@pytest.mark.parametrize("clutter,rho", [(False, 1.0), (True, 0.85)])
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_the_restatement_recovers_the_pose(bases, seed, clutter, rho):
    tpl, Y, R_true, _ = rs.recovery_case(seed, clutter)
    assert tpl.shape == ((478, 3) if clutter else (406, 3)) and Y.shape == (1622, 3)
    res = rs.search(tpl, Y, rs.rotation_samples(64), 10, rho)
    refined = rs.icp_from(tpl, Y, res["R"], res["t"], 50, rho)
    angle = rs.angle_deg(refined[0], R_true @ bases[clutter])
    print(f"seed {seed} clutter {clutter}: best {res['best']} score {res['score']:.4f} angle after refinement {angle:.3f} deg")
    assert not res["failed"].any() and angle <= 3.0


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert len(_native.SIGNATURES["gingr_rigid_search"][1]) == 14
    mk = open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()
    assert " rigid_search.hip" in mk and "rigid_search_plan.h" in mk


def test_rotation_samples_need_no_device():
    from gingr_amd import _native
    lib = _native.load()
    out = np.empty((64, 3, 3))
    assert lib.gingr_rotation_samples(64, _native.dptr(out)) == _native.GINGR_OK
    assert np.abs(out - rs.rotation_samples(64)).max() <= 1e-12
    assert lib.gingr_rotation_samples(0, _native.dptr(out)) != _native.GINGR_OK
    assert lib.gingr_rotation_samples(3, None) != _native.GINGR_OK


def test_python_surface():
    import gingr_amd as ga
    from gingr_amd import api, classic
    assert api.RigidSearchResult is ga.RigidSearchResult
    assert [f.name for f in __import__("dataclasses").fields(ga.RigidSearchResult)] == [
        "best", "R", "t", "score", "rotations", "translations", "scores", "kept", "failed"]
    p = inspect.signature(ga.Context.rigid_search).parameters
    assert (p["rotations"].default, p["iterations"].default, p["overlap"].default) == (64, 10, 1.0)
    p = inspect.signature(classic.GlobalRigidAlignment.__init__).parameters
    assert [(k, p[k].default) for k in ("starts", "iterations", "overlap", "maxPoints", "refineIterations")] == [
        ("starts", 64), ("iterations", 10), ("overlap", 1.0), ("maxPoints", 2000), ("refineIterations", 50)]
    tpl = np.arange(15003 * 3, dtype=np.float64).reshape(-1, 3)
    g = classic.GlobalRigidAlignment(None, tpl, maxPoints=2000)                               # fixed stride: ceil(15003 / 2000) = 8
    assert np.array_equal(g.searchPoints(), tpl[::8]) and g.searchPoints().shape[0] <= 2000
    assert np.array_equal(classic.GlobalRigidAlignment(None, tpl[:2000]).searchPoints(), tpl[:2000])
    assert classic.GlobalRigidAlignment(None, tpl[:2001]).searchPoints().shape[0] == 1001
