"""CPU tests of the feature-based global alignment: the plan header (gingr_amd/csrc/feature_align_plan.h) through a stand-alone C++
driver built with the address and undefined-behaviour sanitizers (tests/c/feature_align_plan_driver.cpp), the numpy restatement
(tests/feature_alignment_restatement.py) against itself in extended precision and on the partial recovery inputs, and the C ABI /
Python surface.

Measured with this file (2026-10-21).  Pair features of the femur target, k = 64, radius 25, float64 against longdouble: alpha
4.4e-16, phi 2.6e-16, theta 8.4e-15 at most over 92 486 counted pairs -- DELTA = 2^-46 = 1.42e-14 of the restatement covers it; no
pair lies within 16 DELTA of a bin edge, and both routes give the same tallies.
Recovery of the restatement itself on the partial femur (template femur[::4], the target's lower third cut away, seeds 0..7, radius
25, 2 000 triples, edge similarity 0.8, inlier distance 3, overlap 0.6, 30 refining iterations): the chosen hypothesis lies 3.2
degrees (plain) / 9.4 degrees (72 clutter points) from the true rotation, the refined pose 0.17 / 0.03 degrees from the pose trimmed
ICP reaches from the true alignment -- the same for every seed, the route being invariant under the motion up to rounding.  The bound
is the 3 degrees of tests/test_rigid_search_host.py, the spread of ICP's own fixed points.  The route it replaces (64 spiral starts,
10 iterations, overlap 0.6, the same refinement) ends 28 to 88 degrees away on these inputs."""
import ctypes
import dataclasses
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import feature_alignment_restatement as fa
from tests import rigid_search_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_cloud_fpfh", "gingr_feature_match", "gingr_rigid_poses_from_triples", "gingr_rigid_search_poses"]


# ------------------------------------------------------------------------------------------------------ the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("feature_align_plan") / "feature_align_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "feature_align_plan_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, check=True, text=True).stdout
    assert "FAIL" not in out and "ok 0" in out, out
    return out


def test_bins_equal_the_restatement_at_every_edge(driver):
    rows = [(kind, float.fromhex(f), int(b)) for kind, f, b in re.findall(r"bin (\w) (\S+) (-?\d+)", driver)]
    assert len(rows) >= 2 * (36 + 8)
    for kind, f, b in rows:
        v = np.array([f])
        zero = np.zeros(1)
        want = fa.bins_of(v, zero, zero)[0, 0] if kind == "c" else fa.bins_of(zero, zero, v)[0, 2]
        assert 0 <= b <= 10 and b == want, (kind, f, b, want)
    table = {(kind, f): b for kind, f, b in rows}
    assert table[("c", 0.0)] == 5 and table[("a", 0.0)] == 5 and table[("c", 1.0)] == 10 and table[("c", -1.0)] == 0
    assert table[("c", 1.5)] == 10 and table[("c", -1.5)] == 0 and table[("a", 1e300)] == 10 and table[("a", -1e300)] == 0


def test_argument_rules_of_the_descriptor_and_the_match(driver):
    rows = [(int(n), int(k), float.fromhex(r), int(c)) for n, k, r, c in re.findall(r"fpfh (\d+) (\d+) (\S+) (\d)", driver)]
    assert len(rows) == 7 * 7 * 6
    for N, k, r, code in rows:
        want = 1 if not (3 <= k <= 64 and k <= N) else (2 if not (r > 0.0 and np.isfinite(r)) else 0)
        assert code == want, (N, k, r)
    widths = {int(d): (int(ok), int(w)) for d, ok, w in re.findall(r"match (\d+) (\d) (\d+)", driver)}
    assert [widths[d][0] for d in (0, 1, 16, 33, 64, 65)] == [0, 1, 1, 1, 1, 0]
    assert [widths[d][1] for d in (1, 16, 17, 33, 40, 41, 64)] == [16, 16, 40, 40, 40, 64, 64]      # the padded widths hold the row


def test_match_chunks_are_whole_tiles_and_fill_the_device(driver):
    chunks = {(int(m), int(n)): (int(c), int(r)) for m, n, c, r in re.findall(r"chunks (\d+) (\d+) (\d+) (\d+)", driver)}
    assert len(chunks) == 8 * 10                                                               # (the driver checks the cover)
    assert chunks[(1, 1)] == (1, 32) and chunks[(3, 257)] == (9, 32) and chunks[(65, 64)] == (2, 32)
    assert chunks[(300, 1025)] == (33, 32)
    c, r = chunks[(2000, 50000)]
    assert c * 32 >= 2048 // 2 and c <= 2048 // 32 + 1 and r % 32 == 0                         # 32 row groups x 64 chunks
    assert chunks[(50000, 50000)][0] <= 3                                                      # many rows: no need to cut b


def test_degenerate_triangles_equal_the_restatement(driver):
    rows = re.findall(r"^tri (.*) (\d)$", driver, flags=re.M)
    assert len(rows) == 7
    got = []
    for coords, flag in rows:
        p = np.array([float.fromhex(v) for v in coords.split()]).reshape(3, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            a2, e4 = fa._area2_and_edge4(p)
            want = not a2 > fa.SKIP * e4
        assert bool(int(flag)) == want, coords
        got.append(int(flag))
    assert got == [0, 1, 1, 0, 1, 1, 0]


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def femur_descriptor():
    _, tgt = rs.femur_pair()
    n = fa.normals(tgt, 12, tgt.mean(0))
    return tgt, n, fa.fpfh(tgt, n, 64, 25.0), fa.fpfh(tgt, n, 64, 25.0, np.longdouble)


def test_float64_against_longdouble_and_no_edge_near_pair(femur_descriptor):
    tgt, n, a, b = femur_descriptor
    ok = a["counted"]
    assert np.array_equal(ok, b["counted"]) and np.array_equal(a["neighbour"], b["neighbour"]) and ok.sum() > 50000
    delta = {f: float(np.abs(a[f][ok].astype(np.longdouble) - b[f][ok]).max()) for f in ("alpha", "phi", "theta")}
    print("largest float64 / longdouble difference of a pair feature on the femur target:", delta, "DELTA", fa.DELTA)
    assert max(delta.values()) <= fa.DELTA
    near = fa.edge_near(a["alpha"], a["phi"], a["theta"]) & ok
    print(f"edge-near pairs: {int(near.sum())} of {int(ok.sum())}")
    assert near.sum() == 0                                                                   # the restatement flags none on the fixture
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["valid"], b["valid"])
    # 65 non-negative terms with a square root and a division each, a rescaling over 11: the bound of the GPU test
    worst = float(np.abs(a["fpfh"].astype(np.longdouble) - b["fpfh"]).max())
    print(f"fpfh float64 / longdouble: {worst:.3g}")
    assert worst <= 100 * 256 * 2.0 ** -53
    third = a["fpfh"].reshape(-1, 3, 11).sum(2)
    assert np.all((np.abs(third - 100.0) <= 1e-11) | (third == 0.0))                          # every third sums to 100 or is empty
    assert (a["counts"].reshape(-1, 3, 11).sum(2) == a["valid"][:, None]).all()


def test_descriptor_small_cases():
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.zeros((64, 1))], axis=1)
    up = np.tile([0.0, 0.0, 1.0], (64, 1))
    d = fa.fpfh(flat, up, 64, 3.0)
    assert (d["valid"] > 0).all()
    centre = np.zeros(33, dtype=bool)
    centre[[5, 16, 27]] = True
    assert (d["counts"][:, ~centre] == 0).all() and (d["counts"][:, centre] == d["valid"][:, None]).all()
    assert np.abs(d["fpfh"] - np.where(centre, 100.0, 0.0)[None]).max() <= 100 * 256 * 2.0 ** -53 and (d["fpfh"][:, ~centre] == 0).all()
    # a neighbour exactly along the normal: dn x u = 0, the pair is skipped in both directions
    x = np.array([[0.0, 0, 0], [0, 0, 2.0], [3.0, 0, 0], [0, 4.0, 0]])
    d = fa.fpfh(x, np.tile([0.0, 0.0, 1.0], (4, 1)), 3, 10.0)
    assert d["neighbour"][0].sum() == 2 and d["valid"][0] == 1 and d["idx"][0].tolist() == [0, 1, 2] and not d["counted"][0, 1]
    # a radius below the smallest spacing, duplicates, zero normals
    assert fa.fpfh(flat, up, 64, 0.5)["valid"].sum() == 0 and not fa.fpfh(flat, up, 64, 0.5)["fpfh"].any()
    dup = np.concatenate([flat, flat[:4]])
    d = fa.fpfh(dup, np.concatenate([up, up[:4]]), 64, 3.0)
    assert (d["d2"][[0, 64], :2] == 0).all() and not d["neighbour"][[0, 64], :2].any()         # itself and its copy drop out
    none = up.copy()
    none[::3] = 0.0
    d = fa.fpfh(flat, none, 64, 3.0)
    assert (d["valid"][::3] == 0).all() and (d["valid"][1::3] > 0).all() and (d["valid"][1] < fa.fpfh(flat, up, 64, 3.0)["valid"][1])
    assert np.array_equal(fa.unit_normals([[0, 0, 5.0], [0, 0, 0], [3.0, 4.0, 0]]), [[0, 0, 1.0], [0, 0, 0], [0.6, 0.8, 0]])


def test_match_ties_and_exact_rows():
    rng = np.random.default_rng(3)
    b = rng.normal(size=(40, 33))
    b[17] = b[5]
    b[30] = b[5]
    a = np.stack([b[5], b[39], b[5] + 1e-9])
    idx, d2 = fa.feature_match(a, b)
    assert idx.tolist() == [5, 39, 5] and d2[0] == 0.0 and d2[1] == 0.0 and d2[2] > 0.0
    acc = 0.0
    for c in range(33):
        acc = acc + (a[2, c] - b[5, c]) * (a[2, c] - b[5, c])
    assert d2[2] == acc                                                                      # the bits of the scalar expression


def test_triples_exact_copy_and_degenerate():
    rng = np.random.default_rng(5)
    X = rng.normal(0, 30.0, (20, 3)) + [100.0, -20.0, 40.0]
    R, t = rs.random_rotation(rng), np.array([-50.0, 10.0, 200.0])
    Y = X @ R.T + t
    tri = np.array([[0, 1, 2], [3, 9, 17], [4, 4, 5], [6, 7, 8]])
    tt = tri.copy()
    tt[3] = [6, 7, 7]
    poses, deg = fa.poses_from_triples(X, Y, tri, tt)
    assert deg.tolist() == [False, False, True, True] and np.isnan(poses[2:]).all()
    for h in (0, 1):
        assert np.abs(poses[h, :9].reshape(3, 3) - R).max() < 1e-12 and np.abs(poses[h, 9:] - t).max() < 1e-9
    long_, _ = fa.poses_from_triples(X, Y, tri[:2], tt[:2], np.longdouble)
    assert np.abs(long_.astype(np.float64) - poses[:2]).max() < 1e-9
    line = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 0]])
    assert fa.poses_from_triples(line, line, [[0, 1, 2]], [[0, 1, 3]])[1].tolist() == [True]    # collinear in the moving cloud


def test_selection_rule():
    scores, failed = np.array([2.0, 1.0, 1.0, 0.5, 3.0]), np.array([False, False, False, True, False])
    assert fa.select_best(scores, np.array([5, 7, 7, 9, 7]), failed, 1) == 1                 # most inliers, smaller score, lowest index
    assert fa.select_best(scores, np.array([5, 7, 7, 9, 8]), failed, 1) == 4
    assert fa.select_best(scores, np.array([5, 7, 7, 9, 8]), failed, 0) == 1
    assert fa.select_best(scores, np.zeros(5, int), np.ones(5, bool), 1) == -1


@pytest.fixture(scope="module")
def bases():
    part = fa.partial_target(rs.femur_pair()[1])
    return {clutter: rs.icp_from(rs.recovery_case(0, clutter)[0], part, np.eye(3), np.zeros(3), 50, 0.6)[0] for clutter in (False, True)}


@pytest.fixture(scope="module")
def old_route():
    """angle after the route this replaces, per (seed, clutter): rs.search over 64 spiral rotations, 10 iterations, overlap 0.6, plus
    the same refinement"""
    return {}


@pytest.mark.parametrize("clutter", [False, True])
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_the_restatement_recovers_the_partial_pose(bases, old_route, seed, clutter):
    tpl, Y, R_true, _, part = fa.partial_case(seed, clutter)
    assert tpl.shape == ((478, 3) if clutter else (406, 3)) and Y.shape[0] == part.shape[0] < 1622 * 0.75
    res = fa.align(tpl, Y, 25.0, hypotheses=2000, edge_similarity=0.8, inlier_distance=3.0, overlap=0.6, refine_iterations=30)
    hyp, angle = rs.angle_deg(res["hypothesis"][0], R_true), rs.angle_deg(res["R"], R_true @ bases[clutter])
    old = rs.search(tpl, Y, rs.rotation_samples(64), 10, 0.6)
    old_route[(seed, clutter)] = rs.angle_deg(rs.icp_from(tpl, Y, old["R"], old["t"], 30, 0.6)[0], R_true @ bases[clutter])
    print(f"seed {seed} clutter {clutter}: hypothesis {hyp:.2f} deg from the truth, refined {angle:.3f} deg from the base pose; "
          f"spiral starts + refinement {old_route[(seed, clutter)]:.2f} deg; {res['info']}")
    assert angle <= 3.0


def test_the_centroid_route_misses_these_inputs(old_route):
    """the gap this closes: 64 spiral rotations, 10 iterations at overlap 0.6 and the same refinement miss by more than 3 degrees on at
    least one seed (here: on every one)"""
    if len(old_route) < 2 * len(rs.SEEDS):                                                   # (run alone: measure it here)
        part = fa.partial_target(rs.femur_pair()[1])
        for clutter in (False, True):
            base = rs.icp_from(rs.recovery_case(0, clutter)[0], part, np.eye(3), np.zeros(3), 50, 0.6)[0]
            for seed in rs.SEEDS:
                tpl, Y, R_true, _, _ = fa.partial_case(seed, clutter)
                old = rs.search(tpl, Y, rs.rotation_samples(64), 10, 0.6)
                old_route[(seed, clutter)] = rs.angle_deg(rs.icp_from(tpl, Y, old["R"], old["t"], 30, 0.6)[0], R_true @ base)
    for clutter in (False, True):
        angles = [old_route[(seed, clutter)] for seed in rs.SEEDS]
        print(f"clutter {clutter}: spiral starts + refinement, degrees from the base pose: {[round(a, 1) for a in angles]}")
        assert max(angles) > 3.0


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert [len(_native.SIGNATURES[f][1]) for f in FUNCTIONS] == [10, 8, 10, 17]
    mk = open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()
    assert " feature_align.hip" in mk and "feature_align_plan.h" in mk and "rigid_step.h" in mk
    common = open(os.path.join(ROOT, "gingr_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define GINGR_TIMERS (\d+)", common).group(1)) >= 30                # hooks 27 / 28 / 29
    header = open(os.path.join(ROOT, "gingr_amd", "csrc", "feature_align.hip")).read()
    assert "THIS\n// PACKAGE'S DEFINITION" in header or "PACKAGE'S DEFINITION" in header


def test_python_surface():
    import gingr_amd as ga
    from gingr_amd import api, classic
    assert api.RigidSearchPosesResult is ga.RigidSearchPosesResult and issubclass(ga.RigidSearchPosesResult, ga.RigidSearchResult)
    assert [f.name for f in dataclasses.fields(ga.RigidSearchPosesResult)][-1] == "inliers"
    z = np.zeros(1)
    plain = ga.RigidSearchPosesResult(0, np.eye(3), np.zeros(3), 0.0, z, z, z, z, z)           # constructed as before: the field is defaulted
    assert plain.inliers is None
    p = inspect.signature(ga.Context.cloud_fpfh).parameters
    assert p["k"].default == 64 and list(p)[:5] == ["self", "points", "normals", "k", "radius"]
    p = inspect.signature(ga.Context.rigid_search_poses).parameters
    assert list(p) == ["self", "moving", "target", "poses", "iterations", "overlap", "inlierDistance", "select"]
    assert list(inspect.signature(ga.Context.feature_match).parameters) == ["self", "a", "b"]
    assert hasattr(ga.Context, "rigid_poses_from_triples")
    p = inspect.signature(classic.FeatureRigidAlignment.__init__).parameters
    assert [(k, p[k].default) for k in list(p)[4:]] == [
        ("normalsK", 12), ("descriptorK", 64), ("hypotheses", 2000), ("edgeSimilarity", 0.8), ("inlierDistance", None), ("overlap", 0.6),
        ("refineIterations", 30), ("maxPoints", 2000), ("seed", 0), ("templateNormals", None)]
    assert list(p)[:4] == ["self", "ctx", "template", "radius"] and p["radius"].default is inspect.Parameter.empty
    tpl = np.arange(15003 * 3, dtype=np.float64).reshape(-1, 3)
    f = classic.FeatureRigidAlignment(None, tpl, 25.0)
    assert np.array_equal(f.searchPoints(), classic.GlobalRigidAlignment(None, tpl).searchPoints())
    assert "unmeasured" in classic.FeatureRigidAlignment.__doc__.lower()
    assert "FeatureRigidAlignment" in classic.GlobalRigidAlignment.__doc__
    with pytest.raises(ValueError):
        classic.FeatureRigidAlignment(None, tpl, 0.0)
