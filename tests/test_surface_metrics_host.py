"""CPU side of the surface-distance model metrics (gingr_amd/csrc/surface_metrics.hip): the planner (surface_metrics_plan.h) compiled for
the host with the address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/surface_metrics_plan_driver.cpp) -- the
column blocks, mesh chunks and partial layout cover every (set, mesh) pair once, the seed table on a strip, an isolated vertex and a fan
-- the numpy restatement (tests/surface_metrics_restatement.py) against hand-worked cases on a two-triangle mesh, the argmin cap of the
GPU specificity test, and the three entries in the header, the loader and the Python layer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import model_metrics_restatement as mm
from tests import surface_metrics_restatement as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_mesh_set_distances", "gingr_model_generalization_surface", "gingr_model_specificity_surface"]


# ---------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("surface_metrics_plan") / "surface_metrics_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "surface_metrics_plan_driver.cpp"),
                           "-o", str(exe)])

    def run(*case):
        out = subprocess.run([str(exe)] + [str(c) for c in case], capture_output=True, check=True, text=True).stdout.split("\n")
        return [line.split() for line in out if line.strip()]
    return run


@pytest.mark.parametrize("n_sets,n_meshes,points", [(1, 1, 1), (16, 17, 15), (17, 16, 16), (17, 1, 17), (513, 3, 130), (1025, 2, 1622),
                                                   (2, 4097, 33), (512, 512, 50000), (3, 5, 1 << 20)])
@pytest.mark.parametrize("pairing", [0, 1])
def test_blocks_chunks_and_partials_cover_every_pair_once(plan_driver, n_sets, n_meshes, pairing, points):
    rows = plan_driver("cover", n_sets, n_meshes, pairing, points)
    seen, launch, used, slabs_rows = set(), None, None, []

    def close_launch():
        if launch is None:
            return
        set0, sets, mesh0, meshes, pairs, per_slab, slabs, partial = launch
        assert 1 <= sets <= 512 and 1 <= meshes and pairs == (sets * meshes if pairing == 0 else sets)
        assert pairing == 1 or meshes <= 4096
        assert per_slab % 16 == 0 and partial == slabs * pairs * 2 <= 1 << 24
        assert len(slabs_rows) == slabs >= 1 and slabs_rows[0][0] == 0 and slabs_rows[-1][1] == points
        for s, (b, e) in enumerate(slabs_rows):
            assert b == s * per_slab and b < e <= b + per_slab and (s == 0 or slabs_rows[s - 1][1] == b)
        assert len(used) == 2 * pairs and max(used) < partial, "two pairs share a partial, or one lies outside"

    for row in rows:
        kind, v = row[0], [int(x) for x in row[1:]]
        if kind == "L":
            close_launch()
            launch, used, slabs_rows = v, set(), []
        elif kind == "S":
            slabs_rows.append(v)
        else:
            s, m, pr, first, last = v
            assert (s, m) not in seen and 0 <= pr < launch[4]
            seen.add((s, m))
            assert first == 2 * pr and last == ((launch[6] - 1) * launch[4] + pr) * 2 + 1
            used.update((first, last) if launch[6] > 1 else (first, first + 1))
            assert launch[0] <= s < launch[0] + launch[1]
            assert (launch[2] <= m < launch[2] + launch[3]) if pairing == 0 else m == s % n_meshes
    close_launch()
    want = {(s, m) for s in range(n_sets) for m in range(n_meshes)} if pairing == 0 else {(s, s % n_meshes) for s in range(n_sets)}
    if len(want) <= 1 << 16:
        assert seen == want
    else:
        assert len(seen) == len(want)


def test_slabs_aim_at_the_target_and_fit_the_partials(plan_driver):
    one = plan_driver("cover", 1, 1, 0, 50000)[0]
    assert int(one[7]) == 3125 and int(one[6]) == 16, "one pair: one slab per group of 16 queries"
    big = plan_driver("cover", 512, 512, 0, 50000)[0]
    assert int(big[7]) == 1 and int(big[8]) == 2 * 512 * 512
    assert int(plan_driver("bytes", 100, 10, 50, 4, 300, 0)[0][0]) == (4 * (150 + 60) + 10 * 300 + (1 << 24)) * 8 + (900 + 100) * 4


def seeds(plan_driver, nv, cells):
    cells = np.asarray(cells).reshape(-1, 3)
    return [int(v) for v in plan_driver("seeds", nv, cells.shape[0], *cells.ravel().tolist())[0]]


def test_seed_table_on_a_strip(plan_driver):
    """vertices 0..5 in two rows, triangles (0,1,3) (1,4,3) (1,2,4) (2,5,4): every vertex starts from its lowest-numbered triangle"""
    assert seeds(plan_driver, 6, [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4]]) == [0, 0, 2, 0, 1, 3]


def test_seed_table_with_an_isolated_vertex(plan_driver):
    assert seeds(plan_driver, 5, [[0, 1, 3], [1, 4, 3]]) == [0, 0, -1, 0, 1]


def test_seed_table_on_a_fan(plan_driver):
    """the hub 0 has seven triangles, listed from the highest rim vertex down: its seed is triangle 0 all the same, and a rim vertex
    takes the lower of its two"""
    fan = [[0, k, k + 1] for k in range(7, 0, -1)]
    got = seeds(plan_driver, 9, fan)
    assert got[0] == 0 and got[8] == 0 and got[1] == 6
    assert got == [0] + [min(t for t, c in enumerate(fan) if v in c) for v in range(1, 9)]


# ------------------------------------------------------------------------------------------------------------ the restatement
SQUARE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
SQUARE_CELLS = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def test_restatement_by_hand_on_two_triangles():
    """the unit square cut along its diagonal: above a face the height; beside an edge and beyond a corner the distance to them; on
    the surface (face, shared edge, corner) exactly 0"""
    q = np.array([[0.75, 0.25, 2.0],      # above the face of triangle 0: 2
                  [0.5, -3.0, 4.0],       # beside the edge y = 0: hypot(3, 4) = 5
                  [4.0, 5.0, 0.0],        # beyond the corner (1, 1): hypot(3, 4) = 5
                  [-2.0, -3.0, 6.0],      # beyond the corner (0, 0): 7
                  [0.25, 0.75, 0.0],      # on the face of triangle 1
                  [0.5, 0.5, 0.0],        # on the shared diagonal
                  [1.0, 0.0, 0.0]])       # a corner
    d = sm.distances(q, SQUARE, SQUARE_CELLS)
    assert np.array_equal(d, [2.0, 5.0, 5.0, 7.0, 0.0, 0.0, 0.0])
    avg, mx = sm.avg_max(q, SQUARE, SQUARE_CELLS)
    assert avg == 19.0 / 7.0 and mx == 7.0
    a, m = sm.set_distances(np.stack([q[:4], q[3:]]), np.stack([SQUARE, SQUARE + [0.0, 0.0, 1.0]]), SQUARE_CELLS)
    assert np.array_equal(a[:, 0], [19.0 / 4.0, 7.0 / 4.0]) and np.array_equal(m[:, 0], [7.0, 7.0])
    assert a[0, 1] == (1.0 + np.hypot(3.0, 3.0) + np.hypot(5.0, 1.0) + np.sqrt(4 + 9 + 25)) / 4.0
    ac, mc = sm.set_distances(np.stack([q[:4], q[3:], q[:4]]), np.stack([SQUARE, SQUARE + [0.0, 0.0, 1.0]]), SQUARE_CELLS, "cyclic")
    assert np.array_equal(ac, [a[0, 0], a[1, 1], a[0, 0]]) and np.array_equal(mc, [m[0, 0], m[1, 1], m[0, 0]])


def test_surface_distance_is_blind_to_sliding_and_the_vertex_distance_is_not():
    pts, cells = sm.grid_mesh(5, 4)
    moved = pts.copy()
    inner = (pts[:, 0] > 0) & (pts[:, 0] < 4) & (pts[:, 1] > 0) & (pts[:, 1] < 3)
    moved[inner] += [0.3, -0.2, 0.0]
    assert sm.avg_max(moved, pts, cells) == (0.0, 0.0)
    assert np.linalg.norm(moved - pts, axis=1).max() > 0.3


def test_restated_generalization_and_specificity_on_a_model():
    """rank 2 on two triangles: a shape that is an instance comes back within the ridge's bias, whatever the measure; the specificity
    minimum is 0 at a training shape that is the sample itself and goes to the lower of two identical shapes"""
    mo = mm.Model(SQUARE * 10.0, np.zeros((4, 3)), np.linalg.qr(np.random.default_rng(0).normal(size=(12, 2)))[0], np.array([4.0, 1.0]))
    alphas = np.array([[1.0, -0.5], [0.0, 0.0]])
    x = np.asarray(mm.instances(mo, alphas), dtype=np.float64)
    coef, avg, mx = sm.generalization(mo, x, SQUARE_CELLS, [1, 2])
    assert avg.shape == (2, 2) and float(avg[1].max()) < 1e-4 and float(avg[0, 0]) > float(avg[1, 0])
    train = np.stack([x[1], x[1], x[0]])
    means, mn, am = sm.specificity(mo, train, alphas, SQUARE_CELLS, [2])
    assert am.tolist() == [[2, 0]] and np.array_equal(mn, [[0.0, 0.0]]) and means[0, 1, 0] == means[0, 1, 1] == 0.0


def test_bounds():
    assert sm.summation_term(1 << 20, 2.0) == (1 << 20) * 2.0 ** -53 / (1 - (1 << 20) * 2.0 ** -53) * 2.0
    mo, _ = sm.grid_model(5, 4, 3, 1)
    a = np.random.default_rng(0).standard_normal((4, 3))
    b = sm.query_bound(mo, a)
    assert b.shape == (4,) and np.all(b >= mm.instance_bound(mo, a).reshape(4, -1).max(axis=1)) and float(b.max()) < 1e-12


def test_argmin_cap_of_the_gpu_specificity_test_leaves_out_few_samples():
    """tests/test_gpu_surface_metrics.py requires the device's argmin only where the runner-up lies outside twice the bound: with that
    test's model, shapes and seeds the restatement alone must leave at least 95 % of the samples in"""
    mo, cells, train, alphas, ranks = sm.specificity_block_case()
    means, mn, am = sm.specificity(mo, train, alphas, cells, ranks)
    out = 0
    for q, k in enumerate(ranks):
        bound = sm.query_bound(mo, mm.truncated(alphas, k))[:, None] + sm.summation_term(mo.M, means[q])
        order = np.argsort(means[q], axis=1, kind="stable")
        pick = np.arange(means.shape[1])
        gap = means[q][pick, order[:, 1]] - means[q][pick, order[:, 0]]
        out += int(np.count_nonzero(gap <= 2.0 * np.maximum(bound[pick, order[:, 0]], bound[pick, order[:, 1]])))
        assert np.array_equal(am[q], order[:, 0]) and np.array_equal(mn[q], means[q][pick, order[:, 0]])
    total = len(ranks) * alphas.shape[0]
    print(f"samples whose argmin the cap leaves out: {out} of {total} ({100.0 * out / total:.2f} %), cap 5 %")
    assert out <= 0.05 * total


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entries_are_declared_bound_and_exported():
    import ctypes
    from gingr_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in FUNCTIONS:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    common = open(os.path.join(ROOT, "gingr_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define GINGR_TIMERS (\d+)", common).group(1)) >= 24      # hook 23: the batched scan
    assert "surface_metrics.hip" in open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()


def test_python_layer_names_and_defaults():
    import inspect
    import gingr_amd as ga
    from gingr_amd import metrics
    assert callable(ga.Context.mesh_set_distances)
    for fn in (ga.DeviceModel.project, ga.ModelMetrics.generalization, ga.ModelMetrics.specificity):
        p = inspect.signature(fn).parameters
        assert p["distance"].default == "vertex" and p["cells"].default is None
    assert "distance" not in inspect.signature(ga.ModelMetrics.generalizationLeaveOneOut).parameters
    res = metrics.GeneralizationResult(np.array([1]), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2, 1)))
    spec = metrics.SpecificityResult(np.array([1]), np.zeros((1, 3)), np.zeros((1, 3), dtype=np.int64), np.zeros((3, 1)))
    assert res.distance == spec.distance == "vertex"
    assert [f.name for f in __import__("dataclasses").fields(res)] == ["ranks", "avg", "max", "coefficients", "distance"]
    assert [f.name for f in __import__("dataclasses").fields(spec)] == ["ranks", "min_avg", "argmin", "alphas", "distance"]


def test_surface_distance_needs_cells():
    import gingr_amd as ga
    dm = ga.DeviceModel.__new__(ga.DeviceModel)
    dm.host = ga.PointDistributionModel(np.zeros((2, 3)), np.zeros((2, 3)), np.eye(6)[:, :1], np.array([1.0]))
    dm.handle = None
    assert dm._surface_cells("vertex", None) is None
    with pytest.raises(ValueError, match="cells"):
        dm._surface_cells("surface", None)
    with pytest.raises(ValueError, match="distance"):
        dm._surface_cells("closest", None)
    got = dm._surface_cells("surface", [[0, 1, 0]])
    assert got.dtype == np.int32 and got.shape == (1, 3)
