"""CPU pins of gingr_mesh_decimate, before any kernel runs:

1. tests/decimate_restatement.py -- the algorithm as plain loops in the kernels' order -- returns exactly what the definition
   gingr_amd.simple.cluster_decimate returns (np.array_equal on vertices and cells) on every case of the device test's table, at sizes
   a Python loop can afford; this pins the order of the arithmetic;
2. gingr_amd/csrc/decimate_bisect.h, the one home of the cube-size recurrence and of the cell key, compiled for the host with the
   address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/decimate_bisect_driver.cpp) and fed tables of
   (extent, count sequence, n_target): the cube sizes it asks for, the one it chooses and its step count are the Python recurrence's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gingr_amd.simple import cluster_decimate
from tests import decimate_restatement as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def same(vertices, cells, n_target):
    want_v, want_c = cluster_decimate(vertices, cells, n_target)
    got_v, got_c = dr.cluster_decimate(vertices, cells, n_target)
    assert got_v.dtype == want_v.dtype and np.array_equal(got_v, want_v), (n_target, got_v.shape, want_v.shape)
    if cells is None:
        assert got_c is None and want_c is None
    else:
        assert got_c.dtype == want_c.dtype == np.int32 and got_c.shape == want_c.shape and np.array_equal(got_c, want_c), n_target
    return got_v, got_c


@pytest.fixture(scope="module")
def femur():
    return dr.femur()


@pytest.mark.parametrize("n_target", dr.FEMUR_TARGETS)
def test_femur(femur, n_target):
    v, c = femur
    assert v.shape == (1622, 3) and c.shape == (3240, 3)
    got_v, got_c = same(v, c, n_target)
    if n_target >= 1622:
        assert np.array_equal(got_v, v) and np.array_equal(got_c, c)
    else:
        assert n_target <= got_v.shape[0] < 1622


def test_femur_as_a_point_cloud(femur):
    same(femur[0], None, 400)


@pytest.mark.parametrize("n", dr.CLOUD_SIZES)
def test_random_clouds(n):
    for n_target in dr.cloud_targets(n):
        same(dr.cloud(n), None, n_target)


@pytest.mark.parametrize("shifted", (False, True))
def test_lattice_ties_go_to_the_lowest_index(shifted):
    v = dr.lattice(shifted)
    sizes = []
    for n_target in dr.LATTICE_TARGETS:
        got_v, _ = same(v, None, n_target)
        sizes.append(got_v.shape[0])
    assert sizes == [8, 27, 125]              # the count is a step function of the cube size: the next value above 100 is 5^3


def test_no_cube_size_is_accepted():
    v = dr.repeated_positions()
    got_v, _ = same(v, None, 100)
    assert got_v.shape[0] == np.unique(v, axis=0).shape[0] == 40
    _, h, = dr.decimate(v, None, 100)[1:]
    assert h == float(np.max(v.max(0) - v.min(0))) * 1e-6      # the cells of lo


@pytest.mark.parametrize("kind,n_target", dr.DEGENERATE)
def test_degenerate_extents(kind, n_target):
    got_v, _ = same(dr.degenerate(kind), None, n_target)
    if kind == "identical":
        assert got_v.shape[0] == 1


def test_repeated_and_collapsing_triangles():
    v, tri = dr.repeated_triangles()
    got_v, got_c = same(v, tri, 6)
    assert got_v.shape[0] == 6
    # the groups are far apart: a vertex's cluster is the kept vertex nearest to it.  Rows 1, 2 repeat row 0, rows 6, 7 collapse,
    # row 8 repeats row 3 and row 10 repeats row 9: the first of every corner set stays, with its own winding, in the original order
    nearest = ((v[:, None, :] - got_v[None, :, :]) ** 2).sum(-1).argmin(1)
    assert np.array_equal(nearest, np.repeat(np.arange(6), 4))                 # the design: one cluster per group
    assert np.array_equal(got_c, nearest[tri[[0, 3, 4, 5, 9]]])
    # untouched by the identity: all eleven stay, the repeated ones included
    _, all_c = same(v, tri, v.shape[0])
    assert np.array_equal(all_c, tri)


@pytest.mark.parametrize("n_target", (30, 200))
def test_grid_surface_small(n_target):
    v, tri = dr.grid_surface(24)
    assert v.shape[0] == 576 and tri.shape[0] == 2 * 23 * 23
    same(v, tri, n_target)


# ------------------------------------------------------------------------------------------------------------------ the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("decimate") / "decimate_bisect_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "decimate_bisect_driver.cpp"), "-o", str(exe)])
    return str(exe)


def bisect_tables():
    rng = np.random.default_rng(11)
    tables = []
    for k in range(300):
        e = rng.uniform(0.0, 1.0, 3) * 10.0 ** rng.integers(-6, 7)
        if k % 10 == 0:
            e[:] = 0.0                                        # extent 0 -> 1
        n_target = int(rng.integers(1, 5000))
        kind = k % 4
        if kind == 0:
            counts = rng.integers(0, 2 * n_target + 1, 60)    # any sequence at all
        elif kind == 1:
            counts = np.full(60, n_target - 1)                # never accepted
        elif kind == 2:
            counts = np.full(60, n_target)                    # always accepted
        else:
            counts = np.sort(rng.integers(0, 2 * n_target + 1, 60))[::-1]
        tables.append((e, n_target, [int(c) for c in counts]))
    return tables


def test_bisection_header_against_the_python_recurrence(driver):
    tables = bisect_tables()
    raw = b"".join(np.array([*e, n_target, len(counts), *counts], dtype=np.float64).tobytes() for e, n_target, counts in tables)
    out = subprocess.run([driver, "bisect"], input=raw, capture_output=True, check=True).stdout
    res = np.frombuffer(out, dtype=np.float64).reshape(len(tables), 64)
    taken = set()
    for (e, n_target, counts), r in zip(tables, res):
        extent = float(np.max(e)) or 1.0
        h, steps, accepted, mids = dr.bisect(extent, counts, n_target)
        assert r[0] == extent and r[1] == h and int(r[2]) == steps and bool(r[3]) == accepted
        assert np.array_equal(r[4:4 + steps], np.array(mids)) and not r[4 + steps:].any()
        taken.add(steps)
    assert taken == {15}, taken      # hi / lo takes its square root whichever way a step goes: 2e6 -> below 1.0005 in 15 steps


def test_cell_key_header(driver):
    rng = np.random.default_rng(12)
    rows = []
    for _ in range(2000):
        lo = rng.normal(0.0, 1.0, 3) * 10.0 ** rng.integers(-3, 7)
        extent = 10.0 ** rng.uniform(-3, 4)
        h = extent * 10.0 ** rng.uniform(-6, 0.3)
        p = lo + rng.uniform(0.0, 1.0, 3) * extent
        p = np.maximum(p, lo)
        rows.append([*p, *lo, h])
    rows.append([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1e-6])          # the largest index an axis can have
    rows = np.array(rows, dtype=np.float64)
    out = subprocess.run([driver, "key"], input=rows.tobytes(), capture_output=True, check=True).stdout
    keys = np.frombuffer(out, dtype=np.uint64)
    want = np.array([dr.cell_key(r[:3], r[3:6], r[6]) for r in rows], dtype=np.uint64)
    assert np.array_equal(keys, want)
    cell = np.floor((rows[:, :3] - rows[:, 3:6]) / rows[:, 6:7]).astype(np.int64)
    assert cell.min() >= 0 and cell.max() < 2 ** 20
    assert np.array_equal(keys, (cell[:, 0] | (cell[:, 1] << 21) | (cell[:, 2] << 42)).astype(np.uint64))
    assert not (keys >> np.uint64(63)).any()                   # never the table's empty mark
