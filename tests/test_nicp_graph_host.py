"""CPU pin of gingr_amd/csrc/nicp_graph.h, the host side of the sparse N-ICP step: the header compiled for the host with the address and
undefined-behaviour sanitizers into a stand-alone driver (tests/c/nicp_graph_driver.cpp) and fed edge lists; its CSR adjacency,
degrees, component labels and its verdict on unanchored components are those of the numpy restatement
(tests/nicp_pcg_restatement.py: graph, unanchored_component), and it refuses what the C ABI refuses."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import nicp_pcg_restatement as nr
from tests.test_gpu_nicp import sphere_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
OK, BAD_EDGE, DUPLICATE = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("nicp_graph") / "nicp_graph_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "nicp_graph_driver.cpp"), "-o", str(exe)])
    return str(exe)


def run(driver, n, edges, has_term=None):
    edges = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    has_term = np.ones(n, dtype=np.int32) if has_term is None else np.asarray(has_term, dtype=np.int32)
    raw = np.concatenate([[n, edges.shape[0]], edges.ravel(), has_term]).astype(np.int32).tobytes()
    out = np.frombuffer(subprocess.run([driver], input=raw, capture_output=True, check=True).stdout, dtype=np.int32)
    status, bad, ncomp, unanchored = (int(v) for v in out[:4])
    if status != OK:
        assert out.shape[0] == 4
        return status, bad, None
    E = edges.shape[0]
    assert out.shape[0] == 4 + (n + 1) + 2 * E + n + n
    row_ptr, col, degree, component = np.split(out[4:], np.cumsum([n + 1, 2 * E, n]))
    return status, bad, (row_ptr, col, degree, component, ncomp, unanchored)


def hull_edges(n, seed):
    from gingr_amd.classic import nicp_edges
    return nicp_edges(sphere_mesh(n, seed)[1])


def same_as_numpy(driver, n, edges, has_term=None):
    status, _, got = run(driver, n, edges, has_term)
    assert status == OK
    row_ptr, col, degree, component = nr.graph(n, edges)
    for g, w in zip(got[:4], (row_ptr, col, degree, component)):
        assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w)
    assert got[4] == int(component.max()) + 1
    assert got[5] == nr.unanchored_component(component, np.ones(n) if has_term is None else has_term)
    return got


def test_tetrahedron(driver):
    edges = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    row_ptr, col, degree, component, ncomp, unanchored = same_as_numpy(driver, 4, edges)
    assert np.array_equal(row_ptr, [0, 3, 6, 9, 12]) and np.array_equal(col, [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2])
    assert np.array_equal(degree, [3, 3, 3, 3]) and np.array_equal(component, [0, 0, 0, 0]) and ncomp == 1 and unanchored == -1
    # the rows come out ascending whatever the order of the edge list
    shuffled = same_as_numpy(driver, 4, edges[::-1])
    assert np.array_equal(shuffled[1], col)


def test_two_hulls_and_an_isolated_vertex(driver):
    a, b = hull_edges(30, 1), hull_edges(47, 2)
    n = 30 + 1 + 47                                              # the isolated vertex sits between the hulls: labels follow the lowest vertex
    edges = np.concatenate([a, b + 31])
    rng = np.random.default_rng(3)
    edges = edges[rng.permutation(edges.shape[0])]
    row_ptr, col, degree, component, ncomp, unanchored = same_as_numpy(driver, n, edges)
    assert ncomp == 3 and np.array_equal(component, np.concatenate([np.zeros(30), [1], np.full(47, 2)]))
    assert degree[30] == 0 and row_ptr[30] == row_ptr[31] and degree.sum() == 2 * edges.shape[0]
    # which component has no data term: none / the isolated vertex / the second hull / the first of two
    has = np.ones(n, dtype=np.int32)
    has[30] = 0
    assert same_as_numpy(driver, n, edges, has)[5] == 1
    has[30], has[31:] = 1, 0
    assert same_as_numpy(driver, n, edges, has)[5] == 2
    has[:] = 0
    has[50] = 1
    assert same_as_numpy(driver, n, edges, has)[5] == 0


def test_hull_220(driver):
    edges = hull_edges(220, 0)
    assert edges.shape[0] == 3 * 220 - 6                          # a closed genus-0 triangulation
    row_ptr, col, degree, component, ncomp, unanchored = same_as_numpy(driver, 220, edges)
    assert ncomp == 1 and degree.min() >= 3 and unanchored == -1
    # symmetric: j in row i <=> i in row j
    pairs = {(i, int(j)) for i in range(220) for j in col[row_ptr[i]:row_ptr[i + 1]]}
    assert all((j, i) in pairs for i, j in pairs) and len(pairs) == 2 * edges.shape[0]


@pytest.mark.parametrize("edges,status,bad", [
    ([[0, 1], [3, 2]], BAD_EDGE, 1),               # p1 > p2
    ([[2, 2]], BAD_EDGE, 0),                       # p1 == p2
    ([[0, 1], [1, 2], [2, 5]], BAD_EDGE, 2),       # id out of range
    ([[-1, 2]], BAD_EDGE, 0),
    ([[0, 1], [1, 2], [0, 1]], DUPLICATE, 2),      # a repeated edge
    ([[0, 4], [1, 2], [1, 2], [0, 4]], DUPLICATE, 3),   # the first vertex with a repeated neighbour decides which edge is named
])
def test_rejections(driver, edges, status, bad):
    got = run(driver, 5, edges)
    assert got[0] == status and got[1] == bad and got[2] is None
    with pytest.raises(nr.GraphError):
        nr.graph(5, edges)
