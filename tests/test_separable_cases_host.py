"""Host side of the separable-model edge tests (separable_cases.py): the restatements against hand-worked values, the row order of
the test clouds under the library's own k-d header, the references against plain numpy, the bounds against damage they must
catch, and the float64 figures of the block sizes the three-block solve is tested at.  No GPU."""
import shutil

import numpy as np
import pytest

from tests import posterior_solve_cases as pc
from tests import separable_cases as sc

pytestmark = pytest.mark.skipif(not sc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")


# ------------------------------------------------------------------------------------------------ slab plan
def test_slab_plan_by_hand():
    for M in (1, 15, 16, 17, 48, 64):
        assert sc.slabs(M) == [(0, M)], M
    assert sc.slabs(65) == [(0, 48), (48, 65)]
    assert sc.slabs(193) == [(0, 64), (64, 128), (128, 192), (192, 193)]
    assert sc.compact_plan(257) == (5, 64)          # want 5, ceil(257 / 5) = 52 -> 64-row slabs, the fifth holds one row
    n, rps = sc.compact_plan(10881)
    assert rps == 80 and n == 137 and sc.slabs(10881)[-1] == (10880, 10881)
    for M in sc.ROWS + [1000, 50000, 200000]:       # the slabs tile the rows, 16-row steps, at most 170 of them
        sl = sc.slabs(M)
        assert sl[0][0] == 0 and sl[-1][1] == M and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert sc.compact_plan(M)[1] % 16 == 0 and len(sl) <= 170 and all(b > a for a, b in sl)


def test_rows_cover_the_plan_edges():
    assert set(sc.ROWS) >= {1, 15, 16, 17, 48, 64, 65, 193, 257, 10881}
    single_last = [M for M in sc.ROWS if len(sc.slabs(M)) > 1 and sc.slabs(M)[-1][1] - sc.slabs(M)[-1][0] == 1]
    assert single_last == [193, 257, 10881]


# ------------------------------------------------------------------------------------------------ SepMap and the class rule
def test_sep_map_by_hand():
    sm = sc.SepMap(16)
    assert (sm.cls(5), sm.pos(5), sm.col(0, 0), sm.col(1, 0), sm.col(2, 47), sm.total()) == (5, 21, 32, 80, 175, 176)
    m = sc.sep_map(np.array([2, 0, 0, 1, 2]))       # five columns, rp = 16
    assert list(m[:5]) == [2, 0, 0, 1, 2] and np.all(m[5:16] == -1)
    assert list(m[16:21]) == [0, 0, 1, 0, 1] and np.all(m[21:32] == -1)
    assert list(m[32:34]) == [1, 2] and m[34] == -1 and list(m[80:82]) == [3, -1] and list(m[128:131]) == [0, 4, -1]
    assert m.shape == (176,) and m.dtype == np.int32
    for counts in sc.COUNTS:                          # col is the inverse of (cls, pos)
        for order in sc.ORDERS:
            classes = sc.basis(64, counts, order)[2]
            m, s = sc.sep_map(classes), sc.SepMap(sc.rp_of(len(classes)))
            for k, d in enumerate(classes):
                assert m[s.cls(k)] == d and m[s.col(d, m[s.pos(k)])] == k
            assert [int(np.count_nonzero(m[s.col(d, 0): s.col(d, 0) + 48] >= 0)) for d in range(3)] == list(counts)


def test_class_rule_by_hand():
    U = np.zeros((6, 4))
    U[0, 0], U[3, 0] = 1.0, -2.0      # rows 3 i + 0
    U[4, 1] = 1e-300                  # row 3 + 1
    U[2, 2], U[0, 2] = 5.0, -0.0      # rows 3 i + 2; a negative zero on coordinate 0 holds nothing
    assert list(sc.column_classes(U)) == [0, 1, 2, 0]   # the all-zero column: class 0
    U[1, 0] = 1e-300
    assert sc.column_classes(U) is None


def test_bases():
    assert len(sc.COUNTS) == 12 and [c for c in sc.COUNTS if sc.rp_of(sum(c)) == 112 and sum(c) == 112] == sc.COUNTS[-3:]
    for counts in sc.COUNTS:
        for order in sc.ORDERS:
            for M in (17, 64, 257):
                U, lam, classes = sc.basis(M, counts, order)
                r = sum(counts)
                assert U.shape == (3 * M, r) and list(sc.column_classes(U)) == list(classes)
                assert tuple(int(np.count_nonzero(classes == d)) for d in range(3)) == counts
                assert np.all(np.diff(lam) <= 0) and lam.min() >= 4.5 ** 2 and lam.max() <= 20.0 ** 2
                assert np.array_equal(np.sqrt(lam) * np.sqrt(lam), lam)                    # exact square roots
                if sc.admits(M, counts):
                    assert np.abs(U.T @ U - np.eye(r)).max() < 1e-13
                if order == "grouped_201" and r > 1:
                    assert list(classes) == sorted(classes, key=lambda d: (2, 0, 1).index(d))
                if order == "interleaved" and counts == (17, 15, 16):
                    assert list(classes[:6]) == [0, 1, 2, 0, 1, 2] and list(classes[-2:]) == [2, 0]
    a, b = sc.basis(64, (17, 15, 16), "random")[2], sc.basis(64, (17, 15, 16), "interleaved")[2]
    assert not np.array_equal(a, b) and np.array_equal(a, sc.basis(64, (17, 15, 16), "random")[2])   # seeded


# ------------------------------------------------------------------------------------------------ row order
def test_line_clouds_keep_the_callers_order_restated():
    for M in sc.ROWS:
        ref, mean = sc.line_reference(M)
        assert np.array_equal(sc.kd_leaf_order(ref + mean), np.arange(M)), M
    pts = np.random.default_rng(2).normal(0, [30.0, 20.0, 10.0], (1000, 3))   # (the restatement does reorder other clouds)
    assert not np.array_equal(sc.kd_leaf_order(pts), np.arange(1000))


def test_line_clouds_keep_the_callers_order_under_the_library_header(tmp_path):
    """kd_order.h itself, through the stand-alone driver of test_kd_order_host.py: the identity on every test cloud, and the
    restatement's order on a cloud that is reordered."""
    from tests import test_kd_order_host as kd
    if kd.CXX is None or shutil.which(kd.CXX) is None:
        pytest.skip("no host C++ compiler")
    exe = kd.compile_driver(tmp_path / "kd_order_driver", "address,undefined")
    for M in sc.ROWS:
        ref, mean = sc.line_reference(M)
        assert np.array_equal(kd.order(exe, ref + mean), np.arange(M)), M
    pts = kd.cloud(1000, 5)
    assert np.array_equal(kd.order(exe, pts), sc.kd_leaf_order(pts))


# ------------------------------------------------------------------------------------------------ pairs of the Gram cases
def test_marker_pairs():
    for M in sc.ROWS:
        pid, var, empty = sc.marker_pairs(M)
        sl = sc.slabs(M)
        assert (empty is None) == (len(sl) == 1) and (empty is None or empty != len(sl) - 1)
        assert var.min() == 1e-6 and var.max() <= 1e6 and len(set(pid)) == len(pid)
        for b, (r0, r1) in enumerate(sl):
            inside = pid[(pid >= r0) & (pid < r1)]
            if b == empty:
                assert inside.size == 0
            else:
                assert r0 in inside and r1 - 1 in inside
                assert var[pid == r0][0] == 1e-6 and var[pid == r1 - 1][0] == 1e-6
        if M >= 48:
            assert 0 < M - len(pid) and len(pid) < M   # vertices without a pair


# ------------------------------------------------------------------------------------------------ references and bounds
def _gram_case(M=65, counts=(17, 15, 16), order="random"):
    ref, mean = sc.line_reference(M)
    U, lam, classes = sc.basis(M, counts, order)
    Q = sc.scaled_basis(U, lam)
    pid, var, _ = sc.marker_pairs(M)
    rng = np.random.default_rng(3)
    w, obs = np.zeros(M), np.zeros((M, 3))
    w[pid] = 1.0 / var
    obs[pid] = (ref + mean)[pid] + rng.normal(0, 1.0, (len(pid), 3))
    return ref, mean, Q, classes, w, obs


def test_gram_reference_against_numpy_and_bound_against_a_dropped_row():
    ref, mean, Q, classes, w, obs = _gram_case()
    e = sc.observation_e(w, obs, ref, mean)
    G, rhs, bG, brhs = sc.gram_bounds(Q, classes, w, e, obs, ref, mean, len(sc.slabs(65)))
    G64 = Q.T @ (np.repeat(w, 3)[:, None] * Q)
    rhs64 = Q.T @ (np.repeat(w, 3) * (obs - ref - mean).reshape(-1))
    same = classes[:, None] == classes[None, :]
    assert np.all(np.abs(G64 - G)[same] <= bG[same]) and np.all(np.abs(rhs64 - rhs) <= brhs)   # the float64 product is inside
    assert np.all(np.asarray(G, dtype=np.float64)[~same] == 0.0)
    # dropping the last row of the last slab (a marker) is far outside, in G and in rhs
    w2 = w.copy()
    w2[-1] = 0.0
    G2 = Q.T @ (np.repeat(w2, 3)[:, None] * Q)
    rhs2 = Q.T @ (np.repeat(w2, 3) * (obs - ref - mean).reshape(-1))
    assert np.max(np.abs(G2 - G)[same] / bG[same]) > 1e6 and np.max(np.abs(rhs2 - rhs) / brhs) > 1e6
    # so is any other single row with a weight, and a swap of two positions of one class in the scatter
    for i in np.flatnonzero(w)[:5]:
        w3 = w.copy()
        w3[i] = 0.0
        G3 = Q.T @ (np.repeat(w3, 3)[:, None] * Q)
        assert np.max(np.abs(G3 - G)[same] / bG[same]) > 1.0, i
    assert np.max(np.abs(G64.T[::-1, ::-1] - G)[same] / bG[same]) > 1e6
    assert bG.max() < 1e-9 * np.abs(np.asarray(G, dtype=np.float64)).max()


def test_cpd_weight_and_observation_restated():
    rng = np.random.default_rng(4)
    P1, PX = rng.uniform(0.2, 3.0, 50), rng.normal(0, 30, (50, 3))
    w = sc.cpd_weight(P1, 0.37, 2.0)
    assert np.max(np.abs(w - P1 / (0.37 * 2.0)) / w) <= 4 * sc.U53 * 2
    assert np.allclose(sc.cpd_observation(None, P1, PX), PX / P1[:, None], rtol=1e-15, atol=0)


def test_fit_reference_and_bound():
    ref, mean, Q, classes, _, _ = _gram_case(257, (48, 1, 0), "interleaved")
    alpha = np.random.default_rng(5).normal(0, 1, Q.shape[1])
    fit, bound = sc.fit_reference(ref, mean, Q, alpha, classes)
    f64 = ref + mean + (Q @ alpha).reshape(-1, 3)
    assert np.all(np.abs(f64 - fit) <= bound)
    assert np.array_equal(np.asarray(fit, dtype=np.float64)[:, 2], (ref + mean)[:, 2])     # the empty class: ref + mean, one rounding
    assert bound[:, 0].max() < 52 * sc.U53 * 1e5 and np.all(bound[:, 2] == 3 * sc.U53 * (np.abs(ref) + np.abs(mean))[:, 2])
    wrong = alpha.copy()
    wrong[[0, 2]] = wrong[[2, 0]]                                                           # two positions of class 0 exchanged
    assert np.max(np.abs(ref + mean + (Q @ wrong).reshape(-1, 3) - fit) / bound) > 1e6


# ------------------------------------------------------------------------------------------------ block systems
def test_block_solve_ignores_entries_between_the_classes():
    classes = sc.basis(64, (17, 15, 16), "random")[2]
    blocks = [pc.make_case(f, n)[:2] for f, n in (("well", 17), ("graded_up", 15), ("ill", 16))]
    G, rhs = sc.scatter_blocks(classes, blocks)
    a = sc.block_solve(G, rhs, classes)
    for cols, (f, n) in zip(sc.class_columns(classes), (("well", 17), ("graded_up", 15), ("ill", 16))):
        assert np.array_equal(a[cols], pc.reference(f, n)["a"])
    i, j = int(np.flatnonzero(classes == 0)[3]), int(np.flatnonzero(classes == 2)[5])
    G2 = G.copy()
    G2[i, j] = G2[j, i] = 0.5
    assert np.array_equal(sc.block_solve(G2, rhs, classes), a)
    dense = np.linalg.solve(np.eye(48) + G2, rhs)
    assert np.linalg.norm(dense - np.asarray(a, dtype=np.float64)) > 1e-6 * np.linalg.norm(dense)


def test_block_cases_cover_what_they_claim():
    at = {48: set(), 17: set()}
    sizes = set()
    for case in sc.BLOCK_CASES:
        fams = [c[0] for c in case if c is not None]
        assert len(set(fams)) == len(fams)                       # a different family in each class
        assert sum(sc.block_counts(case)) <= 112
        for c in case:
            sizes.add(0 if c is None else c[1])
            if c is not None and c[1] in at:
                at[c[1]].add(c[0])
    assert at[48] == set(pc.FAMILIES) and at[17] == set(pc.FAMILIES) and sizes == set(sc.BLOCK_SIZES)
    assert [tuple(c[0] for c in case) for case in sc.BLOCK_CASES[:2]] == [("ill", "zero", "graded_up"), ("diagonal", "graded_down", "well")]
    assert max(sum(sc.block_counts(c)) for c in sc.BLOCK_CASES) == 112


def test_float64_figures_hold_at_the_block_sizes():
    """The table the GPU bounds hang on (posterior_solve_cases.F64_FIGURES: maximum over RANKS) was not measured at 47 and 48.  Printed
    and asserted here: at the block sizes the plain float64 route stays within the committed figures, so gpu_bound serves per block
    as it stands (a figure here above the table's would be the one reason to raise the table)."""
    got = pc.measure_float64_figures(ranks=[n for n in sc.BLOCK_SIZES if n])
    print()
    for fam in pc.FAMILIES:
        print(f'    "{fam}": {{' + ", ".join(f'"{k}": {got[fam][k]:.2e}' for k in ("forward", "backward")) + "},")
    for fam in pc.FAMILIES:
        for k in ("forward", "backward"):
            # (the table keeps three digits: half a unit of the last one)
            assert got[fam][k] <= 1.005 * pc.F64_FIGURES[fam][k], (fam, k, got[fam][k], pc.F64_FIGURES[fam][k])
