"""The cases and the tolerance of the direct eigen-solver tests (tests/sym_eig_cases.py), on the host: both host routes over every case,
every figure printed, EIG_ROUTE_SPREAD asserted to cover them; the case lists pinned to the sizes at which the device's kernels change
path, so that nobody shrinks them silently.  No GPU."""
import numpy as np

from tests import sym_eig_cases as sc


def test_route_spread():
    """numpy.linalg.eigh and the cyclic two-sided Jacobi of sym_eig_cases.py, judged in np.longdouble against LAPACK's spectrum of the
    rounded matrix.  The largest figure over all cases but `null_many` is the constant EIG_ROUTE_SPREAD."""
    worst, where = 0.0, None
    for kind, n, variant in sc.all_cases():
        G, ref = sc.matrix(kind, n, variant), sc.reference_spectrum(kind, n, variant)
        e1, V1 = sc.lapack_eigh(G)
        e2, V2, sweeps = sc.jacobi_eigh(G)
        f1, f2 = sc.judge(G, e1, V1, ref), sc.judge(G, e2, V2, ref)
        print(f"{kind:13s} n={n:3d} v={variant}  eigh: resid {f1[0]:.2e} orth {f1[1]:.2e} evals {f1[2]:.2e}   "
              f"jacobi ({sweeps:2d} sweeps): resid {f2[0]:.2e} orth {f2[1]:.2e} evals {f2[2]:.2e}")
        assert f1[3] and f2[3], (kind, n, variant)
        assert sweeps < 60, (kind, n, variant)
        if kind == "null_many":
            continue
        big = max(f1[:3] + f2[:3])
        if big > worst:
            worst, where = big, (kind, n, variant)
    print(f"largest: {worst:.2e} at {where}; EIG_ROUTE_SPREAD = {sc.EIG_ROUTE_SPREAD:.2e}")
    assert worst <= sc.EIG_ROUTE_SPREAD
    assert sc.EIG_ROUTE_SPREAD <= 2.0 * worst                      # the constant is the measurement, not a generous round number


def test_case_lists_hold_the_class_edges():
    """the sizes at which sym_eig changes kernel, template, block count or row padding (eig.hip, sym_eig.hip)"""
    assert set(sc.KINDS) == {"graded", "shifted", "clustered"}
    assert set(sc.REGISTER_SIZES) >= {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192}
    assert set(sc.SPECIAL_SIZES) >= {5, 64, 129} and set(sc.SPECIAL_KINDS) >= {"identity", "diagonal", "diagonal_perm"}
    assert set(sc.STRIDED_SIZES) >= {5, 64, 65, 129, 192} and sc.STRIDED_COUNT >= 4
    assert (5, 70, 190) in sc.MIXED_BATCHES and (64, 65, 129) in sc.MIXED_BATCHES
    assert set(sc.BLOCK_SIZES) >= {193, 224, 225, 256, 257, 321, 449, 512}
    assert (193, 192, 193) in sc.BLOCK_BATCHES and (257, 256, 257) in sc.BLOCK_BATCHES
    assert set(sc.FALLBACK_ONE_WORKGROUP) >= {2, 31, 64, 128} and max(sc.FALLBACK_ONE_WORKGROUP) <= 128
    assert set(sc.FALLBACK_GRID) >= {129, 192} and min(sc.FALLBACK_GRID) > 128
    assert set(sc.TWO_SIDED_DIRECT) >= {193, 257} and max(sc.TWO_SIDED_DIRECT) <= 257
    assert sc.ZERO_ROW_BLOCKS == 200 and sc.DEFECT_SIZE == 200 and sc.DEFECT_KINDS == ("graded", "zero_row", "shifted")
    assert set(sc.NULL_MANY_SIZES) >= {20, 130}
    cases = sc.all_cases()
    assert len(cases) == len(set(cases))
    for kind in sc.KINDS:
        for n in sc.REGISTER_SIZES + sc.BLOCK_SIZES:
            assert (kind, n, 0) in cases


def test_matrices_are_what_they_claim():
    for kind, n, variant in sc.all_cases():
        G = sc.matrix(kind, n, variant)
        assert G.shape == (n, n) and G.dtype == np.float64 and np.array_equal(G, G.T) and np.isfinite(G).all()
    # a problem that comes twice in a batch is two different matrices
    assert not np.array_equal(sc.matrix("graded", 193, 0), sc.matrix("graded", 193, 1))
    # clusters: 1, 2, 3 and 7 equal values
    lam = sc.clustered_spectrum(20)
    assert [int((lam == v).sum()) for v in sorted(set(lam), reverse=True)][:4] == [1, 2, 3, 7]
    # the conditioning each kind promises, by LAPACK on the rounded matrix
    for n in (64, 200):
        e = sc.reference_spectrum("shifted", n)
        assert e[-1] > 0 and e[0] / e[-1] <= n + 1 + 1e-9
        e = sc.reference_spectrum("graded", n)
        assert abs(e[0] - 1.0) < 1e-12 and abs(e[-1] - 1e-10) < 1e-14
    for n in sc.FALLBACK_ONE_WORKGROUP + sc.FALLBACK_GRID:
        assert abs(sc.reference_spectrum("null1", n)[-1]) < 1e-15
        Z = sc.matrix("zero_row", n)
        assert not Z[n // 2].any() and not Z[:, n // 2].any() and Z[0, 0] > 0
    for n in sc.NULL_MANY_SIZES:
        e = sc.reference_spectrum("null_many", n)
        assert e[n // 2 - 1] > 1e-11 and np.abs(e[n // 2:]).max() < 1e-15
    for kind in ("diagonal", "diagonal_perm"):
        D = sc.matrix(kind, 64)
        assert np.count_nonzero(D - np.diag(np.diag(D))) == 0 and np.unique(np.diag(D)).shape[0] == 63
    assert np.all(np.diff(np.diag(sc.matrix("diagonal", 64))) <= 0) and not np.all(np.diff(np.diag(sc.matrix("diagonal_perm", 64))) <= 0)


def test_judge_sees_a_wrong_decomposition():
    """what the figures do with the failures they are there for: an un-rotated factor, a swapped pair of eigenvalues, a NaN"""
    G, ref = sc.matrix("graded", 65), sc.reference_spectrum("graded", 65)
    e, V = sc.lapack_eigh(G)
    good = sc.judge(G, e, V, ref)
    assert max(good[:3]) < 1e-13 and good[3]
    L = np.linalg.cholesky(G + 1e-9 * np.eye(65))                  # columns of a Cholesky factor passed off as eigenvectors
    bad = sc.judge(G, (L * L).sum(0), L / np.sqrt((L * L).sum(0))[None, :], ref)
    assert bad[0] > 1e-3 and bad[1] > 1e-3
    e2 = e.copy()
    e2[[3, 4]] = e2[[4, 3]]
    swapped = sc.judge(G, e2, V, ref)
    assert not swapped[3] and swapped[0] > 1e-3
    V2 = V.copy()
    V2[5, 7] = np.nan
    assert sc.judge(G, e, V2, ref)[0] == float("inf") and sc.judge(G, e, V2, ref)[1] == float("inf")
