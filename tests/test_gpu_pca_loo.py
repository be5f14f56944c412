"""gingr_pca_leave_one_out (gingr_amd/csrc/pca_leave_one_out.hip) against the definition restated in tests/pca_loo_restatement.py:
loo_direct builds every fold's model by the SVD of its centred shapes and projects the shape left out in longdouble; the device forms one
Gram matrix, corrects it per fold and works every fold's error field out in n-space.  Two correct routes: the tolerance is
1000 x LOO_ROUTE_SPREAD x max |shape - ref| (the repository's rule, pca_restatement.ROUTE_SPREAD), the fold ranks
must be equal exactly.  Sizes are the smallest at which a piece can go wrong (pca_loo_restatement.CASES).  Each check prints
observed / tolerance; test_report_worst_ratios prints the largest.  On an MI355X: avg 0.00055, max 0.0039 (both at (M, n) = (130, 40),
16 ranks), shuffled vertices 0.0021."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pca_loo_restatement as lr
from tests import pca_restatement as pr

pytestmark = pytest.mark.gpu

WORST = {}


def tolerance(ref, X):
    return 1000.0 * lr.LOO_ROUTE_SPREAD * lr.scale_of(ref, X)


def ratio(name, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.all(np.isfinite(got)), name
    worst = float(np.abs(got - want).max() / tol)
    key = name.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"{name}: observed / tolerance = {worst:.3g}")
    assert worst <= 1.0, (name, worst)


@functools.lru_cache(maxsize=None)
def case(M, n, r=None):
    """(ref, shapes) of a data set, computed once"""
    ref, X = pr.dataset(M, n) if r is None else pr.low_rank_dataset(M, n, r)
    X.setflags(write=False)
    return ref, X


@functools.lru_cache(maxsize=None)
def direct(M, n, ranks, r=None):
    """the definition's figures of a data set, computed once and shared"""
    out = lr.loo_direct(case(M, n, r)[1], list(ranks))
    for a in out:
        a.setflags(write=False)
    return out


def device(ctx, X, ranks, rt=1e-10):
    import gingr_amd as ga
    return ga.ModelMetrics.generalizationLeaveOneOut(ctx, X, ranks=ranks, relativeTolerance=rt)


def compare(ctx, name, ref, X, ranks, want):
    res = device(ctx, X, ranks)
    tol = tolerance(ref, X)
    assert res.ranks.tolist() == list(ranks) and res.avg.shape == res.max.shape == (len(ranks), X.shape[0])
    assert np.array_equal(res.foldRanks, want[2]), (name, res.foldRanks, want[2])
    ratio(f"avg: {name}", res.avg, want[0], tol)
    ratio(f"max: {name}", res.max, want[1], tol)
    return res


# ------------------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("M,n,ranks", lr.CASES, ids=[f"M{M}-n{n}" for M, n, _ in lr.CASES])
def test_against_the_definition(ctx, M, n, ranks):
    ref, X = case(M, n)
    res = compare(ctx, f"M={M} n={n} ranks={ranks}", ref, X, ranks, direct(M, n, tuple(ranks)))
    if (M, n) == (1, 8):
        assert res.foldRanks.tolist() == [3] * 8                   # 3 M < n - 2: rank 6 counts as the fold rank 3
        assert np.array_equal(res.avg[3], res.avg[2]) and np.array_equal(res.max[3], res.max[2])
    if (M, n) in ((60, 193), (60, 194)):
        assert res.foldRanks.tolist() == [180] * n                 # fold rank 3 M


@pytest.mark.parametrize("M,n,r,ranks", lr.LOW_RANK)
def test_null_space_of_many_dimensions(ctx, M, n, r, ranks):
    ref, X = case(M, n, r)
    res = compare(ctx, f"low rank M={M} n={n} r={r}", ref, X, ranks, direct(M, n, tuple(ranks), r))
    assert res.foldRanks.tolist() == [r] * n
    assert np.array_equal(res.avg[2], res.avg[1])                  # rank 10 is clipped to 4: the same columns


def test_ranks_none_is_the_full_fold_rank(ctx):
    ref, X = case(37, 5)
    res = device(ctx, X, None)
    assert res.ranks.tolist() == [3]
    ratio("avg: ranks=None", res.avg, direct(37, 5, (1, 2, 3))[0][2:3], tolerance(ref, X))
    assert np.array_equal(res.curve(), res.avg.mean(axis=1))


def test_zero_tolerance_keeps_at_most_n_minus_2_components(ctx):
    """relativeTolerance = 0 keeps every positive eigenvalue: the null direction of a centred fold may come back as a positive
    rounding residue, and the cap n - 2 is what keeps it out"""
    ref, X = case(37, 5)
    res = device(ctx, X, [1, 2, 3], rt=0.0)
    want = lr.loo_direct(X, [1, 2, 3], relative_tolerance=0.0)
    assert res.foldRanks.tolist() == want[2].tolist() == [3] * 5
    ratio("avg: relativeTolerance = 0", res.avg, want[0], tolerance(ref, X))


# ---------------------------------------------------------------------------------------------------------------- special folds
def test_fold_of_rank_zero(ctx):
    """n - 1 identical shapes and one different: the fold without the different one has rank 0, its projection is the fold's mean --
    the identical shape -- so the distance is |x_i - y| per vertex; the other folds have rank 1"""
    ref, X = case(130, 8)
    Y = np.repeat(X[:1], 8, axis=0)
    Y[5] = X[5]
    res = device(ctx, Y, [1, 3, 6])
    want = lr.loo_direct(Y, [1, 3, 6])
    assert want[2].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]
    assert np.array_equal(res.foldRanks, want[2])
    tol = tolerance(ref, Y)
    ratio("avg: one fold of rank 0", res.avg, want[0], tol)
    ratio("max: one fold of rank 0", res.max, want[1], tol)
    dist = np.sqrt(((X[5] - X[0]) ** 2).sum(axis=1))
    for q in range(3):
        assert abs(res.avg[q, 5] - dist.mean()) <= tol and abs(res.max[q, 5] - dist.max()) <= tol


def test_two_duplicate_shapes(ctx):
    ref, X = case(130, 12)
    Y = X.copy()
    Y[7] = Y[2]
    want = lr.loo_direct(Y, [1, 5, 10])
    res = device(ctx, Y, [1, 5, 10])
    assert np.array_equal(res.foldRanks, want[2])
    tol = tolerance(ref, Y)
    ratio("avg: duplicate shapes", res.avg, want[0], tol)
    ratio("max: duplicate shapes", res.max, want[1], tol)
    assert abs(res.avg[0, 7] - res.avg[0, 2]) <= tol               # the twins see the same fold


def test_reach_of_every_vertex(ctx):
    """one vertex of one shape far away: no model of the others reaches it, that shape's max is the distance of that vertex"""
    ref, X = case(130, 12)
    plain = device(ctx, X, [3]).max[0, 4]
    for v in (0, 15, 16, 127, 128, 129):
        Y = X.copy()
        Y[4, v] += np.array([300.0, -400.0, 1200.0])
        res = device(ctx, Y, [3])
        want = lr.loo_direct(Y, [3])
        ratio(f"max-reach: vertex {v}", res.max[0, 4:5], want[1][0, 4:5], tolerance(ref, Y))
        assert res.max[0, 4] > 1000.0 and plain < 250.0


def test_shuffled_vertices_give_the_same_values(ctx):
    ref, X = case(257, 17)
    perm = np.random.default_rng(3).permutation(257)
    a, b = device(ctx, X, [1, 4, 15]), device(ctx, np.ascontiguousarray(X[:, perm]), [1, 4, 15])
    tol = tolerance(ref, X)
    assert np.array_equal(a.foldRanks, b.foldRanks)
    ratio("avg-shuffled: vertices in another order", b.avg, a.avg, tol)
    ratio("max-shuffled: vertices in another order", b.max, a.max, tol)


def test_two_calls_give_the_same_bits(ctx):
    for M, n, ranks in [(130, 40, [1, 7, 38]), (60, 194, [1, 12])]:
        _, X = case(M, n)
        a, b = device(ctx, X, ranks), device(ctx, X, ranks)
        assert np.array_equal(a.avg, b.avg) and np.array_equal(a.max, b.max) and np.array_equal(a.foldRanks, b.foldRanks)


def test_three_problem_eigen_path_keeps_its_bits(ctx):
    """createUsingPCA at n = 40 (the three-problem entry of the register kernel) gives the same variances before and after a
    leave-one-out call (the strided entry of the same kernel)"""
    import gingr_amd as ga
    ref, X = case(130, 40)

    def variances():
        m = ga.PointDistributionModel.createUsingPCA(ctx, ref, X)
        try:
            return np.array(m.to_host().variance)
        finally:
            m.device().close()
    before = variances()
    device(ctx, X, [1, 38])
    after = variances()
    assert before.shape == (39,) and np.array_equal(before, after)


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_usable(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd._native import dptr, iptr
    ref, X = case(37, 5)
    X = np.array(X)

    def fails(code, word, shapes, ranks, rt=1e-10):
        with pytest.raises(ga.GingrNativeError) as e:
            device(ctx, shapes, ranks, rt)
        assert e.value.code == code and "pca_leave_one_out" in str(e.value) and word in str(e.value), str(e.value)

    fails(nat.ERR_BAD_ARGUMENT, "shapes", X[:2], [1])
    fails(nat.ERR_BAD_ARGUMENT, "shapes", np.zeros((513, 2, 3)), [1])
    fails(nat.ERR_BAD_ARGUMENT, "M =", np.zeros((5, 0, 3)), [1])
    fails(nat.ERR_BAD_ARGUMENT, "ranks", X, [])
    fails(nat.ERR_BAD_ARGUMENT, "ranks", X, list(range(1, 18)))
    fails(nat.ERR_BAD_ARGUMENT, "ranks[0]", X, [0])
    fails(nat.ERR_BAD_ARGUMENT, "ranks[1]", X, [1, 4])
    fails(nat.ERR_BAD_ARGUMENT, "increasing", X, [2, 2])
    fails(nat.ERR_BAD_ARGUMENT, "relative_tolerance", X, [1], rt=1.0)
    fails(nat.ERR_BAD_ARGUMENT, "relative_tolerance", X, [1], rt=-1e-3)
    fails(nat.ERR_BAD_ARGUMENT, "relative_tolerance", X, [1], rt=float("nan"))
    fails(nat.ERR_BAD_ARGUMENT, "identical", np.repeat(X[:1], 5, axis=0), [1])
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[3, 11, 2] = bad
        fails(nat.ERR_NONFINITE, "shape 3", Y, [1])
    # null pointers, one at a time; nothing is written
    k = np.array([1], dtype=np.int32)
    avg, mx, fr = np.full((1, 5), -7.0), np.full((1, 5), -7.0), np.full(5, -7, dtype=np.int32)
    args = [dptr(X), 1e-10, 1, iptr(k), dptr(avg), dptr(mx), iptr(fr)]
    for at in (0, 3, 4, 5, 6):
        a = list(args)
        a[at] = None
        code = ctx._lib.gingr_pca_leave_one_out(ctx.handle, 37, 5, *a)
        text = ctx._lib.gingr_last_error(ctx.handle).decode()
        assert code == nat.ERR_BAD_ARGUMENT and "pca_leave_one_out" in text and "null" in text, (at, code, text)
    assert ctx._lib.gingr_pca_leave_one_out(ctypes.c_void_p(), 37, 5, *args) == nat.ERR_BAD_ARGUMENT
    assert np.all(avg == -7.0) and np.all(mx == -7.0) and np.all(fr == -7)
    # the context still works
    res = device(ctx, X, [1, 2, 3])
    ratio("avg: after the errors", res.avg, direct(37, 5, (1, 2, 3))[0], tolerance(ref, X))


def test_report_worst_ratios():
    """(last in the file) the largest observed / tolerance per quantity of this run, for the record"""
    for name in sorted(WORST):
        print(f"worst observed / tolerance, {name}: {WORST[name]:.3g}")
