"""gingr_model_instances / gingr_model_generalization / gingr_model_specificity (gingr_amd/csrc/model_metrics.hip) element by element
against the longdouble restatement (tests/model_metrics_restatement.py) and against the existing single-call route --
truncate(k), coefficients, instance, numpy distances -- under bounds derived in the restatement from the summation lengths, the unit
roundoff and cond(S / eps + I), never from what the code gives.  Each check prints observed / bound.

Sizes are the smallest at which the kernels take another path: a wave's 16 vertices, a workgroup's 128, a 64-column chunk, more than
512 columns, one and several slabs.  Non-finite input: GINGR_ERR_NONFINITE, nothing computed (documented in include/gingr_hip.h).
Observed / bound on an MI355X, the largest per quantity (test_report_worst_ratios prints them): coefficients
0.0042, avg 0.0032, max 0.0059, instances 0.31, min_avg 0.076; against the single-call route 0.0028, 0.0028, 0.011 and 0.15."""

import numpy as np
import pytest

from tests import model_metrics_restatement as mm

pytestmark = pytest.mark.gpu

WORST = {}


def ratio(name, got, want, bound, factor=1.0):
    """largest |got - want| / (factor * bound), printed and kept; the assertion of every element-wise check"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.all(np.isfinite(np.asarray(got, dtype=float))), name
    worst = float((np.abs(got - want) / (factor * np.asarray(bound, dtype=np.longdouble))).max())
    WORST[name.split(":")[0]] = max(WORST.get(name.split(":")[0], 0.0), worst)
    print(f"{name}: observed / bound = {worst:.3g}")
    assert worst <= 1.0, (name, worst)
    return worst


def host_model(mo):
    import gingr_amd as ga
    return ga.PointDistributionModel(mo.ref, mo.mean, mo.basis, mo.variance)


def restated(dm):
    """the restatement's model of a resident model (basis = Q0 / sd comes back through the download)"""
    h = dm.download()
    return mm.Model(np.asarray(h.reference), np.asarray(h.mean), np.asarray(h.basis), np.asarray(h.variance))


def shapes_around(mo, n, seed, spread=2.0):
    rng = np.random.default_rng(seed)
    return mo.ref[None] + mo.mean[None] + rng.normal(0.0, spread, (n, mo.M, 3))


# ------------------------------------------------------------------------------------------------------------------ instances
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("r", [1, 16, 17, 48, 100])
def test_instances_every_coordinate(ctx, M, r):
    import gingr_amd as ga
    mo = mm.random_model(M, r, 100 * M + r)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        for n in (1, 16, 65):   # 65 crosses a 64-column chunk
            A = np.random.default_rng(n).normal(0.0, 1.0, (n, r))
            got = dm.instances(A)
            bound = mm.instance_bound(mo, A)
            ratio(f"instances: M={M} r={r} n={n} against the restatement", got, mm.instances(mo, A), bound)
            single = np.stack([dm.instance(a) for a in A])
            ratio(f"instances-single: M={M} r={r} n={n} against instance() one by one", got, single, bound, factor=2.0)
    finally:
        dm.close()


def test_instances_past_one_block_and_row_reach(ctx):
    """513 coefficient vectors: two blocks; and a last basis column that is non-zero at the caller's last row only moves that one
    coordinate, by exactly sqrt(variance) * alpha (one product, added to ref + mean)"""
    import gingr_amd as ga
    mo = mm.random_model(17, 17, 5)
    mo.basis[:, -1] = 0.0
    mo.basis[-1, -1] = 1.0
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        A = np.random.default_rng(3).normal(0.0, 1.0, (513, 17))
        got = dm.instances(A)
        ratio("instances: 513 vectors", got, mm.instances(mo, A), mm.instance_bound(mo, A))
        A0 = A[:5].copy()
        A0[:, -1] = 0.0
        base, moved = dm.instances(A0), dm.instances(np.concatenate([A0[:, :-1], A[:5, -1:]], axis=1))
        diff = moved - base
        assert np.all(diff.reshape(5, -1)[:, :-1] == 0.0), "the last column reaches other rows"
        assert np.all(diff[:, -1, 2] != 0.0)
        ratio("instances: last column, last row", diff[:, -1, 2], np.sqrt(mo.variance[-1]) * A[:5, -1], 4 * mm.U * (np.abs(moved[:, -1, 2]) + np.abs(base[:, -1, 2]) + np.abs(diff[:, -1, 2])))
    finally:
        dm.close()


# ------------------------------------------------------------------------------------------------------------- generalization
def single_route(dm, X, ranks):
    """truncate(k), coefficients, instance, numpy distances: the existing API, shape by shape"""
    n, r = X.shape[0], dm.rank
    coef, avg, mx = np.zeros((len(ranks), n, r)), np.zeros((len(ranks), n)), np.zeros((len(ranks), n))
    for q, k in enumerate(ranks):
        tm = dm.truncate(int(k)) if k < r else dm
        try:
            for i in range(n):
                a = tm.coefficients(X[i])
                dist = np.linalg.norm(tm.instance(a) - X[i], axis=1)
                coef[q, i, :k], avg[q, i], mx[q, i] = a, dist.sum() / X.shape[1], dist.max()
        finally:
            if tm is not dm:
                tm.close()
    return coef, avg, mx


def check_generalization(ctx, dm, mo, X, ranks, label, single=True, cond_limit=1e5):
    coef, avg, mx = dm.project(X, ranks)
    b = mm.projection_bounds(mo, X, ranks)
    print(f"{label}: cond_inf(S_k / eps + I) = {b['cond'].max():.1f}")
    assert b["cond"].max() < cond_limit
    wc, wa, wx = mm.project_direct(mo, X, ranks)
    for q, k in enumerate(ranks):
        assert not np.any(coef[q, :, k:]), "coefficients from entry k on must be zero"
    ratio(f"coefficients: {label}", coef, wc, np.broadcast_to(b["coef"][:, :, None], coef.shape))
    ratio(f"avg: {label}", avg, wa, b["avg"])
    ratio(f"max: {label}", mx, wx, b["max"])
    if single:
        # the sum of both routes' bounds: the single-call route solves the same system from the same sums (its own rounding, the same
        # bound) and then rounds ref + mean + Q alpha and the subtraction of the shape coordinate by coordinate (instance_bound)
        sc, sa, sx = single_route(dm, X, ranks)
        inst = np.stack([mm.instance_bound(mo, np.asarray(wc[q], dtype=float)).sum(axis=2).max(axis=1) for q in range(len(ranks))])
        ratio(f"coefficients-single: {label}", coef, sc, np.broadcast_to(b["coef"][:, :, None], coef.shape), factor=2.0)
        ratio(f"avg-single: {label}", avg, sa, 2.0 * b["avg"] + inst)
        ratio(f"max-single: {label}", mx, sx, 2.0 * b["max"] + inst)
    return coef, avg, mx


def test_generalization_uploaded_non_orthogonal_model(ctx):
    """random columns, not orthonormalised: Binv is full and the nested solve is really exercised.  Ranks 1, 5, 16, 17 and r = 48;
    5 shapes in 16 padded columns x 5 ranks = 80 columns: two 64-column chunks.  Shape 1 is exactly an instance of the model -- its
    distance is the ridge's bias, orders of magnitude below the others: a relative bound could not be met, the absolute one is;
    shape 2 lies far outside the span."""
    import gingr_amd as ga
    mo = mm.random_model(130, 48, 12)
    X = shapes_around(mo, 5, 1)
    X[1] = np.asarray(mm.instances(mo, np.random.default_rng(2).normal(0, 1, (1, 48))), dtype=np.float64)[0]
    X[2] = shapes_around(mo, 1, 3, spread=200.0)[0]
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        _, avg, _ = check_generalization(ctx, dm, mo, X, [1, 5, 16, 17, 48], "uploaded M=130 r=48")
        assert 0.0 < avg[-1, 1] < 1e-3 * avg[-1, 0] and avg[-1, 2] > 50.0 * avg[-1, 0]
        # ModelMetrics on the host model (uploaded for the call), ranks=None: the full rank only
        res = ga.ModelMetrics.generalization(ctx, host_model(mo), X)
        assert res.ranks.tolist() == [48] and np.array_equal(res.avg[0], avg[-1]) and res.curve().shape == (1,)
    finally:
        dm.close()


def test_generalization_past_512_columns(ctx):
    """n = 40 (48 padded columns) x 16 ranks = 768 columns"""
    import gingr_amd as ga
    mo = mm.random_model(40, 20, 14)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        check_generalization(ctx, dm, mo, shapes_around(mo, 40, 4), list(range(1, 16)) + [20], "uploaded M=40 r=20, 40 shapes x 16 ranks")
    finally:
        dm.close()


def test_generalization_pca_model_and_gpmm(ctx):
    """a PCA-built model (12 fits of a random model, held-out shapes measured) and a small Gaussian GPMM, through ModelMetrics"""
    import gingr_amd as ga
    src = mm.random_model(257, 35, 13)
    fits = np.asarray(mm.instances(src, np.random.default_rng(5).normal(0, 1, (12, 35))), dtype=np.float64)
    pca = ga.PointDistributionModel.createUsingPCA(ctx, src.ref + src.mean, fits)
    dm = pca.device()
    mo = restated(dm)
    held_out = np.asarray(mm.instances(src, np.random.default_rng(6).normal(0, 1, (4, 35))), dtype=np.float64)
    check_generalization(ctx, dm, mo, held_out, [1, 3, mo.rank], f"PCA M=257 rank={mo.rank}")
    res = ga.ModelMetrics.generalization(ctx, pca, held_out, ranks=[1, 3, mo.rank])
    assert np.all(np.diff(res.curve()) < 0) and res.coefficients.shape == (3, 4, mo.rank)
    ref = np.random.default_rng(8).normal(0, 30, (100, 3))
    gpmm = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=40.0, scaling=0.25)
    gm = restated(gpmm.device())
    assert gm.variance.max() <= 64.0
    check_generalization(ctx, gpmm.device(), gm, shapes_around(gm, 3, 9, spread=0.5), sorted({1, max(1, gm.rank // 2), gm.rank}),
                         f"GPMM M=100 rank={gm.rank}", cond_limit=1e7)


def test_generalization_reach_of_every_vertex(ctx):
    """130 vertices: a second slab step of two vertices.  Shape j + 1 is shape 0 with vertex j moved: each is checked on its own, so
    a vertex that the measure pass drops -- wherever the model's row order puts it -- shows in that shape's figures"""
    import gingr_amd as ga
    mo = mm.random_model(130, 17, 11)
    X = np.repeat(shapes_around(mo, 1, 7), 131, axis=0)
    for j in range(130):
        X[j + 1, j] += [3.0, -4.0, 12.0]
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        _, avg, mx = check_generalization(ctx, dm, mo, X, [17], "uploaded M=130 r=17, one vertex moved per shape", single=False)
        # every moved vertex shows in its shape's mean, far above the bound the figures were just held to
        assert np.all(np.abs(avg[0, 1:] - avg[0, 0]) > 1e6 * mm.projection_bounds(mo, X[:1], [17])["avg"][0, 0])
    finally:
        dm.close()


def test_row_order_shuffled_input_gives_permuted_results(ctx):
    """random points: the model's k-d order is not the caller's.  The same model and shapes with the points shuffled must give the
    same figures (the shapes go through model->perm) and the instances permuted."""
    import gingr_amd as ga
    mo = mm.random_model(130, 17, 11)
    p = np.random.default_rng(0).permutation(130)
    rows = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
    ms = mm.Model(mo.ref[p], mo.mean[p], mo.basis[rows], mo.variance)
    X = shapes_around(mo, 6, 21)
    A = np.random.default_rng(22).normal(0, 1, (6, 17))
    da, ds = ga.DeviceModel(ctx, host_model(mo)), ga.DeviceModel(ctx, host_model(ms))
    try:
        ca, aa, xa = da.project(X, [3, 17])
        cs, as_, xs = ds.project(np.ascontiguousarray(X[:, p]), [3, 17])
        b = mm.projection_bounds(mo, X, [3, 17])
        ratio("row order: coefficients", cs, ca, np.broadcast_to(b["coef"][:, :, None], ca.shape), factor=2.0)
        ratio("row order: avg", as_, aa, b["avg"], factor=2.0)
        ratio("row order: max", xs, xa, b["max"], factor=2.0)
        ratio("row order: instances", ds.instances(A), da.instances(A)[:, p], mm.instance_bound(ms, A), factor=2.0)
        tr = shapes_around(mo, 15, 23)
        ra = ga.ModelMetrics.specificity(ctx, da, tr, 9, alphas=A[:1].repeat(9, 0) * np.linspace(0.2, 2, 9)[:, None])
        rs = ga.ModelMetrics.specificity(ctx, ds, np.ascontiguousarray(tr[:, p]), 9, alphas=ra.alphas)
        assert np.array_equal(ra.argmin, rs.argmin)
        ratio("row order: min_avg", rs.min_avg, ra.min_avg, mm.specificity_bound(mo, tr, ra.alphas, [17]).max(axis=2), factor=2.0)
    finally:
        da.close()
        ds.close()


# ---------------------------------------------------------------------------------------------------------------- specificity
def check_specificity(ctx, dm, mo, train, A, ranks, label):
    import gingr_amd as ga
    res = ga.ModelMetrics.specificity(ctx, dm, train, A.shape[0], ranks=ranks, alphas=A)
    means, mn, am = mm.specificity(mo, train, A, ranks)
    bound = mm.specificity_bound(mo, train, A, ranks)
    # no two candidate means within 1 000 x the bound of each other (identical training shapes aside: their means are equal, and the
    # lower index must win)
    srt = np.sort(np.asarray(means, dtype=float), axis=2)
    gaps = np.diff(srt, axis=2)
    assert gaps.size == 0 or np.all((gaps > 1000.0 * bound.max()) | (gaps == 0.0)), "the inputs do not separate the candidates"
    picked = np.take_along_axis(bound, np.asarray(am)[:, :, None], axis=2)[:, :, 0]
    ratio(f"min_avg: {label}", res.min_avg, mn, picked)
    assert np.array_equal(res.argmin, am), label
    return res


@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, 2049])
def test_specificity_slab_edges(ctx, M):
    """S in {1, 63, 65} samples against n_train in {1, 15, 17} shapes, ranks 1, 5 and r"""
    import gingr_amd as ga
    r = 9 if M > 3 else 3
    mo = mm.random_model(M, r, 31 + M)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        for S, nt in ((1, 17), (63, 1), (65, 15)):
            A = np.random.default_rng(S).normal(0, 1, (S, r))
            check_specificity(ctx, dm, mo, shapes_around(mo, nt, 40 + nt, spread=3.0), A, sorted({1, min(5, r), r}), f"M={M} S={S} n_train={nt}")
    finally:
        dm.close()


def test_specificity_ties_exact_zero_and_blocks(ctx):
    """two identical training shapes: the lower index; a training shape that IS a sample (the output of instances()): distance
    exactly 0, the square root sees 0; 513 samples: two blocks of columns"""
    import gingr_amd as ga
    mo = mm.random_model(130, 17, 11)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        A = np.random.default_rng(1).normal(0, 1, (513, 17))
        train = shapes_around(mo, 6, 50, spread=0.3)   # (close to the mean: each of them is the nearest of some samples)
        train[4] = train[1]
        train[5] = dm.instances(A[7:8])[0]
        res = check_specificity(ctx, dm, mo, train, A, [17], "M=130, 513 samples, a tie and an exact hit")
        assert res.min_avg[0, 7] == 0.0 and res.argmin[0, 7] == 5
        assert np.any(res.argmin[0] == 1) and not np.any(res.argmin[0] == 4)
        only = ga.ModelMetrics.specificity(ctx, dm, train[[1, 4]], 20, alphas=A[:20])
        assert np.all(only.argmin == 0)
        drawn = ga.ModelMetrics.specificity(ctx, dm, train, 10, seed=3)
        assert np.array_equal(drawn.alphas, np.random.default_rng(3).standard_normal((10, 17)))
    finally:
        dm.close()


def test_specificity_reach_of_every_vertex(ctx):
    """two training shapes that differ in vertex j only, the second one closer to the sample there: it must win, for every j -- a pair
    pass that drops a vertex sees two equal shapes at that j and returns the first"""
    import gingr_amd as ga
    mo = mm.random_model(130, 9, 61)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        A = np.random.default_rng(2).normal(0, 1, (1, 9))
        sample = dm.instances(A)[0]
        far = sample + np.random.default_rng(3).normal(0, 3.0, sample.shape)
        for j in range(130):
            near = far.copy()
            near[j] = sample[j] + 0.5 * (far[j] - sample[j])
            res = ga.ModelMetrics.specificity(ctx, dm, np.stack([far, near]), 1, alphas=A)
            assert res.argmin[0, 0] == 1, j
    finally:
        dm.close()


# ------------------------------------------------------------------------------------------------------ determinism and errors
def test_two_calls_give_the_same_bits(ctx):
    import gingr_amd as ga
    mo = mm.random_model(257, 35, 13)
    dm = ga.DeviceModel(ctx, host_model(mo))
    try:
        X, A = shapes_around(mo, 20, 70), np.random.default_rng(71).normal(0, 1, (70, 35))
        first = dm.project(X, [1, 7, 35]) + (dm.instances(A),)
        second = dm.project(X, [1, 7, 35]) + (dm.instances(A),)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        s1 = ga.ModelMetrics.specificity(ctx, dm, X, 70, ranks=[7, 35], alphas=A)
        s2 = ga.ModelMetrics.specificity(ctx, dm, X, 70, ranks=[7, 35], alphas=A)
        assert np.array_equal(s1.min_avg, s2.min_avg) and np.array_equal(s1.argmin, s2.argmin)
    finally:
        dm.close()


def test_clean_errors(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    mo = mm.random_model(20, 6, 81)
    dm = ga.DeviceModel(ctx, host_model(mo))
    shard = ga.DeviceModel(ctx, host_model(mo), 0, 10)
    X, A = shapes_around(mo, 3, 82), np.random.default_rng(83).normal(0, 1, (4, 6))

    def refused(code, text, call):
        with pytest.raises(ga.GingrNativeError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
    try:
        refused(nat.ERR_BAD_ARGUMENT, "strictly increasing", lambda: dm.project(X, [3, 3]))
        refused(nat.ERR_BAD_ARGUMENT, "strictly increasing", lambda: dm.project(X, [4, 2]))
        refused(nat.ERR_BAD_ARGUMENT, "outside 1..6", lambda: dm.project(X, [7]))
        refused(nat.ERR_BAD_ARGUMENT, "outside 1..6", lambda: dm.project(X, [0, 2]))
        refused(nat.ERR_BAD_ARGUMENT, "ranks", lambda: dm.project(X, list(range(1, 7)) * 3))
        refused(nat.ERR_BAD_ARGUMENT, "0 shapes", lambda: dm.project(X[:0], [2]))
        refused(nat.ERR_BAD_ARGUMENT, "513 shapes", lambda: dm.project(np.repeat(X[:1], 513, axis=0), [2]))
        refused(nat.ERR_BAD_ARGUMENT, "513 training shapes", lambda: ga.ModelMetrics.specificity(ctx, dm, np.repeat(X[:1], 513, axis=0), 4, alphas=A))
        refused(nat.ERR_BAD_ARGUMENT, "0 training shapes", lambda: ga.ModelMetrics.specificity(ctx, dm, X[:0], 4, alphas=A))
        refused(nat.ERR_BAD_ARGUMENT, "n_samples", lambda: ga.ModelMetrics.specificity(ctx, dm, X, 0, alphas=A[:0]))
        refused(nat.ERR_BAD_ARGUMENT, "strictly increasing", lambda: ga.ModelMetrics.specificity(ctx, dm, X, 4, ranks=[2, 1], alphas=A))
        refused(nat.ERR_BAD_ARGUMENT, "n = 0", lambda: dm.instances(A[:0]))
        for call in (lambda: shard.project(X[:, :10], [2]), lambda: shard.instances(A),
                     lambda: ga.ModelMetrics.specificity(ctx, shard, X[:, :10], 4, alphas=A)):
            refused(nat.ERR_STATE, "row shard", call)
        bad = X.copy()
        bad[1, 5, 2] = np.nan
        refused(nat.ERR_NONFINITE, "shape 1", lambda: dm.project(bad, [2]))
        bad[1, 5, 2] = np.inf
        refused(nat.ERR_NONFINITE, "training shape 1", lambda: ga.ModelMetrics.specificity(ctx, dm, bad, 4, alphas=A))
        Ab = A.copy()
        Ab[2, 0] = np.nan
        refused(nat.ERR_NONFINITE, "coefficient vector 2", lambda: dm.instances(Ab))
        rc = ctx._lib.gingr_model_generalization(ctx.handle, dm.handle, 3, nat.dptr(X), 1, None, None, None, None)
        assert rc == nat.ERR_BAD_ARGUMENT
        # the context and the model stay usable
        coef, avg, mx = dm.project(X, [2, 6])
        assert np.all(np.isfinite(avg)) and np.all(mx >= avg)
    finally:
        dm.close()
        shard.close()


def test_report_worst_ratios():
    """(last in the file) the largest observed / bound per quantity of this run, for the record"""
    for name in sorted(WORST):
        print(f"worst observed / bound, {name}: {WORST[name]:.3g}")
