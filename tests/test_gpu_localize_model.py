"""gingr_model_localize / PointDistributionModel.localizeModel / DeviceModel.localize against the numpy restatement
(tests/localize_restatement.py) and against exact properties of a tapered covariance.

What is compared is well posed whatever the pivots and the eigenvalue gaps: reference and mean (exact), column count and rank, the
eigenvalues (relative to the largest), the covariance operator Q'(Q'^T p) on random probes against K p of the dense K, the 3 x 3
marginal blocks, and single eigenvectors only where the gap to both neighbours is wide.  Where the factor stops before the end (a
tolerance or the ceiling of 512 columns) the pivots may differ from the restatement's, and the bound is the one that holds for any
pivot sequence: the residual K - Q'Q'^T is positive semi-definite with the trace the info reports, so |K p - Q'Q'^T p| <= that trace
times |p|.  The sources carry mean displacements of 12 units per coordinate, independent from vertex to vertex, on a reference that
spreads over 30: the model's row order (the spatial order of reference + mean) has nothing to do with the caller's, nor with the
order of the reference alone, over which the taper is taken.  Everything is compared per vertex in the caller's order through
downloads, where a wrong gather between the orders is an O(1) error."""
import ctypes
import gc
import os

import numpy as np
import pytest

from tests import localize_restatement as lr
from tests.localize_restatement import FULL_CASES, PIVOT_STABLE, ROUTE_SPREAD, STOPPED_CASES, TOLERANCE_REACHED

pytestmark = pytest.mark.gpu

# 1000 x the spread between two correct host routes to the same model (localize_restatement.ROUTE_SPREAD, measured by the host test)
TOL = 1000.0 * ROUTE_SPREAD


def host_model(m):
    import gingr_amd as ga
    return ga.PointDistributionModel(np.array(m.reference), np.array(m.mean), np.array(m.basis, order="F"), np.array(m.variance))


def upload(ctx, m):
    import gingr_amd as ga
    return ga.DeviceModel(ctx, host_model(m))


def q0_of(host):
    return np.asarray(host.basis) * np.sqrt(np.asarray(host.variance))[None, :]


def operator_of(host, P):
    Q = q0_of(host)
    return Q @ (Q.T @ P)


def rel_columns(x, want):
    return float((np.linalg.norm(x - want, axis=0) / np.linalg.norm(want, axis=0)).max())


def blocks6(K):
    """(M, 6): {xx, xy, xz, yy, yz, zz} of the diagonal 3 x 3 blocks of a (3M, 3M) matrix"""
    M = K.shape[0] // 3
    i = 3 * np.arange(M)
    return np.stack([K[i, i], K[i, i + 1], K[i, i + 2], K[i + 1, i + 1], K[i + 1, i + 2], K[i + 2, i + 2]], axis=1)


@pytest.mark.parametrize("case", FULL_CASES)
def test_full_factorisations_against_the_dense_covariance(ctx, case):
    M, r, sigma, tol = case
    src, K, want = lr.source(M, r), lr.case_K(M, r, sigma), lr.expected(*case)
    m = want.model
    lam1 = m.variance[0]
    ds = upload(ctx, src)
    dm = None
    try:
        dm = ds.localize(sigma, relativeTolerance=tol)
        info, host = dm.host.localizeInfo, dm.download()
        np.testing.assert_array_equal(host.reference, src.reference)
        np.testing.assert_array_equal(host.mean, src.mean)
        print(f"{case}: {info.columns} columns (restatement {want.columns}), rank {host.rank} / {m.rank}, residual fraction {info.residual_fraction:.2e}")
        if case == (37, 1, 25.0, 0.0):
            assert 37 <= info.columns <= 3 * M         # (rounding noise may pivot a few more entries; the cutoff removes them)
        else:
            assert info.columns == 3 * M
        assert host.rank == m.rank == info.rank == dm.rank
        assert info.tolerance_reached
        d_lam = np.abs(host.variance - m.variance).max() / lam1
        print(f"{case}: eigenvalues {d_lam:.2e} of lambda_1")
        assert d_lam <= TOL and np.all(np.diff(host.variance) <= 0)
        P = lr.probes(3 * M)
        d_op = rel_columns(operator_of(host, P), K @ P)
        print(f"{case}: operator on 8 probes {d_op:.2e} of K p")
        assert d_op <= TOL
        cov, want_cov = dm.marginalCovariance(), blocks6(K)
        d_cov = np.abs(cov - want_cov).max() / np.abs(want_cov).max()
        print(f"{case}: marginal covariance {d_cov:.2e} of the largest entry")
        assert d_cov <= TOL
        # single eigenvectors where the gap to both neighbours exceeds 1e-3 lambda_1: a perturbation E of the covariance turns such a
        # vector by at most |E| / gap (Davis-Kahan), and |E| <= TOL lambda_1 above
        lam_all = np.concatenate([m.all_variance, [0.0]])
        worst, checked = 0.0, 0
        for j in range(m.rank):
            gap = min(lam_all[j - 1] - lam_all[j] if j > 0 else np.inf, lam_all[j] - lam_all[j + 1]) / lam1
            if gap <= 1e-3:
                continue
            u, v = np.asarray(host.basis)[:, j], m.basis[:, j]
            d = np.linalg.norm(u - np.sign(u @ v) * v)
            worst, checked = max(worst, d * gap), checked + 1
            assert d <= TOL / gap, (j, d, gap)
        print(f"{case}: {checked} eigenvectors with a wide gap, worst deviation x gap {worst:.2e}")
        assert abs(info.total_variance - src.variance.sum()) <= TOL * lam1 * r
        assert abs(info.kept_variance - m.variance.sum()) <= TOL * lam1 * m.rank
    finally:
        for d in (dm, ds):
            if d is not None:
                d.close()


@pytest.mark.parametrize("case", STOPPED_CASES)
def test_tolerance_and_ceiling_stops(ctx, case):
    M, r, sigma, tol = case
    src, K, want = lr.source(M, r), lr.case_K(M, r, sigma), lr.expected(*case)
    lam1 = want.model.variance[0]
    ds = upload(ctx, src)
    dm = None
    try:
        dm = ds.localize(sigma, relativeTolerance=tol)
        info, host = dm.host.localizeInfo, dm.download()
        np.testing.assert_array_equal(host.reference, src.reference)
        np.testing.assert_array_equal(host.mean, src.mean)
        print(f"{case}: {info.columns} columns (restatement {want.columns}), rank {host.rank}, residual fraction {info.residual_fraction:.3e} "
              f"(restatement {want.residual_fraction:.3e}), tolerance reached {info.tolerance_reached}")
        trace = src.variance.sum()
        # the residual K - Q'Q'^T is positive semi-definite, so its norm is at most its trace
        P = lr.probes(3 * M)
        err = np.linalg.norm(K @ P - operator_of(host, P), axis=0)
        bound = (info.residual_fraction * trace + TOL * lam1) * np.linalg.norm(P, axis=0)
        print(f"{case}: |K p - Q'Q'^T p| / bound at most {(err / bound).max():.3f}")
        assert np.all(err <= bound)
        assert abs(info.total_variance - trace) <= TOL * lam1 * r
        # no eigenvalue of these cases lies near the cutoff (host test): every column is kept, the kept variance is the factor's trace
        assert host.rank == info.rank == info.columns
        assert abs(info.total_variance - info.kept_variance - info.residual_fraction * info.total_variance) <= TOL * lam1 * info.columns
        assert abs(info.kept_variance - host.variance.sum()) <= TOL * lam1 * info.columns
        var = dm.marginalCovariance()[:, [0, 3, 5]].sum(axis=1)
        src_var = (src.Q0 * src.Q0).sum(axis=1).reshape(M, 3).sum(axis=1)
        print(f"{case}: largest excess of a vertex's variance over the source's {(var - src_var).max() / src_var.max():.2e} of the largest")
        assert np.all(var <= src_var + TOL * src_var.max())
        assert info.tolerance_reached == TOLERANCE_REACHED[case]
        assert (info.residual_fraction < tol) == info.tolerance_reached
        if case in PIVOT_STABLE:
            assert info.columns == want.columns
        elif info.tolerance_reached:
            assert abs(info.columns - want.columns) <= 0.1 * want.columns
        else:
            assert info.columns == 512
    finally:
        for d in (dm, ds):
            if d is not None:
                d.close()


def test_a_wide_taper_gives_the_source_back(ctx):
    src = lr.random_model(np.random.default_rng(17), lr.source(150, 100).reference, 17, 400.0, 12.0)
    ds = upload(ctx, src)
    dm = ds.localize(1e9, relativeTolerance=1e-10)
    try:
        host = dm.download()
        P = lr.probes(450)
        d_op = rel_columns(operator_of(host, P), src.operator(P))
        d_lam = np.abs(host.variance - src.variance).max() / src.variance[0] if host.rank == 17 else np.inf
        print(f"sigma = 1e9: rank {host.rank} of {dm.host.localizeInfo.columns} columns, operator {d_op:.2e}, eigenvalues {d_lam:.2e}")
        assert dm.rank == host.rank == 17 and d_op <= TOL and d_lam <= TOL
        np.testing.assert_array_equal(host.mean, src.mean)
    finally:
        dm.close()
        ds.close()


def test_localizing_twice_is_localizing_once_with_a_narrower_taper(ctx):
    """g_sigma^2 = g_(sigma / sqrt 2): both sides are full factorisations at M = 86 (tolerance 0)"""
    M, r, sigma, _ = (86, 20, 30.0, 0.0)
    ds = upload(ctx, lr.source(M, r))
    made = [ds]
    try:
        once = ds.localize(sigma, relativeTolerance=0.0)
        made.append(once)
        twice = once.localize(sigma, relativeTolerance=0.0)
        made.append(twice)
        narrow = ds.localize(sigma / np.sqrt(2.0), relativeTolerance=0.0)
        made.append(narrow)
        assert once.rank == twice.rank == narrow.rank == 3 * M
        P = lr.probes(3 * M)
        a, b = operator_of(twice.download(), P), operator_of(narrow.download(), P)
        print(f"twice at sigma against once at sigma / sqrt 2: operator {rel_columns(a, b):.2e}")
        assert rel_columns(a, b) <= TOL
    finally:
        for d in made:
            d.close()


def test_max_rank_cuts_where_the_restatement_cuts(ctx):
    case = (86, 20, 30.0, 0.0)
    full, cut = lr.expected(*case), lr.expected(*case, 9)
    ds = upload(ctx, lr.source(86, 20))
    made = [ds]
    try:
        whole = ds.localize(30.0, relativeTolerance=0.0)
        made.append(whole)
        dm = ds.localize(30.0, relativeTolerance=0.0, maxRank=9)
        made.append(dm)
        assert dm.rank == cut.model.rank == 9 and dm.host.localizeInfo.columns == 258
        var = dm.download(basis=False).variance
        np.testing.assert_array_equal(var, whole.download(basis=False).variance[:9])     # the leading ones of the uncut result
        np.testing.assert_allclose(var, full.model.variance[:9], rtol=0, atol=TOL * full.model.variance[0])
        info = dm.host.localizeInfo
        assert info.kept_variance < info.total_variance and abs(info.kept_variance - var.sum()) <= TOL * var[0] * 9
        big = ds.localize(30.0, relativeTolerance=0.0, maxRank=4000)
        made.append(big)
        assert big.rank == 258
    finally:
        for d in made:
            d.close()


def test_the_result_is_a_model(ctx):
    import gingr_amd as ga
    M, r, sigma, tol = (150, 100, 15.0, 0.0)
    src, want = lr.source(M, r), lr.expected(150, 100, 15.0, 0.0)
    cells = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    # through the public entry point, from a host model (uploaded for the call)
    dev = ga.PointDistributionModel.localizeModel(ctx, host_model(src), sigma, relativeTolerance=tol, cells=cells)
    assert isinstance(dev, ga.LocalizedDevicePointDistributionModel) and isinstance(dev.localizeInfo, ga.LocalizeInfo)
    assert dev.localizeInfo.rank == dev.rank == want.model.rank == 450 and dev.cells is cells
    with pytest.raises(ValueError):
        dev._build(ctx, 0, M)
    dm = dev.device()
    host = dev.to_host()
    np.testing.assert_array_equal(dev.reference, src.reference)
    np.testing.assert_array_equal(dev.mean, src.mean)
    np.testing.assert_allclose(host.variance, want.model.variance, rtol=0, atol=TOL * want.model.variance[0])
    # instance, coefficients
    alpha = np.random.default_rng(2).normal(size=dm.rank)
    shape = host.reference + host.mean + (q0_of(host) @ alpha).reshape(-1, 3)
    np.testing.assert_allclose(dm.instance(alpha), shape, rtol=0, atol=1e-9)
    back = dm.coefficients(shape)
    # (GP regression with noise 1e-5 I: coefficient j comes back scaled by lambda_j / (lambda_j + 1e-5))
    assert np.abs(back - alpha).max() <= 2.0 * 1e-5 / host.variance.min() * np.abs(alpha).max()
    # truncate
    t = dev.truncate(5)
    assert t.rank == 5
    np.testing.assert_array_equal(t.variance, dev.variance[:5])
    np.testing.assert_array_equal(np.asarray(t.basis), np.asarray(dev.basis)[:, :5])
    t.device().close()
    # posterior: three landmarks pull the mean; the result is a model of the same rank with less variance
    pids = np.array([3, 70, 140], dtype=np.int32)
    pts = (host.reference + host.mean)[pids] + 2.0
    post = dm.posterior(np.zeros((M, 3)), np.zeros(M), landmarks=ga.LandmarkCorrespondences(pids, pts, np.tile(0.25 * np.eye(3), (3, 1, 1))))
    hp = post.download(basis=False)
    assert post.rank == dm.rank and hp.variance.sum() < host.variance.sum() and np.isfinite(hp.mean).all()
    assert np.abs((hp.reference + hp.mean)[pids] - pts).max() < np.abs((host.reference + host.mean)[pids] - pts).max()
    post.close()
    # augment with a kernel model, compactness
    few = ga.PointDistributionModel.localizeModel(ctx, dev, 60.0, relativeTolerance=0.05, maxRank=40)      # from a device-built model
    assert isinstance(few, ga.LocalizedDevicePointDistributionModel) and few.rank <= 40 and few.cells is cells
    prior = ga.PointDistributionModel.augmentModel(ctx, few, [ga.GaussianKernelParameters(40.0, 5.0)], biasTolerance=0.1)
    assert prior.rank > few.rank and prior.cells is cells
    frac = ga.ModelMetrics.compactness(few)
    assert frac.shape == (few.rank,) and np.all(np.diff(frac) > 0) and abs(frac[-1] - 1.0) < 1e-12
    prior.device().close()
    few.device().close()
    # from a device-built PCA model and from a DeviceModel
    rng = np.random.default_rng(3)
    shapes = np.stack([src.reference + src.mean + (src.Q0[:, :6] @ rng.normal(size=6)).reshape(-1, 3) for _ in range(5)])
    pca = ga.PointDistributionModel.createUsingPCA(ctx, src.reference, shapes, cells=cells)
    loc = ga.PointDistributionModel.localizeModel(ctx, pca, 25.0, relativeTolerance=0.01)
    assert isinstance(loc, ga.LocalizedDevicePointDistributionModel) and loc.rank > pca.rank == 4 and loc.cells is cells
    np.testing.assert_array_equal(loc.mean, pca.mean)
    again = ga.PointDistributionModel.localizeModel(ctx, loc.device(), 25.0, relativeTolerance=0.01, maxRank=20)
    assert again.rank == 20 and again.localizeInfo.columns >= 20 and again.cells is cells
    for d in (again, loc, pca):
        d.device().close()
    dm.close()


def test_cpd_on_the_femur_from_a_localized_pca_prior(ctx):
    import gingr_amd as ga
    here = os.path.dirname(os.path.abspath(__file__))
    d = np.load(os.path.join(here, "golden", "inputs.npz"))
    cells = np.load(os.path.join(here, "golden", "femur_mesh.npz"))["femur_cells"].astype(np.int32)
    ref, target = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
    gpmm = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01, cells=cells).Gaussian(sigma=70.0, scaling=50.0)
    rng = np.random.default_rng(1)
    shapes = np.stack([gpmm.device().instance(rng.normal(0, 0.7, gpmm.rank)) for _ in range(6)])
    pca = ga.PointDistributionModel.createUsingPCA(ctx, ref, shapes, alignment="gpa", cells=cells)
    assert pca.rank == 5
    prior = ga.PointDistributionModel.localizeModel(ctx, pca, 70.0, relativeTolerance=0.02)
    info = prior.localizeInfo
    print(f"PCA rank {pca.rank} localized at sigma 70: {info.columns} columns, rank {info.rank}, residual fraction {info.residual_fraction:.3e}, "
          f"variance {info.kept_variance:.1f} of {info.total_variance:.1f}")
    assert prior.rank == info.rank > pca.rank
    np.testing.assert_array_equal(prior.reference, pca.reference)
    np.testing.assert_array_equal(prior.mean, pca.mean)
    assert prior.cells is cells
    var = prior.device().marginalCovariance()[:, [0, 3, 5]].sum(axis=1)
    pca_var = pca.device().marginalCovariance()[:, [0, 3, 5]].sum(axis=1)
    assert np.all(var <= pca_var + TOL * pca_var.max())
    cpd = ga.CpdRegistration(ctx)
    cfg = ga.CpdConfiguration(maxIterations=15, w=0.0, threshold=1e-10)
    best = cpd.run(cpd.createInitialState(prior, target, cfg, transform=ga.GlobalTranformationType.RigidTransforms))
    cpd.close()
    print(f"CPD of the femur pair: status {best.general.status} after {best.general.iteration} iterations")
    assert best.general.status in (ga.FittingStatuses.Converged, ga.FittingStatuses.MaxIteration) or best.general.iteration == 15
    assert np.isfinite(best.general.fit).all()
    for dev in (prior, pca, gpmm):
        dev.device().close()


def test_errors_leave_the_context_usable(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    src = lr.source(37, 16)
    ds = upload(ctx, src)
    lib = ctx._lib

    def refused(model, sigma=25.0, tol=0.01, max_rank=0, word="", code=nat.ERR_BAD_ARGUMENT, info=True):
        h, inf = ctypes.c_void_p(1), nat.LocalizeInfo(7, 7, 7, 7.0, 7.0, 7.0)
        rc = lib.gingr_model_localize(ctx.handle, model, sigma, tol, max_rank, ctypes.byref(h), ctypes.byref(inf) if info else None)
        text = lib.gingr_last_error(ctx.handle).decode()
        print(rc, text)
        assert rc == code and not h.value
        assert "model_localize" in text and word in text
        if info:
            assert (inf.columns, inf.rank, inf.tolerance_reached, inf.residual_fraction, inf.total_variance, inf.kept_variance) == (0, 0, 0, 0.0, 0.0, 0.0)
        # the next valid call on the same context succeeds
        dm = ds.localize(25.0, relativeTolerance=0.0)
        assert dm.rank == 111
        dm.close()

    other_ctx = ga.Context(0)
    closers = [ds]
    try:
        refused(None, word="null")
        refused(None, word="null", info=False)
        assert lib.gingr_model_localize(ctx.handle, ds.handle, 25.0, 0.01, 0, None, None) == nat.ERR_BAD_ARGUMENT
        foreign = upload(other_ctx, src)
        closers.append(foreign)
        refused(foreign.handle, word="another context")
        shard = ga.DeviceModel(ctx, host_model(src), 0, 20)            # (a shard is not finalized either)
        closers.append(shard)
        refused(shard.handle, word="row shard")
        for bad in (0.0, -3.0, float("inf"), float("nan")):
            refused(ds.handle, sigma=bad, word="sigma")
        for bad in (-1e-3, 1.0, 1.5, float("nan")):
            refused(ds.handle, tol=bad, word="relative_tolerance")
        refused(ds.handle, max_rank=-1, word="max_rank")
        # a model whose basis is all zero: nothing to pivot
        zero = ga.DeviceModel(ctx, ga.PointDistributionModel(np.array(src.reference), np.array(src.mean), np.zeros((111, 2), order="F"), np.ones(2)))
        closers.append(zero)
        refused(zero.handle, word="rank 0")
        # (GINGR_ERR_NONFINITE has no test: a basis that is not finite does not survive gingr_model_finalize, so no finalized model has one)
        # through the Python layer
        with pytest.raises(ga.GingrNativeError) as e:
            ds.localize(-1.0)
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "sigma" in str(e.value)
        with pytest.raises(ValueError):
            ga.PointDistributionModel.localizeModel(other_ctx, ga.GPMMTriangleMesh3D(ctx, src.reference, 0.1).Gaussian(30.0, 5.0), 20.0)
    finally:
        for d in closers:
            d.close()
        other_ctx.close()


@pytest.mark.parametrize("case", [(86, 20, 30.0, 0.0), (2500, 3, 500.0, 1e-8)])
def test_two_builds_give_identical_bits(ctx, case):
    M, r, sigma, tol = case
    ds = upload(ctx, lr.source(M, r))
    x, y = ds.localize(sigma, relativeTolerance=tol), ds.localize(sigma, relativeTolerance=tol)
    hx, hy = x.download(), y.download()
    for f in ("reference", "mean", "variance", "basis"):
        assert np.array_equal(np.asarray(getattr(hx, f)), np.asarray(getattr(hy, f))), f
    assert x.host.localizeInfo == y.host.localizeInfo
    for d in (x, y, ds):
        d.close()


def test_create_and_destroy_returns_device_memory(ctx):
    """Thirty localizations at M = 100 000, r = 8, sigma = 2000, maxRank = 16 must not cost device memory.  The buffers of a call that
    scale with the input, left behind once per call, exceed the bound: the transposed basis Qt 18 MiB (8 x 300 000 doubles), the
    result model at least as much, the factor's column buffer 1.1 GiB -- 550 MiB over the thirty calls for the smallest of them."""
    import torch

    def free_bytes():
        torch.cuda.synchronize(0)
        return torch.cuda.mem_get_info(0)[0]

    M, cycles, bound = 100_000, 30, 64 << 20
    rng = np.random.default_rng(4)
    ref = rng.normal(0.0, 30.0, (M, 3))
    ds = upload(ctx, lr.random_model(rng, ref, 8, 400.0, 12.0))
    assert cycles * 8 * 3 * M * 8 > bound                       # (the transposed basis, leaked every cycle)

    def cycle():
        dm = ds.localize(2000.0, maxRank=16)
        assert 1 <= dm.rank <= 16
        dm.close()

    cycle()
    gc.collect()
    before = free_bytes()
    for _ in range(cycles):
        cycle()
    gc.collect()
    after = free_bytes()
    ds.close()
    assert before - after < bound, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
