"""gingr_model_augment / PointDistributionModel.augmentModel / DeviceModel.augment against the numpy restatement
(tests/augment_restatement.py) and against exact properties of a sum of covariances.

What is compared is well posed whatever the eigenvalue gaps: reference (exact), mean, rank, eigenvalues (relative to the largest), the
covariance operator Q0 (Q0^T p) on random probes (relative to the result), and single eigenvectors only where the gap to both
neighbours is wide.  The two models of every case carry mean displacements of 12 and 9 units per coordinate, independent from vertex
to vertex, on a reference that spreads over 30 (test_augment_model_host.py asserts their size): the spatial row orders of a, b and the
result have nothing to do with each other.  The row permutations are not visible through the ABI; everything is compared per vertex
in the caller's order through downloads, where a wrong gather between the three orders is an O(1) error."""
import ctypes
import functools
import gc
import os

import numpy as np
import pytest

from tests import augment_restatement as ar
from tests.augment_restatement import CASES, ROUTE_SPREAD

pytestmark = pytest.mark.gpu

# 1000 x the spread between two correct host routes to the same model (augment_restatement.ROUTE_SPREAD, measured by the host test)
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


def compare(dm, m, a, b, label="", tol=TOL):
    """resident result dm (DeviceModel) against the restatement m of augment(a, b)"""
    host = dm.download()
    info = dm.host.augmentInfo
    lam1 = m.variance[0]
    np.testing.assert_array_equal(host.reference, m.reference)
    scale = np.abs(m.reference + m.mean).max()
    d_mean = np.abs(host.mean - m.mean).max() / scale
    print(f"{label} rank {host.rank} / {m.rank} of {info.columns} columns; mean {d_mean:.2e} of the largest coordinate")
    assert host.rank == m.rank == info.rank == dm.rank
    assert info.columns == a.rank + b.rank
    assert d_mean <= tol
    d_lam = np.abs(host.variance - m.variance).max() / lam1
    print(f"{label} eigenvalues {d_lam:.2e} of lambda_1")
    assert d_lam <= tol
    assert np.all(np.diff(host.variance) <= 0)
    P = ar.probes(3 * m.reference.shape[0])
    d_op = rel_columns(operator_of(host, P), m.operator(P))
    print(f"{label} operator on 8 probes {d_op:.2e} of the result")
    assert d_op <= tol
    # single eigenvectors where the gap to both neighbours (the first discarded eigenvalue included) exceeds 1e-3 lambda_1: a
    # perturbation E of the covariance turns such a vector by at most |E| / gap (Davis-Kahan), and |E| <= tol lambda_1 above
    lam_all = np.concatenate([m.all_variance, [0.0]])
    worst, checked = 0.0, 0
    for j in range(m.rank):
        gap = min(lam_all[j - 1] - lam_all[j] if j > 0 else np.inf, lam_all[j] - lam_all[j + 1]) / lam1
        if gap <= 1e-3:
            continue
        u, v = np.asarray(host.basis)[:, j], m.basis[:, j]
        d = np.linalg.norm(u - np.sign(u @ v) * v)
        worst, checked = max(worst, d * gap), checked + 1
        assert d <= tol / gap, (j, d, gap)
    print(f"{label} {checked} eigenvectors with a wide gap, worst deviation x gap {worst:.2e}")
    total = a.variance.sum() + b.variance.sum()
    assert abs(info.total_variance - total) <= tol * lam1 * (a.rank + b.rank)
    assert abs(info.kept_variance - m.variance.sum()) <= tol * lam1 * m.rank
    # (the kept sum adds eigenvalues, the total is the trace of the two moments: equal up to the rounding allowed above when all are kept)
    assert info.kept_variance <= info.total_variance + tol * lam1 * (a.rank + b.rank)
    return host


@pytest.mark.parametrize("M,ra,rb", CASES)
def test_augment_against_the_restatement(ctx, M, ra, rb):
    a, b = ar.case(M, ra, rb)
    m = ar.expected(M, ra, rb)
    da, db = upload(ctx, a), upload(ctx, b)
    dm = None
    try:
        # the sources come back per vertex in the caller's order, each from its own row order
        for d, src in ((da, a), (db, b)):
            h = d.download(basis=False)
            np.testing.assert_array_equal(h.reference, src.reference)
            np.testing.assert_array_equal(h.mean, src.mean)
        dm = da.augment(db)
        compare(dm, m, a, b, label=f"M={M} ra={ra} rb={rb}:")
        if (M, ra, rb) == (5, 10, 10):
            assert dm.rank == 15
        if (M, ra, rb) == (300, 200, 312):
            assert dm.rank == 512
    finally:
        for d in (dm, da, db):
            if d is not None:
                d.close()


@functools.lru_cache(maxsize=None)
def triple():
    """three models on one reference, 147 columns together on 450 coordinates: nothing is discarded"""
    a, b = ar.case(150, 17, 100)
    c = ar.random_model(np.random.default_rng(5), a.reference, 30, 200.0, 7.0)
    return a, b, c


def test_exact_properties_of_the_sum(ctx):
    a, b, c = triple()
    M = a.reference.shape[0]
    P = ar.probes(3 * M)
    da, db, dc = upload(ctx, a), upload(ctx, b), upload(ctx, c)
    made = []
    try:
        ab, ba = da.augment(db), db.augment(da)
        made += [ab, ba]
        assert ab.rank == ba.rank == 117
        hab, hba = ab.download(), ba.download()
        want = a.operator(P) + b.operator(P)
        d_ab, d_ba = rel_columns(operator_of(hab, P), want), rel_columns(operator_of(hba, P), want)
        print(f"operator against Q_a Q_a^T p + Q_b Q_b^T p: a+b {d_ab:.2e}, b+a {d_ba:.2e}")
        assert d_ab <= TOL and d_ba <= TOL
        np.testing.assert_array_equal(hab.mean, hba.mean)
        # marginal covariance of every vertex, in the caller's order
        cov, want_cov = ab.marginalCovariance(), da.marginalCovariance() + db.marginalCovariance()
        top = np.abs(want_cov).max()
        print(f"marginal covariance against the sum of the two: {np.abs(cov - want_cov).max() / top:.2e} of the largest entry")
        assert np.abs(cov - want_cov).max() <= TOL * top
        # the mean shape
        shape = ab.instance(np.zeros(ab.rank))
        want_shape = a.reference + a.mean + b.mean
        assert np.abs(shape - want_shape).max() <= TOL * np.abs(want_shape).max()
        # (a + b) + c against a + (b + c)
        bc = db.augment(dc)
        made.append(bc)
        left, right = ab.augment(dc), da.augment(bc)
        made += [left, right]
        assert left.rank == right.rank == 147
        hl, hr = left.download(), right.download()
        want3 = want + c.operator(P)
        d_l, d_r = rel_columns(operator_of(hl, P), want3), rel_columns(operator_of(hr, P), want3)
        print(f"(a+b)+c {d_l:.2e}, a+(b+c) {d_r:.2e}, one against the other {rel_columns(operator_of(hl, P), operator_of(hr, P)):.2e}")
        assert d_l <= TOL and d_r <= TOL and rel_columns(operator_of(hl, P), operator_of(hr, P)) <= TOL
        d_lam = np.abs(hl.variance - hr.variance).max() / hl.variance[0]
        assert d_lam <= TOL
        assert np.abs(hl.mean - (a.mean + b.mean + c.mean)).max() <= TOL * 40.0 and np.abs(hr.mean - hl.mean).max() <= TOL * 40.0
    finally:
        for d in made + [da, db, dc]:
            d.close()


def test_self_augment_and_rank_limits(ctx):
    a, b = ar.case(150, 17, 100)
    full = ar.expected(150, 17, 100)
    da, db = upload(ctx, a), upload(ctx, b)
    try:
        aa = da.augment(da)
        h = aa.download()
        assert aa.rank == a.rank and aa.host.augmentInfo.columns == 2 * a.rank
        d = np.abs(h.variance - 2.0 * a.variance).max() / (2.0 * a.variance[0])
        print(f"a + a: variance against 2 lambda {d:.2e}")
        assert d <= TOL
        np.testing.assert_array_equal(h.mean, 2.0 * a.mean)
        P = ar.probes(450)
        assert rel_columns(operator_of(h, P), 2.0 * a.operator(P)) <= TOL
        aa.close()
        # maxRank and a large relativeTolerance cut where the restatement cuts (the cut halfway between two eigenvalues)
        cut = 0.5 * (full.variance[30] + full.variance[31]) / full.variance[0]
        for kw, rkw in (({"maxRank": 9}, {"max_rank": 9}), ({"relativeTolerance": cut}, {"relative_tolerance": cut}),
                        ({"relativeTolerance": cut, "maxRank": 12}, {"relative_tolerance": cut, "max_rank": 12}), ({"maxRank": 4000}, {})):
            want = ar.augment(a, b, **rkw)
            dm = da.augment(db, **kw)
            print(f"{kw}: rank {dm.rank} / {want.rank}")
            assert dm.rank == want.rank
            np.testing.assert_allclose(dm.download(basis=False).variance, full.variance[:want.rank], rtol=0, atol=TOL * full.variance[0])
            info = dm.host.augmentInfo
            assert (info.kept_variance < info.total_variance) == (want.rank < 117)
            dm.close()
    finally:
        da.close()
        db.close()


def test_an_uploaded_basis_that_is_not_orthonormal(ctx):
    """S_a = Q_a^T Q_a of such a model is a full matrix: the diagonal blocks of G are used as stored"""
    import gingr_amd as ga
    rng = np.random.default_rng(21)
    M, ra, rb = 150, 20, 33
    ref = rng.normal(0.0, 30.0, (M, 3))
    Ba = rng.normal(size=(3 * M, ra)) / np.sqrt(3 * M) + rng.normal(size=(3 * M, 1)) / np.sqrt(3 * M)     # columns that share a direction
    Bb = rng.normal(size=(3 * M, rb)) / np.sqrt(3 * M)
    va, vb = ar.spectrum(ra, 300.0, 1e-2)[::-1].copy(), ar.spectrum(rb, 50.0, 1e-2)
    a = ar.Model(ref, rng.normal(0, 12, (M, 3)), va, Ba * np.sqrt(va)[None])
    b = ar.Model(ref, rng.normal(0, 9, (M, 3)), vb, Bb * np.sqrt(vb)[None])
    Sa = a.Q0.T @ a.Q0
    assert np.abs(Sa - np.diag(np.diag(Sa))).max() > 0.1 * np.abs(np.diag(Sa)).min()
    m = ar.augment(a, b)
    assert m.rank == ra + rb
    da = ga.DeviceModel(ctx, ga.PointDistributionModel(ref, a.mean, np.asfortranarray(Ba), va))
    db = ga.DeviceModel(ctx, ga.PointDistributionModel(ref, b.mean, np.asfortranarray(Bb), vb))
    dm = None
    try:
        dm = da.augment(db)
        host = dm.download()
        P = ar.probes(3 * M)
        d_op = rel_columns(operator_of(host, P), a.operator(P) + b.operator(P))
        d_lam = np.abs(host.variance - m.variance).max() / m.variance[0]
        print(f"non-orthonormal bases: operator {d_op:.2e}, eigenvalues {d_lam:.2e}")
        assert dm.rank == m.rank and d_op <= TOL and d_lam <= TOL
        info = dm.host.augmentInfo
        assert abs(info.total_variance - (np.trace(Sa) + np.trace(b.Q0.T @ b.Q0))) <= TOL * m.variance[0] * (ra + rb)
    finally:
        for d in (dm, da, db):
            if d is not None:
                d.close()


def test_the_result_is_a_model(ctx):
    import gingr_amd as ga
    a, b = ar.case(150, 17, 100)
    m = ar.expected(150, 17, 100)
    # through the public entry point, from host models (uploaded for the call)
    dev = ga.PointDistributionModel.augmentModel(ctx, host_model(a), host_model(b))
    assert isinstance(dev, ga.AugmentedDevicePointDistributionModel) and dev.augmentInfo.rank == dev.rank == 117
    dm = dev.device()
    compare(dm, m, a, b, label="augmentModel:")
    with pytest.raises(ValueError):
        dev._build(ctx, 0, 150)
    host = dev.to_host()
    np.testing.assert_array_equal(dev.reference, a.reference)
    assert np.abs(dev.mean - m.mean).max() <= TOL * 40.0
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
    post = dm.posterior(np.zeros((150, 3)), np.zeros(150), landmarks=ga.LandmarkCorrespondences(pids, pts, np.tile(0.25 * np.eye(3), (3, 1, 1))))
    hp = post.download(basis=False)
    assert post.rank == dm.rank and hp.variance.sum() < host.variance.sum() and np.isfinite(hp.mean).all()
    assert np.abs((hp.reference + hp.mean)[pids] - pts).max() < np.abs((host.reference + host.mean)[pids] - pts).max()
    post.close()
    # a device model and a DeviceModel mix, and augmenting the result again
    again = ga.PointDistributionModel.augmentModel(ctx, dev, upload(ctx, a), maxRank=20)
    assert again.rank == 20 and again.augmentInfo.columns == 117 + 17
    again.device().close()
    dm.close()


def test_cpd_on_the_femur_from_a_pca_plus_kernel_prior(ctx):
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
    prior = ga.PointDistributionModel.augmentModel(ctx, pca, [ga.GaussianKernelParameters(70.0, 20.0)], biasTolerance=0.02)
    info = prior.augmentInfo
    print(f"PCA rank {pca.rank} + kernel model: {info.columns} columns, rank {info.rank}, variance {info.kept_variance:.1f} of {info.total_variance:.1f}")
    assert info.columns > pca.rank + 5 and prior.rank == info.rank > pca.rank
    np.testing.assert_array_equal(prior.reference, pca.reference)        # the bias was built on the Procrustes target
    assert prior.cells is cells
    assert np.abs(prior.mean - pca.mean).max() <= TOL * np.abs(ref).max()      # (a kernel model has zero mean)
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
    a, b = ar.case(37, 1, 16)
    big_a, big_b = ar.case(300, 200, 312)
    da, db = upload(ctx, a), upload(ctx, b)
    lib = ctx._lib

    def refused(x, y, tol=1e-10, max_rank=0, word="", code=nat.ERR_BAD_ARGUMENT, info=True):
        h, inf = ctypes.c_void_p(), nat.AugmentInfo()
        rc = lib.gingr_model_augment(ctx.handle, x, y, tol, max_rank, ctypes.byref(h), ctypes.byref(inf) if info else None)
        text = lib.gingr_last_error(ctx.handle).decode()
        print(rc, text)
        assert rc == code and not h.value
        assert "model_augment" in text and word in text
        # the next valid call on the same context succeeds
        dm = da.augment(db)
        assert dm.rank == 17
        dm.close()

    other_ctx = ga.Context(0)
    closers = [da, db]
    try:
        refused(None, db.handle, word="null")
        refused(da.handle, None, word="null", info=False)
        assert lib.gingr_model_augment(ctx.handle, da.handle, db.handle, 1e-10, 0, None, None) == nat.ERR_BAD_ARGUMENT
        foreign = upload(other_ctx, b)
        closers.append(foreign)
        refused(da.handle, foreign.handle, word="another context")
        refused(foreign.handle, db.handle, word="another context")
        shard = ga.DeviceModel(ctx, host_model(b), 0, 20)            # (a shard is not finalized either)
        closers.append(shard)
        refused(da.handle, shard.handle, word="row shard")
        refused(shard.handle, da.handle, word="row shard")
        fewer = upload(ctx, ar.case(5, 3, 4)[0])
        closers.append(fewer)
        refused(da.handle, fewer.handle, word="points")
        moved = np.array(b.reference)
        moved[11, 2] = np.nextafter(moved[11, 2], np.inf)
        shifted = ga.DeviceModel(ctx, ga.PointDistributionModel(moved, np.array(b.mean), np.array(b.basis, order="F"), np.array(b.variance)))
        closers.append(shifted)
        refused(da.handle, shifted.handle, word="point 11")
        wa, wb = upload(ctx, big_a), upload(ctx, big_b)
        closers += [wa, wb]
        refused(wb.handle, wb.handle, word="truncate")
        refused(da.handle, db.handle, tol=-1e-3, word="negative")
        refused(da.handle, db.handle, tol=float("nan"), word="negative")
        refused(da.handle, db.handle, max_rank=-1, word="negative")
        refused(da.handle, db.handle, tol=1.0, word="rank 0")
        # through the Python layer
        with pytest.raises(ga.GingrNativeError) as e:
            da.augment(shifted)
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "point 11" in str(e.value)
        with pytest.raises(ValueError):
            ga.PointDistributionModel.augmentModel(ctx, host_model(a), [])
        with pytest.raises(ValueError):
            ga.PointDistributionModel.augmentModel(other_ctx, ga.GPMMTriangleMesh3D(ctx, a.reference, 0.1).Gaussian(30.0, 5.0), host_model(b))
    finally:
        for d in closers:
            d.close()
        other_ctx.close()


@pytest.mark.parametrize("M,ra,rb", [(150, 112, 113), (2500, 100, 8)])
def test_two_builds_give_identical_bits(ctx, M, ra, rb):
    a, b = ar.case(M, ra, rb)
    da, db = upload(ctx, a), upload(ctx, b)
    x, y = da.augment(db), da.augment(db)
    hx, hy = x.download(), y.download()
    for f in ("reference", "mean", "variance", "basis"):
        assert np.array_equal(np.asarray(getattr(hx, f)), np.asarray(getattr(hy, f))), f
    assert x.host.augmentInfo == y.host.augmentInfo
    for d in (x, y, da, db):
        d.close()


def test_create_and_destroy_returns_device_memory(ctx):
    """Thirty augmentations at M = 100 000 with 8 + 24 columns must not cost device memory.  The buffers of a call that scale with the
    input, left behind once per call, exceed the bound: the result model 77 MiB, the slab partials of the cross Gram pass 3 MiB --
    90 MiB over the thirty calls."""
    import torch

    def free_bytes():
        torch.cuda.synchronize(0)
        return torch.cuda.mem_get_info(0)[0]

    M, cycles, bound = 100_000, 30, 64 << 20
    rng = np.random.default_rng(4)
    ref = rng.normal(0.0, 30.0, (M, 3))
    da = upload(ctx, ar.random_model(rng, ref, 8, 400.0, 12.0))
    db = upload(ctx, ar.random_model(rng, ref, 24, 90.0, 9.0))
    assert cycles * 768 * 16 * 32 * 8 > bound                   # (the smaller of the buffers above, leaked every cycle)

    def cycle():
        dm = da.augment(db)
        assert dm.rank == 32
        dm.close()

    cycle()
    gc.collect()
    before = free_bytes()
    for _ in range(cycles):
        cycle()
    gc.collect()
    after = free_bytes()
    da.close()
    db.close()
    assert before - after < bound, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
