"""gingr_model_from_shapes / PointDistributionModel.createUsingPCA against the numpy restatement (tests/pca_restatement.py).

What is compared is well posed whatever the eigenvalue gaps: mean, rank, eigenvalues (relative to the largest), the covariance
operator Q0 (Q0^T p) on random probes (relative to the result), and single eigenvectors only where the gap to both neighbours is
wide.  The ABI does not hand back the aligned shapes; they are checked through what the model keeps of them -- the final Procrustes
target (its reference), the mean, the sweep count and the covariance -- and, for the rigid mode, exactly: a set {shape, reference}
aligned to the reference has the mean (aligned shape + reference) / 2.  For generalised Procrustes this is weaker than comparing
the aligned shapes one by one: a deviation of single shapes that left target, mean and covariance alone would pass."""
import functools
import gc

import numpy as np
import pytest

from tests import pca_restatement as pr
from tests.pca_restatement import LOW_RANK, ROUTE_SPREAD, SHAPES, dataset, low_rank_dataset

pytestmark = pytest.mark.gpu

# 1000 x the spread between two correct host routes to the same model (pca_restatement.ROUTE_SPREAD, measured by the host test)
TOL = 1000.0 * ROUTE_SPREAD

MODES = {"none": 0, "rigid": 1, "gpa": 2}


@functools.lru_cache(maxsize=None)
def case(M, n, alignment="none", moved=False):
    """(ref, shapes, restatement); moved: every shape under a random rigid motion of its own"""
    ref, X = dataset(M, n)
    if moved:
        rng = np.random.default_rng(77 + M + n)
        X = np.stack([x @ R.T + t for x, (R, t) in ((x, pr.random_rigid(rng)) for x in X)])
    m = pr.pca_model(ref, X, MODES[alignment])
    for a in (ref, X, m.Q0, m.variance, m.mean, m.reference):
        a.setflags(write=False)
    return ref, X, m


def build(ctx, ref, X, alignment="none", **kw):
    import gingr_amd as ga
    return ga.PointDistributionModel.createUsingPCA(ctx, ref, X, alignment=alignment, **kw)


def q0_of(host):
    return np.asarray(host.basis) * np.sqrt(np.asarray(host.variance))[None, :]


def compare(dev, m, X, tol=TOL, label=""):
    """device model (DevicePointDistributionModel) against the restatement m"""
    host = dev.to_host()
    scale = np.abs(X).max()
    lam1 = m.variance[0]
    d_ref = np.abs(host.reference - m.reference).max() / scale
    d_mean = np.abs(host.mean - m.mean).max() / scale
    print(f"{label} rank {host.rank} / {m.rank}; reference {d_ref:.2e}, mean {d_mean:.2e} (of the largest coordinate)")
    assert host.rank == m.rank == dev.pcaInfo.rank
    assert d_ref <= tol and d_mean <= tol
    d_lam = np.abs(host.variance - m.variance).max() / lam1
    print(f"{label} eigenvalues {d_lam:.2e} of lambda_1")
    assert d_lam <= tol
    assert np.all(np.diff(host.variance) <= 0)
    Q = q0_of(host)
    P = np.random.default_rng(9).normal(size=(Q.shape[0], 8))
    a, b = Q @ (Q.T @ P), m.operator(P)
    d_op = (np.linalg.norm(a - b, axis=0) / np.linalg.norm(b, axis=0)).max()
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
    info = dev.pcaInfo
    assert info.kept_variance <= info.total_variance * (1 + 1e-15)
    assert abs(info.kept_variance - m.variance.sum()) <= tol * lam1 * m.rank
    assert abs(info.total_variance - m.all_variance.sum()) <= tol * lam1 * len(m.all_variance)
    return host


@pytest.mark.parametrize("M,n", SHAPES)
def test_pca_against_the_restatement(ctx, M, n):
    ref, X, m = case(M, n)
    dev = build(ctx, ref, X)
    host = compare(dev, m, X, label=f"M={M} n={n}:")
    if (M, n) == (37, 2):
        assert host.rank == 1
    if (M, n) == (5, 20):
        assert host.rank <= 15
    np.testing.assert_array_equal(host.reference, ref)
    dev.device().close()


@pytest.mark.parametrize("M,n,r", LOW_RANK)
def test_shapes_from_a_low_rank_model(ctx, M, n, r):
    """a Gram matrix with a null space of many dimensions (n - r): the rank is r, nothing of the null space comes back"""
    ref, X = low_rank_dataset(M, n, r)
    m = pr.pca_model(ref, X)
    assert m.rank == r
    dev = build(ctx, ref, X)
    compare(dev, m, X, label=f"rank {r} shapes, M={M} n={n}:")
    dev.device().close()


def test_known_spectrum_through_the_abi(ctx):
    rng = np.random.default_rng(3)
    lam = np.array([400.0, 90.0, 25.0, 4.0, 0.5, 0.01])
    ref, shapes, U = pr.known_spectrum_shapes(rng, 150, 21, lam)
    dev = build(ctx, ref, shapes, relativeTolerance=1e-8)
    host = dev.to_host()
    assert host.rank == 6
    print("known spectrum, relative to lambda_1:", np.abs(host.variance - lam) / lam[0])
    assert np.abs(host.variance - lam).max() <= TOL * lam[0]
    assert np.abs(np.abs((np.asarray(host.basis) * U).sum(axis=0)) - 1.0).max() <= TOL / (0.01 / 400.0)
    assert np.abs(host.mean).max() <= TOL * np.abs(shapes).max()
    dev.device().close()


@pytest.mark.parametrize("M,n", [(257, 17), (1000, 40), (5000, 6)])
def test_rigid_alignment_gives_the_aligned_shapes(ctx, M, n):
    """mode 1, shape by shape: {shape, reference} aligned to the reference has the mean (aligned + reference) / 2"""
    ref, X, m = case(M, n, "rigid", True)
    scale = np.abs(X).max()
    for i in (0, n - 1):
        dev = build(ctx, ref, np.stack([X[i], ref]), "rigid")
        aligned = 2.0 * (dev.reference + dev.mean) - ref
        d = np.abs(aligned - m.aligned.shapes[i]).max() / scale
        print(f"M={M} shape {i}: aligned shape {d:.2e} of the largest coordinate")
        assert d <= TOL
        dev.device().close()
    dev = build(ctx, ref, X, "rigid")
    assert dev.pcaInfo.gpa_sweeps == 0
    compare(dev, m, X, label=f"rigid M={M} n={n}:")
    dev.device().close()


@pytest.mark.parametrize("M,n", [(257, 17), (1000, 40), (5000, 6)])
def test_generalised_procrustes_against_the_restatement(ctx, M, n):
    ref, X, m = case(M, n, "gpa", True)
    dev = build(ctx, ref, X, "gpa")
    info = dev.pcaInfo
    print(f"gpa M={M} n={n}: sweeps {info.gpa_sweeps} / {m.aligned.sweeps}, last change {info.gpa_last_change:.6e} / {m.aligned.last_change:.6e}")
    assert info.gpa_sweeps == m.aligned.sweeps
    assert abs(info.gpa_last_change - m.aligned.last_change) <= TOL * np.abs(X).max()
    compare(dev, m, X, label=f"gpa M={M} n={n}:")          # reference = the final target, mean, covariance of the aligned shapes
    dev.device().close()
    # the stopping rule: a loose tolerance ends the sweeps early, on the device as in the restatement
    loose = pr.align_shapes(ref, X, 2, 5, 1e-2)
    dev = build(ctx, ref, X, "gpa", gpaMaxIterations=5, gpaTolerance=1e-2)
    assert dev.pcaInfo.gpa_sweeps == loose.sweeps < 5
    dev.device().close()


def test_gpa_is_invariant_under_rigid_motions_of_the_inputs(ctx):
    """alignment without the restatement: independent rigid motions of the inputs change nothing the model keeps"""
    ref, X, _ = case(257, 17)
    _, Xm, _ = case(257, 17, "gpa", True)
    da, db = build(ctx, ref, X, "gpa"), build(ctx, ref, Xm, "gpa")
    a, b = da.to_host(), db.to_host()
    da.device().close()
    db.device().close()
    assert a.rank == b.rank
    d_lam = np.abs(a.variance - b.variance).max() / a.variance[0]
    Qa, Qb = q0_of(a), q0_of(b)
    P = np.random.default_rng(9).normal(size=(Qa.shape[0], 8))
    ra, rb = Qa @ (Qa.T @ P), Qb @ (Qb.T @ P)
    d_op = (np.linalg.norm(ra - rb, axis=0) / np.linalg.norm(ra, axis=0)).max()
    print(f"invariance: eigenvalues {d_lam:.2e}, operator {d_op:.2e}")
    assert d_lam <= TOL and d_op <= TOL


def test_rank_deficiency_and_rank_limit(ctx):
    ref, X, _ = case(257, 17)
    Xd = np.concatenate([X[:6], X[:3], X[2:4]])         # 11 shapes, 6 distinct
    dev = build(ctx, ref, Xd)
    assert dev.rank == 5 == pr.pca_model(ref, Xd).rank
    assert dev.pcaInfo.kept_variance <= dev.pcaInfo.total_variance
    compare(dev, pr.pca_model(ref, Xd), Xd, label="duplicates:")
    dev.device().close()
    dev = build(ctx, ref, X, maxRank=4)
    assert dev.rank == 4 and dev.pcaInfo.kept_variance < dev.pcaInfo.total_variance
    np.testing.assert_allclose(dev.variance, case(257, 17)[2].variance[:4], rtol=0, atol=TOL * dev.variance[0])
    dev.device().close()


def test_the_result_is_a_model(ctx):
    import gingr_amd as ga
    ref, X, m = case(257, 17)
    dev = build(ctx, ref, X)
    dm = dev.device()
    # what the restatement would upload, resident next to it: the same marginal covariance, and the diagonal blocks of Q0 Q0^T
    up = ga.DeviceModel(ctx, ga.PointDistributionModel(m.reference, m.mean, m.basis, m.variance))
    cov, cov_up = dm.marginalCovariance(), up.marginalCovariance()
    Q = m.Q0.reshape(-1, 3, m.rank)
    blocks = np.einsum("mdk,mek->mde", Q, Q)
    want = np.stack([blocks[:, 0, 0], blocks[:, 0, 1], blocks[:, 0, 2], blocks[:, 1, 1], blocks[:, 1, 2], blocks[:, 2, 2]], axis=1)
    top = np.abs(want).max()
    print(f"marginal covariance: against Q0 Q0^T {np.abs(cov - want).max() / top:.2e}, against the uploaded model {np.abs(cov - cov_up).max() / top:.2e}")
    assert np.abs(cov - want).max() <= TOL * top and np.abs(cov - cov_up).max() <= TOL * top
    # instance: reference + mean + Q0 alpha of what download returns
    alpha = np.random.default_rng(2).normal(size=dm.rank)
    host = dev.to_host()
    np.testing.assert_allclose(dm.instance(alpha), host.reference + host.mean + (q0_of(host) @ alpha).reshape(-1, 3), rtol=0, atol=1e-9)
    # truncate
    t = dev.truncate(3)
    assert t.rank == 3
    np.testing.assert_array_equal(t.variance, dev.variance[:3])
    np.testing.assert_array_equal(np.asarray(t.basis), np.asarray(dev.basis)[:, :3])
    t.device().close()
    up.close()
    # three CPD updates with it as prior
    target = dm.instance(0.5 * alpha) + np.random.default_rng(3).normal(0, 0.1, ref.shape)
    algo = ga.CpdRegistration(ctx)
    state = algo.createInitialState(dev, target, ga.CpdConfiguration(maxIterations=5, w=0.0))
    s0 = state.general.sigma2
    for _ in range(3):
        state = algo.update(state)
    assert state.general.status == 0 and np.isfinite(state.general.fit).all() and state.general.sigma2 < s0
    algo.close()
    dm.close()


def test_model_from_log_samples(ctx):
    import gingr_amd as ga
    from gingr_amd import helper, io as gio
    ref, X, m = case(257, 17)
    prior = ga.PointDistributionModel(m.reference, m.mean, m.basis, m.variance)
    rng = np.random.default_rng(11)
    log = [gio.JsonLogEntry(i, "x", {"product": 0.0}, True, [float(v) for v in rng.normal(size=m.rank)], [0.5 * i, 0.0, -1.0],
                            [0.01 * i, 0.02, -0.01], [1.0, 2.0, 3.0], 1.0, "") for i in range(9)]
    shapes = np.stack(helper.logSamples2shapes(ctx, prior, log))
    dev = helper.modelFromLog(ctx, prior, log, alignment="gpa")
    want = pr.pca_model(m.reference, shapes, 2)
    assert dev.pcaInfo.gpa_sweeps == want.aligned.sweeps
    compare(dev, want, shapes, label="from a log:")
    dev.device().close()


def test_errors_leave_the_context_usable(ctx):
    import ctypes
    import gingr_amd as ga
    from gingr_amd import _native as nat
    ref, X, m = case(37, 5)
    bad = X.copy()
    bad[2, 5, 1] = np.nan
    bad_ref = ref.copy()
    bad_ref[0, 0] = np.inf
    for args, code in [((ref, X[:1]), nat.ERR_BAD_ARGUMENT), ((ref, np.zeros((513, 37, 3))), nat.ERR_BAD_ARGUMENT),
                       ((ref, bad), nat.ERR_NONFINITE), ((bad_ref, X), nat.ERR_NONFINITE),
                       ((ref, np.stack([X[0]] * 3)), nat.ERR_BAD_ARGUMENT), ((ref, np.stack([X[0]] * 2)), nat.ERR_BAD_ARGUMENT),
                       # identical shapes at the upper limit: the rounding of a mean over 512 terms is still no variance
                       ((ref, np.stack([X[0]] * 512)), nat.ERR_BAD_ARGUMENT), ((ref, np.stack([X[1]] * 311)), nat.ERR_BAD_ARGUMENT)]:
        with pytest.raises(ga.GingrNativeError) as e:
            build(ctx, *args)
        assert e.value.code == code, str(e.value)
        assert "model_from_shapes" in str(e.value)
    with pytest.raises(ValueError):
        build(ctx, ref, X, "similarity")
    # straight through the ABI: alignment outside 0..2, M < 1
    lib, h, info = ctx._lib, ctypes.c_void_p(), nat.PcaInfo()
    r, x = nat.f64(ref), nat.f64(X)
    for M, n, mode in [(37, 5, 3), (37, 5, -1), (0, 5, 0)]:
        rc = lib.gingr_model_from_shapes(ctx.handle, M, n, nat.dptr(r), nat.dptr(x), mode, 3, 1e-5, 1e-10, 0, ctypes.byref(h), ctypes.byref(info))
        assert rc == nat.ERR_BAD_ARGUMENT and not h.value
        assert b"model_from_shapes" in lib.gingr_last_error(ctx.handle)
    dev = build(ctx, ref, X)
    compare(dev, m, X, label="after the errors:")
    dev.device().close()


@pytest.mark.parametrize("M,n,alignment", [(257, 17, "gpa"), (300, 193, "none")])
def test_two_builds_give_identical_bits(ctx, M, n, alignment):
    ref, X, _ = case(M, n, alignment, alignment != "none")
    a, b = build(ctx, ref, X, alignment), build(ctx, ref, X, alignment)
    ha, hb = a.to_host(), b.to_host()
    for f in ("reference", "mean", "variance", "basis"):
        assert np.array_equal(np.asarray(getattr(ha, f)), np.asarray(getattr(hb, f))), f
    assert a.pcaInfo == b.pcaInfo
    a.device().close()
    b.device().close()


def test_create_and_destroy_returns_device_memory(ctx):
    """Thirty builds with Procrustes at M = 100 000, n = 24 must not cost device memory.  Every device buffer of a build that scales
    with the input, left behind once per build, exceeds the bound: the three per-point buffers (target, mean, interleaved staging of
    the mean) 2.3 MiB each -- 69 MiB over the thirty builds --, the shapes and their staging buffer 55 MiB each, the raw model and
    the result 73 MiB each."""
    import torch

    def free_bytes():
        torch.cuda.synchronize(0)
        return torch.cuda.mem_get_info(0)[0]

    M, n, cycles, bound = 100_000, 24, 30, 64 << 20
    assert cycles * 3 * M * 8 > bound                   # (the smallest of the buffers above, leaked every cycle)
    ref, X = dataset(M, n)

    def cycle():
        dev = build(ctx, ref, X, "gpa")
        assert dev.rank == n - 1
        dev.device().close()

    cycle()
    gc.collect()
    before = free_bytes()
    for _ in range(cycles):
        cycle()
    gc.collect()
    after = free_bytes()
    assert before - after < bound, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
