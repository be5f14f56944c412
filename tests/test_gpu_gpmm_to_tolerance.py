"""GPU tests of the to-tolerance GPMM build (gingr_gpmm_build_diagonal_ex: a factor of up to 1 536 columns, truncation folded into
the build, no silent shortening) and of gingr_model_truncate, against the oracle's restatement of scalismo's route.

Eigenvectors are defined up to sign and, inside an x/y/z triplet of equal eigenvalues, up to a rotation: comparisons are on
eigenvalues and on U diag(lambda) U^T, and a truncated covariance is only compared where the cut falls into a gap of the spectrum
(k = 99, 300, 510 below; k = 100 splits a triplet).  Tolerances: those of tests/test_gpu_gpmm.py for a device-built model against
the oracle (eigenvalues rel < 1e-9, sampled covariance < 1e-9 max, orthonormality 1e-9) and for one model taken two ways through
the update path (fit rel < 1e-12, sigma2 equal)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import gingr_oracle as go

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def cov_of(U, lam, rows):
    A = U[rows] * np.sqrt(lam)[None, :]
    return A @ A.T


def femur_points():
    return np.load(os.path.join(HERE, "golden", "inputs.npz"))["femur"].astype(np.float64)


def femur_target():
    return np.load(os.path.join(HERE, "golden", "inputs.npz"))["femur_target"].astype(np.float64)


def cloud():
    return np.random.default_rng(21).normal(0, 40, (1200, 3))


@functools.lru_cache(maxsize=None)
def femur_oracle():
    f = femur_points()
    return go.build_gpmm_mixture(f, *go.automatic_template_parameters(f), 0.01)


@functools.lru_cache(maxsize=None)
def cloud_oracle(max_columns):
    return go.build_gpmm_mixture(cloud(), [18.0], [10.0], 0.0, max_columns)


def check_truncated_against_oracle(host, mo, k, covariance=True):
    lam = np.asarray(host.variance)
    assert lam.shape[0] == k
    print("eigenvalues rel", rel(lam, mo.lam[:k]))
    assert rel(lam, mo.lam[:k]) < 1e-9
    U = np.asarray(host.basis)
    G = U.T @ U
    print("orthonormality", np.abs(G - np.eye(k)).max())
    assert np.abs(G - np.eye(k)).max() < 1e-9
    if covariance:
        rows = np.random.default_rng(0).permutation(U.shape[0])[:300]
        Cd, Co = cov_of(U, lam, rows), cov_of(mo.U[:, :k], mo.lam[:k], rows)
        print("covariance", np.abs(Cd - Co).max() / np.abs(Co).max())
        assert np.abs(Cd - Co).max() < 1e-9 * np.abs(Co).max()


def same_download(a, b):
    return (np.array_equal(a.reference, b.reference) and np.array_equal(a.mean, b.mean) and np.array_equal(a.variance, b.variance)
            and np.array_equal(np.asarray(a.basis), np.asarray(b.basis)))


# ---- 1. femur, template kernels, tolerance 0.01: 1 358 factor columns ------------------------------------------------------------
@pytest.mark.parametrize("k", [99, 300, 510, 100])
def test_femur_template_model_to_tolerance_then_truncate(ctx, k):
    import gingr_amd as ga
    mo = femur_oracle()
    assert mo.rank == 1358
    dm = ga.automaticGPMMfromTemplate(ctx, femur_points(), 0.01, toTolerance=True).truncate(k)
    info = dm.buildInfo
    print(info)
    assert info.columns == 1358 and info.tolerance_reached and info.rank == k and dm.rank == k
    assert info.residual_fraction < 0.01
    assert abs(info.kept_variance_fraction - mo.lam[:k].sum() / mo.lam.sum()) < 1e-9
    check_truncated_against_oracle(dm.to_host(), mo, k, covariance=(k != 100))   # k = 100 cuts through a triplet


# ---- 2. the block eigen kernel at every size class (blocks of 200, 300, 453, 512 columns) -----------------------------------------
@pytest.mark.parametrize("max_columns", [600, 900, 1359, 1536])
def test_block_eigen_kernel_size_classes(ctx, max_columns):
    import gingr_amd as ga
    mo = cloud_oracle(max_columns)
    assert mo.rank == max_columns
    for k in (99, 300, 510):
        dm = ga.DevicePointDistributionModel(ctx, cloud(), [18.0], [10.0], 0.0, maxRank=max_columns, toTolerance=True, keepRank=k)
        info = dm.buildInfo
        print(max_columns, k, info)
        assert info.columns == max_columns and not info.tolerance_reached and info.rank == k and dm.rank == k
        check_truncated_against_oracle(dm.to_host(), mo, k)
        dm.device().close()


# ---- 3. no silent shortening ----------------------------------------------------------------------------------------------------
def test_more_than_512_columns_without_keep_rank_is_an_error(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    f = femur_points()
    dm = ga.automaticGPMMfromTemplate(ctx, f, 0.01, toTolerance=True)
    with pytest.raises(ga.GingrNativeError) as e:
        dm.device()
    assert e.value.code == nat.ERR_BAD_ARGUMENT and "1358" in str(e.value) and "keep_rank" in str(e.value)
    # the C ABI call itself: *out stays NULL, info says how many columns there are
    sig, sc = go.automatic_template_parameters(f)
    sig, sc = nat.f64(sig), nat.f64(sc)
    k = nat.ScalarKernel()
    k.kind, k.n_kernels, k.sigmas, k.scalings = nat.KERNEL_GAUSSIAN_MIXTURE, 3, nat.dptr(sig), nat.dptr(sc)
    info, h = nat.GpmmInfo(), ctypes.c_void_p()
    rc = ctx._lib.gingr_gpmm_build_diagonal_ex(ctx.handle, f.shape[0], nat.dptr(f), ctypes.byref(k), ctypes.byref(k), ctypes.byref(k), 0.01,
                                               0, 0, 0, 0, ctypes.byref(info), ctypes.byref(h))
    assert rc == nat.ERR_BAD_ARGUMENT and not h.value
    assert info.columns == 1358 and info.tolerance_reached == 1 and info.rank == 1358


def test_ceiling_bad_argument_and_different_kernels(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    ref = cloud()
    with pytest.raises(ga.GingrNativeError) as e:      # tolerance 0 cannot be met by 1 536 columns of 3 600
        ga.DevicePointDistributionModel(ctx, ref, [18.0], [10.0], 0.0, toTolerance=True).device()
    assert e.value.code == nat.ERR_BAD_ARGUMENT and "1536" in str(e.value) and "residual" in str(e.value)
    with pytest.raises(ga.GingrNativeError) as e:
        ga.DevicePointDistributionModel(ctx, ref, [18.0], [10.0], 0.0, maxRank=1537, toTolerance=True).device()
    assert e.value.code == nat.ERR_BAD_ARGUMENT
    for max_columns in (600, 0):
        with pytest.raises(ga.GingrNativeError) as e:  # GaussianSymmetry: the generic route stays within 512 factor columns
            ga.GPMMTriangleMesh3D(ctx, ref, 0.0, maxRank=max_columns, toTolerance=True).GaussianSymmetry(18.0, 10.0).device()
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "coordinate-wise different kernels" in str(e.value)


# ---- 4. nothing reachable before changes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_columns", [30, 31, 192, 300, 512])
def test_new_entry_is_bit_identical_where_the_old_one_reaches(ctx, max_columns):
    import gingr_amd as ga
    ref = cloud()
    old = ga.GPMMTriangleMesh3D(ctx, ref, 0.0, maxRank=max_columns).Gaussian(18.0, 10.0)
    new = ga.GPMMTriangleMesh3D(ctx, ref, 0.0, maxRank=max_columns, toTolerance=True).Gaussian(18.0, 10.0)
    assert new.buildInfo.columns == max_columns == new.rank == old.rank
    assert new.buildInfo.kept_variance_fraction == 1.0
    assert same_download(old.to_host(), new.to_host())


def test_new_entry_is_bit_identical_for_different_kernels(ctx):
    import gingr_amd as ga
    ref = cloud()
    old = ga.GPMMTriangleMesh3D(ctx, ref, 0.0, maxRank=301).GaussianSymmetry(18.0, 10.0)
    new = ga.GPMMTriangleMesh3D(ctx, ref, 0.0, maxRank=301, toTolerance=True).GaussianSymmetry(18.0, 10.0)
    assert new.buildInfo.columns == 301 == old.rank
    assert same_download(old.to_host(), new.to_host())


# ---- 5. gingr_model_truncate ---------------------------------------------------------------------------------------------------
def sliced(host, k):
    import gingr_amd as ga
    return ga.PointDistributionModel(host.reference, host.mean, np.asarray(host.basis)[:, :k], host.variance[:k])


@pytest.mark.parametrize("rank,k", [(300, 99), (130, 112), (130, 100), (512, 256), (130, 130)])
def test_model_truncate_of_built_and_uploaded_models(ctx, rank, k):
    import gingr_amd as ga
    built = ga.GPMMTriangleMesh3D(ctx, cloud(), 0.0, maxRank=rank).Gaussian(18.0, 10.0)
    host = built.to_host()
    assert built.rank == rank
    t = built.truncate(k)                         # resident: gingr_model_truncate
    assert isinstance(t, ga.TruncatedDevicePointDistributionModel) and t.rank == k
    assert same_download(t.to_host(), sliced(host, k))
    up = ga.DeviceModel(ctx, ga.PointDistributionModel(host.reference, host.mean, host.basis, host.variance))
    tu = up.truncate(k)
    assert tu.rank == k
    # (an uploaded basis is scaled by sqrt(variance) on the way in and divided on the way out: the truncated model holds the same
    # device columns as its source, so its download equals the source's download)
    assert same_download(tu.download(), sliced(up.download(), k))
    tu.close()
    up.close()


def test_model_truncate_bounds(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    built = ga.GPMMTriangleMesh3D(ctx, cloud(), 0.0, maxRank=40).Gaussian(18.0, 10.0)
    dev = built.device()
    for k in (0, 41):
        h = ctypes.c_void_p()
        rc = ctx._lib.gingr_model_truncate(ctx.handle, dev.handle, k, ctypes.byref(h))
        assert rc == nat.ERR_BAD_ARGUMENT and not h.value
    with pytest.raises(ValueError):
        built.truncate(0)
    with pytest.raises(ValueError):
        built.truncate(41)


def test_truncated_model_through_the_update_path(ctx):
    """Five CPD updates on the femur pair: the model truncated in HBM against the host model truncated with numpy and uploaded."""
    import gingr_amd as ga
    ref, tgt = femur_points(), femur_target()
    built = ga.GPMMTriangleMesh3D(ctx, ref, 0.01).Gaussian(70.0, 50.0)
    host = built.to_host()
    k = min(60, built.rank - 1)

    def run(model):
        algo = ga.CpdRegistration(ctx)
        st = algo.createInitialState(model, tgt, ga.CpdConfiguration(maxIterations=10, w=0.1))
        for _ in range(5):
            st = algo.update(st)
        algo.close()
        return st.general

    a = run(built.truncate(k))
    b = run(ga.PointDistributionModel(host.reference, host.mean, host.basis, host.variance).truncate(k))
    print("fit rel", rel(a.fit, b.fit), a.sigma2, b.sigma2)
    assert a.status == 0 and b.status == 0
    assert rel(a.fit, b.fit) < 1e-12 and a.sigma2 == b.sigma2


# ---- 6. build-time and later truncation agree ----------------------------------------------------------------------------------
def test_build_time_and_later_truncation_agree(ctx):
    import gingr_amd as ga
    ref = cloud()
    folded = ga.DevicePointDistributionModel(ctx, ref, [18.0], [10.0], 0.0, maxRank=300, toTolerance=True, keepRank=99)
    full = ga.DevicePointDistributionModel(ctx, ref, [18.0], [10.0], 0.0, maxRank=300, toTolerance=True)
    full.device()
    later = full.truncate(99)
    a, b = folded.to_host(), later.to_host()
    assert folded.buildInfo.columns == 300 and folded.rank == 99 == later.rank
    assert np.array_equal(a.variance, b.variance)
    rows = np.random.default_rng(0).permutation(3 * ref.shape[0])[:300]
    Ca, Cb = cov_of(np.asarray(a.basis), a.variance, rows), cov_of(np.asarray(b.basis), b.variance, rows)
    assert np.abs(Ca - Cb).max() < 1e-9 * np.abs(Cb).max()


# ---- 7. row shards ----------------------------------------------------------------------------------------------------------------
def test_row_shards_of_the_new_entry(ctx):
    import gingr_amd as ga
    ref = cloud()
    M = ref.shape[0]
    dm = ga.DevicePointDistributionModel(ctx, ref, [18.0], [10.0], 0.0, maxRank=600, toTolerance=True, keepRank=99)
    whole = dm.to_host()
    assert dm.buildInfo.columns == 600 and dm.rank == 99
    U = np.asarray(whole.basis)
    for rb, re in ((0, M // 2), (M // 2, M)):
        shard = ga.DeviceModel(ctx, dm, rb, re)
        h = shard.download()
        assert np.array_equal(h.reference, whole.reference[rb:re]) and np.array_equal(h.mean, whole.mean[rb:re])
        assert np.array_equal(h.variance, whole.variance)
        assert np.array_equal(np.asarray(h.basis), U[3 * rb:3 * re])
        shard.close()
