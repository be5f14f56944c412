"""GPU tests of gingr_gpmm_build_radial -- radial terms (Gaussian, rational quadratic, inverse multiquadric) with an optional weight
field each -- against the plain-numpy restatement of the kernels (tests/varying_kernel_restatement.py) fed to the oracle's generic
pivoted Cholesky, which is scalismo's route.

Comparison: that of tests/test_gpu_gpmm.py (check_model_against_oracle, copied): equal rank, eigenvalues to 1e-9 relative, U^T U to
1e-9 of the identity, the sampled covariance U diag(lambda) U^T to 1e-9 of its largest entry.

Shapes: M = 300 points of a jittered surface patch (no exact ties).  On the scalar route that is two workgroups of 256 entries, the
second partial; on the generic route 900 entries in four workgroups.  Every build stops at a relative tolerance, and every case asserts
on the CPU that the restatement's residual trace stays at least 1e-6 (relative to the threshold) away from the threshold on both sides
of its stop, so that rounding cannot move the column count."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import varying_kernel_restatement as vk

pytestmark = pytest.mark.gpu
M = 300


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def cov_of(U, lam, rows):
    A = U[rows] * np.sqrt(lam)[None, :]
    return A @ A.T


def check_model_against_oracle(dm_host, mo, tol_lam=1e-9, tol_cov=1e-9):
    assert dm_host.variance.shape[0] == mo.rank
    print("eigenvalues rel", rel(dm_host.variance, mo.lam))
    assert rel(dm_host.variance, mo.lam) < tol_lam
    U = np.asarray(dm_host.basis)
    # unit, mutually orthogonal columns
    G = U.T @ U
    print("orthonormality", np.abs(G - np.eye(G.shape[0])).max())
    assert np.abs(G - np.eye(G.shape[0])).max() < 1e-9
    rows = np.random.default_rng(0).permutation(U.shape[0])[:300]
    Cd, Co = cov_of(U, dm_host.variance, rows), cov_of(mo.U, mo.lam, rows)
    print("covariance", np.abs(Cd - Co).max() / np.abs(Co).max())
    assert np.abs(Cd - Co).max() < tol_cov * np.abs(Co).max()


@functools.lru_cache(maxsize=None)
def patch():
    """a 20 x 15 patch of a wavy surface, 5 apart, every vertex jittered by up to 1.5 in the plane and 0.6 across it"""
    rng = np.random.default_rng(3)
    i, j = np.divmod(np.arange(M), 15)
    x, y = 5.0 * i, 5.0 * j
    P = np.stack([x, y, 8.0 * np.sin(x / 20.0) * np.cos(y / 25.0)], axis=1) + rng.uniform(-1.5, 1.5, (M, 3)) * np.array([1, 1, 0.4])
    P.setflags(write=False)
    return P


def amplitude():
    """a smooth amplitude field between 0.2 and 3"""
    P = patch()
    a = 0.2 + 2.8 * (0.5 + 0.5 * np.sin(P[:, 0] / 30.0) * np.cos(P[:, 1] / 40.0))
    assert a.min() >= 0.2 and a.max() <= 3.0 and a.max() - a.min() > 1.5
    return a


def indicator():
    return vk.sigmoid_field(patch(), [50.0, 35.0, 0.0], [1.0, 0.3, 0.0], 8.0)


PARS_A, PARS_B = [(40.0, 20.0)], [(12.0, 5.0)]            # (sigma, scaling): a stiff part and a small-scale part
PLAIN = [(vk.GAUSSIAN, 40.0, 20.0, None), (vk.GAUSSIAN, 12.0, 5.0, None)]


def restated_cases():
    a, s = amplitude(), indicator()
    zero = np.where(patch()[:, 0] < 14.0, 0.0, a)
    cp = vk.change_point_terms(PARS_A, PARS_B, s)
    return {
        "rq": ([(vk.RATIONAL_QUADRATIC, 30.0, 4.0, None)], 0.01),
        "imq": ([(vk.INVERSE_MULTIQUADRIC, 30.0, 50.0, None)], 0.01),
        "mix8": ([(vk.GAUSSIAN, 40.0, 10.0, None), (vk.RATIONAL_QUADRATIC, 25.0, 2.0, None), (vk.INVERSE_MULTIQUADRIC, 20.0, 30.0, None),
                  (vk.GAUSSIAN, 15.0, 3.0, None), (vk.RATIONAL_QUADRATIC, 60.0, 1.5, None), (vk.INVERSE_MULTIQUADRIC, 45.0, 20.0, None),
                  (vk.GAUSSIAN, 25.0, 6.0, None), (vk.RATIONAL_QUADRATIC, 12.0, 0.5, None)], 0.01),
        "scaled": ([(vk.GAUSSIAN, 25.0, 10.0, a)], 0.02),
        "change_point": (cp, 0.02),
        "change_point_x": ((cp, PLAIN, PLAIN), 0.05),
        "zero_region": ([(vk.GAUSSIAN, 25.0, 10.0, zero), (vk.RATIONAL_QUADRATIC, 30.0, 2.0, zero)], 0.02),
        "wide": ([(vk.GAUSSIAN, 6.0, 10.0, a)], 0.02),
    }


@functools.lru_cache(maxsize=None)
def restated(name):
    """(terms, tolerance, L) of a case, the factor computed once; its stop is checked to be safe from rounding"""
    terms, tol = restated_cases()[name]
    L = vk.factor(patch(), terms, tol)
    before, after = vk.stop_margin(patch(), terms, L, tol)
    print(name, "columns", L.shape[1], "margins", before, after)
    assert before >= 1e-6 and after >= 1e-6, (name, before, after)
    return terms, tol, L


def to_terms(ga, terms):
    """the restatement's term tuples as RadialKernelTerm (the same list for the three coordinates, or one list each)"""
    if isinstance(terms, tuple):
        made = {}
        return tuple(made.setdefault(id(t), to_terms(ga, t)) for t in terms)
    return [ga.RadialKernelTerm(f, p, sc, w) for f, p, sc, w in terms]


def build(ctx, terms, tol, **kw):
    import gingr_amd as ga
    return ga.GPMMTriangleMesh3D(ctx, patch(), relativeTolerance=tol, **kw).RadialMixture(to_terms(ga, terms))


def same_download(a, b):
    return (np.array_equal(a.reference, b.reference) and np.array_equal(a.mean, b.mean) and np.array_equal(a.variance, b.variance)
            and np.array_equal(np.asarray(a.basis), np.asarray(b.basis)))


# ---- 1. the two unported kernels of the reference, and all three families in one kernel of exactly eight terms ---------------------
@pytest.mark.parametrize("name", ["rq", "imq", "mix8"])
def test_rational_families_match_the_restatement(ctx, name):
    terms, tol, L = restated(name)
    assert len(terms) == (8 if name == "mix8" else 1)
    dm = build(ctx, terms, tol)
    assert dm.rank == L.shape[1] < 512, (dm.rank, L.shape[1])
    info = dm.buildInfo
    assert info.columns == L.shape[1] and info.tolerance_reached and info.residual_fraction < tol
    check_model_against_oracle(dm.to_host(), vk.model_of(patch(), L))


def test_named_builders_are_the_one_term_mixtures(ctx):
    import gingr_amd as ga
    g = ga.GPMMTriangleMesh3D(ctx, patch(), relativeTolerance=0.01)
    assert same_download(g.RationalQuadratic(30.0, 4.0).to_host(), build(ctx, restated("rq")[0], 0.01).to_host())
    assert same_download(g.InverseMultiquadric(30.0, 50.0).to_host(), build(ctx, restated("imq")[0], 0.01).to_host())


# ---- 2. one weighted Gaussian: a kernel scaled by a function of position, the scalar route ------------------------------------------
def test_scaled_gaussian_matches_the_restatement(ctx):
    import gingr_amd as ga
    terms, tol, L = restated("scaled")
    dm = ga.GPMMTriangleMesh3D(ctx, patch(), relativeTolerance=tol).ScaledGaussian([ga.GaussianKernelParameters(25.0, 10.0)], amplitude())
    assert dm.rank == L.shape[1]
    check_model_against_oracle(dm.to_host(), vk.model_of(patch(), L))


# ---- 3. change point: two terms weighted by a sigmoid and its complement -----------------------------------------------------------
def change_point_model(ctx, **kw):
    import gingr_amd as ga
    g = ga.GPMMTriangleMesh3D(ctx, patch(), relativeTolerance=restated_cases()["change_point"][1], **kw)
    s = ga.sigmoidField(patch(), [50.0, 35.0, 0.0], [1.0, 0.3, 0.0], 8.0)
    assert np.array_equal(s, indicator())
    return g.ChangePoint([ga.GaussianKernelParameters(*p) for p in PARS_A], [ga.GaussianKernelParameters(*p) for p in PARS_B], s)


def test_change_point_matches_the_restatement(ctx):
    terms, tol, L = restated("change_point")
    dm = change_point_model(ctx)
    assert dm.rank == L.shape[1]
    check_model_against_oracle(dm.to_host(), vk.model_of(patch(), L))


# ---- 4. the field on the x kernel only: coordinates that differ, the generic route over the 900 entries -----------------------------
def test_change_point_on_x_only_runs_the_generic_route(ctx):
    terms, tol, L = restated("change_point_x")
    dm = build(ctx, terms, tol)
    assert dm.rank == L.shape[1] < 512
    assert dm.rank % 3 != 0 or not np.array_equal(dm.variance[0::3], dm.variance[1::3])    # no x/y/z triplets: the coordinates differ
    check_model_against_oracle(dm.to_host(), vk.model_of(patch(), L))


# ---- 5. a region held fixed: weight zero in every term ------------------------------------------------------------------------------
def test_zero_weight_region_stays_on_the_reference(ctx):
    import gingr_amd as ga
    terms, tol, L = restated("zero_region")
    fixed = np.flatnonzero(terms[0][3] == 0.0)
    assert fixed.shape[0] >= 40 and np.array_equal(fixed, np.flatnonzero(terms[1][3] == 0.0))
    dm = build(ctx, terms, tol)
    assert dm.rank == L.shape[1]
    host = dm.to_host()
    check_model_against_oracle(host, vk.model_of(patch(), L))
    rows = (3 * fixed[:, None] + np.arange(3)[None, :]).reshape(-1)
    U = np.asarray(host.basis)
    assert np.all(U[rows] == 0.0)                                          # exact zeros, not small numbers
    moving = np.setdiff1d(np.arange(3 * M), rows)
    assert np.all(np.abs(U[moving]).max(axis=1) > 0.0)
    inst = np.asarray(dm.device().instance(np.random.default_rng(4).normal(0, 1, dm.rank))).reshape(-1, 3)
    assert np.array_equal(inst[fixed], patch()[fixed])
    assert np.abs(inst - patch()).max() > 0.1


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["scalar", "generic"])
def test_gaussian_terms_without_fields_are_the_old_entry_bit_for_bit(ctx, route):
    """gingr_gpmm_build_radial with Gaussian terms and no fields == gingr_gpmm_build_diagonal_ex with the same mixtures"""
    import gingr_amd as ga
    from gingr_amd.models import ScalarKernelSpec
    kx = ScalarKernelSpec("gauss", (40.0, 12.0), (20.0, 5.0))
    ky = kx if route == "scalar" else ScalarKernelSpec("gauss", (25.0,), (10.0,))
    old = ga.DevicePointDistributionModel(ctx, patch(), [], [], 0.02, 0, kernels=(kx, ky, ky), toTolerance=True)
    tx = [(vk.GAUSSIAN, 40.0, 20.0, None), (vk.GAUSSIAN, 12.0, 5.0, None)]
    ty = tx if route == "scalar" else [(vk.GAUSSIAN, 25.0, 10.0, None)]
    new = build(ctx, (tx, ty, ty), 0.02, toTolerance=True)
    assert old.buildInfo == new.buildInfo and old.rank == new.rank > 30
    a, b = old.to_host(), new.to_host()
    assert np.array_equal(a.variance, b.variance) and np.array_equal(np.asarray(a.basis), np.asarray(b.basis))
    if route == "generic":
        assert not np.array_equal(a.variance[0::3][:5], a.variance[1::3][:5])


@pytest.mark.parametrize("route", ["scalar", "generic"])
def test_fields_of_ones_are_no_fields_bit_for_bit(ctx, route):
    one = np.ones(M)
    tx = [(vk.GAUSSIAN, 30.0, 7.0, None), (vk.RATIONAL_QUADRATIC, 25.0, 2.0, None), (vk.INVERSE_MULTIQUADRIC, 20.0, 30.0, None)]
    ty = tx if route == "scalar" else [(vk.GAUSSIAN, 25.0, 10.0, None)]
    with_ones = lambda terms: [(f, p, sc, one) for f, p, sc, _ in terms]
    a = build(ctx, (tx, ty, ty), 0.03)
    b = build(ctx, (with_ones(tx), with_ones(ty), with_ones(ty)), 0.03)
    assert a.rank == b.rank > 10 and same_download(a.to_host(), b.to_host())


def test_two_builds_of_the_change_point_model_are_equal(ctx):
    a, b = change_point_model(ctx), change_point_model(ctx)
    assert same_download(a.to_host(), b.to_host())


# ---- 7. row shards ------------------------------------------------------------------------------------------------------------------
def test_row_shards_of_a_weighted_model_hold_the_rows_of_the_full_model(ctx):
    import gingr_amd as ga
    dm = change_point_model(ctx)
    full = dm.to_host()
    for b, e in [(0, 130), (130, 300)]:
        shard = ga.DeviceModel(ctx, dm, b, e)
        h = shard.download()
        assert shard.rank == dm.rank
        assert np.array_equal(h.reference, patch()[b:e])
        assert np.array_equal(h.variance, full.variance)
        assert np.array_equal(np.asarray(h.basis), np.asarray(full.basis)[3 * b:3 * e])
        shard.close()


# ---- 8. to tolerance past 512 factor columns, truncation folded into the build --------------------------------------------------------
def test_weighted_model_to_tolerance_past_512_columns_with_keep_rank(ctx):
    """keep_rank = 100 cuts through an x/y/z triplet of equal eigenvalues, inside which the eigenvectors are only defined up to a
    rotation (tests/test_gpu_gpmm_to_tolerance.py): eigenvalues and orthonormality are compared for all 100, the covariance for the
    99 leading columns, where the cut falls into a gap of the spectrum."""
    import gingr_amd as ga
    terms, tol, L = restated("wide")
    columns = L.shape[1]
    assert 513 <= columns <= 900
    mo = vk.model_of(patch(), L)
    with pytest.raises(ga.GingrNativeError) as e:                          # never a silently shorter model
        build(ctx, terms, tol, toTolerance=True).device()
    assert e.value.code == ga._native.ERR_BAD_ARGUMENT and str(columns) in str(e.value) and "keep_rank" in str(e.value)
    dm = build(ctx, terms, tol, toTolerance=True).truncate(100)
    info = dm.buildInfo
    print(info)
    assert info.columns == columns and info.rank == 100 and dm.rank == 100 and info.tolerance_reached
    assert info.residual_fraction < tol
    assert abs(info.kept_variance_fraction - mo.lam[:100].sum() / mo.lam.sum()) < 1e-9
    host = dm.to_host()
    lam, U = np.asarray(host.variance), np.asarray(host.basis)
    assert lam.shape[0] == 100 and rel(lam, mo.lam[:100]) < 1e-9
    assert np.abs(U.T @ U - np.eye(100)).max() < 1e-9
    assert mo.lam[98] - mo.lam[99] > 1e-6 * mo.lam[0]                      # a gap after 99 columns
    rows = np.random.default_rng(0).permutation(U.shape[0])[:300]
    Cd, Co = cov_of(U[:, :99], lam[:99], rows), cov_of(mo.U[:, :99], mo.lam[:99], rows)
    print("covariance", np.abs(Cd - Co).max() / np.abs(Co).max())
    assert np.abs(Cd - Co).max() < 1e-9 * np.abs(Co).max()


# ---- 9. argument errors -------------------------------------------------------------------------------------------------------------
def native_kernel(nat, terms, keep):
    arr = (nat.RadialTerm * max(len(terms), 1))()
    for i, (family, parameter, scaling, w) in enumerate(terms):
        arr[i].family, arr[i].parameter, arr[i].scaling = family, parameter, scaling
        if w is not None:
            keep.append(w)
            arr[i].weight = nat.dptr(w)
    k = nat.RadialKernel()
    k.n_terms, k.terms = len(terms), arr
    keep.append(arr)
    return k


def test_argument_errors_leave_no_model_and_a_usable_context(ctx):
    from gingr_amd import _native as nat
    P = np.ascontiguousarray(patch())
    ok = (nat.RADIAL_GAUSSIAN, 30.0, 5.0, None)
    bad_w, zero_w = np.ones(M), np.zeros(M)
    bad_w[77] = np.inf
    nan_w = np.where(np.arange(M) == 5, np.nan, 1.0)
    cases = [([], "n_terms"), ([ok] * 9, "n_terms"),
             ([ok, (3, 30.0, 5.0, None)], "term 1"), ([(-1, 30.0, 5.0, None)], "term 0"),
             ([ok, ok, (nat.RADIAL_RATIONAL_QUADRATIC, 0.0, 5.0, None)], "term 2"), ([(nat.RADIAL_GAUSSIAN, -3.0, 5.0, None)], "term 0"),
             ([(nat.RADIAL_INVERSE_MULTIQUADRIC, np.nan, 5.0, None)], "term 0"), ([(nat.RADIAL_GAUSSIAN, np.inf, 5.0, None)], "term 0"),
             ([ok, (nat.RADIAL_GAUSSIAN, 30.0, 0.0, None)], "term 1"), ([(nat.RADIAL_GAUSSIAN, 30.0, -1.0, None)], "term 0"),
             ([(nat.RADIAL_GAUSSIAN, 30.0, np.inf, None)], "term 0"), ([(nat.RADIAL_GAUSSIAN, 30.0, np.nan, None)], "term 0"),
             ([ok, (nat.RADIAL_GAUSSIAN, 30.0, 5.0, bad_w)], "term 1"), ([(nat.RADIAL_RATIONAL_QUADRATIC, 30.0, 5.0, nan_w)], "term 0"),
             ([(nat.RADIAL_GAUSSIAN, 30.0, 5.0, zero_w), (nat.RADIAL_INVERSE_MULTIQUADRIC, 30.0, 5.0, zero_w)], "diagonal is zero")]
    keep = []
    good = native_kernel(nat, [ok], keep)
    for terms, names in cases:
        for slot in range(3):                                             # the bad kernel on x, on y, on z
            ks = [good, good, good]
            ks[slot] = native_kernel(nat, terms, keep)
            info, h = nat.GpmmInfo(), ctypes.c_void_p(1)
            rc = ctx._lib.gingr_gpmm_build_radial(ctx.handle, M, nat.dptr(P), ctypes.byref(ks[0]), ctypes.byref(ks[1]), ctypes.byref(ks[2]),
                                                  0.05, 0, 0, 0, 0, ctypes.byref(info), ctypes.byref(h))
            text = (ctx._lib.gingr_last_error(ctx.handle) or b"").decode()
            assert rc == nat.ERR_BAD_ARGUMENT and not h.value, (terms, rc)
            assert names in text and f"kernel {'xyz'[slot]}" in text, text
    # the entry's shared checks: tolerance, columns above the ceiling
    for tol, max_columns in [(1.0, 0), (float("nan"), 0), (0.05, nat.GPMM_MAX_COLUMNS + 1)]:
        h = ctypes.c_void_p(1)
        rc = ctx._lib.gingr_gpmm_build_radial(ctx.handle, M, nat.dptr(P), ctypes.byref(good), ctypes.byref(good), ctypes.byref(good), tol,
                                              max_columns, 0, 0, 0, None, ctypes.byref(h))
        assert rc == nat.ERR_BAD_ARGUMENT and not h.value
    # the context still builds
    h = ctypes.c_void_p()
    rc = ctx._lib.gingr_gpmm_build_radial(ctx.handle, M, nat.dptr(P), ctypes.byref(good), ctypes.byref(good), ctypes.byref(good), 0.05, 0, 0,
                                          0, 0, None, ctypes.byref(h))
    assert rc == nat.GINGR_OK and h.value
    ctx._lib.gingr_model_destroy(h)


# ---- 10. end to end -------------------------------------------------------------------------------------------------------------------
def test_point_cloud_icp_with_the_change_point_model(ctx):
    """ten ICP updates with the device-built change-point model == go.icp_update on the restated model; the bounds of
    test_registration_with_a_device_built_model (fit 1e-5 relative, sigma2 1e-6)"""
    import gingr_amd as ga
    terms, tol, L = restated("change_point")
    mo = vk.model_of(patch(), L)
    rng = np.random.default_rng(21)
    target = mo.instance(rng.normal(0, 0.7, mo.rank)) @ go.euler_to_rot(0.02, -0.03, 0.025).T + np.array([0.8, -0.6, 0.4])
    dm = change_point_model(ctx)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=10, initialSigma=4.0, endSigma=1.0, correspondenceMethod="PointcloudClosestPoint")
    s_dev = algo.createInitialState(dm, target, cfg)
    st = go.initial_state(mo, s_dev.general.sigma2)
    for it in range(10):
        s_dev = algo.update(s_dev)
        st = go.icp_update(mo, target, st, 4.0, 1.0, 10)[0]
        assert s_dev.general.status == st.status == 0
    print("fit rel", rel(s_dev.general.fit, st.fit), "sigma2", s_dev.general.sigma2, st.sigma2)
    assert rel(s_dev.general.fit, st.fit) < 1e-5, rel(s_dev.general.fit, st.fit)
    assert abs(s_dev.general.sigma2 - st.sigma2) < 1e-6 * st.sigma2
    assert np.abs(s_dev.general.fit - patch()).max() > 0.3                  # the model moved
    algo.close()
