"""GPU tests of the per-vertex covariance maps (gingr_amd/csrc/posterior_cov.hip): the kernel alone for arbitrary right factors,
and the posterior of a registration state against the oracle's restatement of scalismo's posterior model.

Error measure, per vertex: largest absolute entry difference of the 3 x 3 block / largest absolute expected entry of that block.
Tolerance, per case: 1000 x the same measure between two CPU routes to the expected blocks (the spread), and the spread itself
must stay below 1e-13 -- a condition on the inputs -- so that no case is ever judged looser than 1e-10.
  posterior cases: route A = the oracle (go.PDM.transform + posterior_model, pinv / SVD), route B = numpy Cholesky, L^-1 Q0^T.
  kernel-alone cases: route A = (Q W)(Q W)^T, route B = Q (W W^T) Q^T -- equal in exact arithmetic, summed in another order.
The factor 1000 covers the device's summation order, its blocked Cholesky and the explicit L^-T.

Largest device error seen per case on an MI355X (spread in brackets) -- see the table in DESIGN.md, section "per-vertex covariance maps".
"""
import functools

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests.test_gpu_surface_icp import femur, make_state, oracle_state_of

pytestmark = pytest.mark.gpu

POSE = ((0.3, -0.2, 0.1), (1.0, -2.0, 0.5))


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def model_of(M, r):
    """ref ~ N(0, 30^2); small ranks: the Gaussian GPMM of the oracle; r > 64: QR-orthonormal random U, lam = 400 * 0.97^k.
    (A single point carries at most three basis functions: max_rank = 5 gives rank 3 at M = 1.)"""
    rng = np.random.default_rng(1000 * r + M)
    ref = rng.normal(0, 30, (M, 3))
    if r <= 64:
        return go.build_gaussian_gpmm(ref, 40, 20, rel_tol=1e-9, max_rank=r)
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    return go.PDM(ref=ref, mean=np.zeros_like(ref), U=np.ascontiguousarray(U), lam=400.0 * 0.97 ** np.arange(r))


def ga_model(mo, cells=None):
    import gingr_amd as ga
    return ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells)


def Q3(mo):
    return (mo.U * np.sqrt(mo.lam)[None, :]).reshape(mo.M, 3, mo.rank)


def block_error(got, want):
    """largest per-vertex |difference|_max / |expected block|_max"""
    got, want = np.asarray(got).reshape(-1, 9), np.asarray(want).reshape(-1, 9)
    return float((np.abs(got - want).max(1) / np.abs(want).max(1)).max())


def mats(cov6):
    from gingr_amd.helper import covariance6_to_matrices
    return covariance6_to_matrices(cov6)


def check(name, got, route_a, route_b):
    spread = block_error(route_b, route_a)
    err = block_error(got, route_a)
    print(f"{name}: device error {err:.3e}, CPU spread {spread:.3e}, allowed {1000 * spread:.3e}")
    assert spread <= 1e-13, (name, spread)
    assert err <= 1000 * spread, (name, err, spread)


def assert_psd_blocks(cov6):
    c = np.asarray(cov6)
    xx, xy, xz, yy, yz, zz = c.T
    assert (xx >= 0).all() and (yy >= 0).all() and (zz >= 0).all()
    eps = 64 * np.finfo(float).eps                       # rounding of the products of two sums of squares
    assert (xx * yy - xy * xy >= -eps * xx * yy).all()
    assert (xx * zz - xz * xz >= -eps * xx * zz).all()
    assert (yy * zz - yz * yz >= -eps * yy * zz).all()


# ---------------------------------------------------------------------------------------------------------------- kernel alone
KERNEL_SHAPES = [(1, 5), (17, 5), (400, 24), (257, 100), (211, 130), (200, 512)]


def factor_routes(mo, W, R=None, pid=None):
    """the two CPU routes to R (Q_i W)(Q_p W)^T R^T (p = i without pid)"""
    Q = Q3(mo)
    if R is not None:
        Q = np.einsum("ab,mbk->mak", R, Q)
    Y = Q @ W
    QS = Q @ (W @ W.T)
    if pid is None:
        return np.einsum("mdk,mek->mde", Y, Y), np.einsum("mdk,mek->mde", QS, Q)
    return np.einsum("mdk,ek->mde", Y, Y[pid]), np.einsum("mdk,ek->mde", QS, Q[pid])


def check_cross(name, cross, marginal, marg_a, ca, cb, row):
    """cross-covariance blocks against the two CPU routes; per-vertex scale: the geometric mean of the two marginals that bound
    the block (a cross block may vanish, its bound does not).  The block at the point itself (local row `row`) is its marginal."""
    scale = np.sqrt(np.abs(marg_a).max((1, 2)) * np.abs(marginal[row]).max())
    spread = float((np.abs(cb - ca).max((1, 2)) / scale).max())
    err = float((np.abs(cross - ca).max((1, 2)) / scale).max())
    print(f"{name}: device error {err:.3e}, CPU spread {spread:.3e}, allowed {1000 * spread:.3e}")
    assert spread <= 1e-13, (name, spread)
    assert err <= 1000 * spread, (name, err, spread)
    assert block_error(cross[row], marginal[row]) <= 1000 * spread, name


@pytest.mark.parametrize("M,r", KERNEL_SHAPES)
def test_marginal_and_cross_covariance_of_a_dense_factor(ctx, M, r):
    import gingr_amd as ga
    mo = model_of(M, r)
    W = np.random.default_rng(r + M).normal(0, 1, (mo.rank, mo.rank))
    dm = ga.DeviceModel(ctx, ga_model(mo))
    try:
        got = dm.marginalCovariance(W)
        a, b = factor_routes(mo, W)
        check(f"marginal M={M} r={r}", mats(got), a, b)
        assert_psd_blocks(got)
        for pid in sorted({0, M - 1}):
            cross = dm.crossCovariance(pid, W)
            ca, cb = factor_routes(mo, W, pid=pid)
            check_cross(f"cross M={M} r={r} pid={pid}", cross, mats(got), a, ca, cb, pid)
    finally:
        dm.close()


def test_prior_marginal_and_rotation_at_the_first_wide_rank(ctx):
    import gingr_amd as ga
    mo = model_of(211, 130)
    dm = ga.DeviceModel(ctx, ga_model(mo))
    try:
        I = np.eye(mo.rank)
        a, b = factor_routes(mo, I)
        prior = np.einsum("mdk,k,mek->mde", mo.U.reshape(mo.M, 3, -1), mo.lam, mo.U.reshape(mo.M, 3, -1))   # U_i diag(lam) U_i^T
        got = dm.marginalCovariance()
        check("prior marginal", mats(got), prior, a)
        assert_psd_blocks(got)
        W = np.random.default_rng(5).normal(0, 1, (mo.rank, mo.rank))
        euler = (0.3, -0.2, 0.1)
        ra, rb = factor_routes(mo, W, R=go.euler_to_rot(*euler))
        got = dm.marginalCovariance(W, euler=euler)
        check("rotated marginal", mats(got), ra, rb)
        cross = dm.crossCovariance(17, W, euler=euler)
        ca, cb = factor_routes(mo, W, R=go.euler_to_rot(*euler), pid=17)
        check_cross("rotated cross pid=17", cross, mats(got), ra, ca, cb, 17)
    finally:
        dm.close()


def test_row_shard_covers_its_local_rows(ctx):
    import gingr_amd as ga
    mo = model_of(211, 130)
    W = np.random.default_rng(6).normal(0, 1, (mo.rank, mo.rank))
    a, b = factor_routes(mo, W)
    dm = ga.DeviceModel(ctx, ga_model(mo), 5, 150)
    try:
        got = dm.marginalCovariance(W)
        assert got.shape == (145, 6)
        check("row shard [5, 150)", mats(got), a[5:150], b[5:150])
        cross = dm.crossCovariance(149, W)
        ca, cb = factor_routes(mo, W, pid=149)
        check_cross("row shard cross pid=149", cross, mats(got), a[5:150], ca[5:150], cb[5:150], 144)
        with pytest.raises(ga.GingrNativeError) as e:
            dm.crossCovariance(0, W)                       # a point of another shard
        assert e.value.code == 6                            # GINGR_ERR_STATE
    finally:
        dm.close()


# ---------------------------------------------------------------------------------------------------------------- posterior of a state
def posterior_routes(mo, st, pids, pts, covs):
    """(oracle blocks, Cholesky-route blocks) of the posterior of model.transform(rigid of st) given the observations"""
    posed = mo.transform(st.rotation(), st.translation, st.center)
    post = posed.posterior_model(pids, pts, covs)
    U3 = post.U.reshape(mo.M, 3, -1)
    route_a = np.einsum("mdk,k,mek->mde", U3, post.lam, U3)
    Q = posed.U * np.sqrt(posed.lam)[None, :]
    G = np.zeros((mo.rank, mo.rank))
    for k, pid in enumerate(np.asarray(pids)):
        Qk = Q[3 * pid:3 * pid + 3]
        G += Qk.T @ np.linalg.solve(covs[k], Qk)
    L = np.linalg.cholesky(np.eye(mo.rank) + G)
    Y = np.linalg.solve(L, Q.T).T.reshape(mo.M, 3, -1)             # rows of Q L^-T
    return route_a, np.einsum("mdk,mek->mde", Y, Y)


def synthetic_target(mo, seed, n=None):
    rng = np.random.default_rng(seed)
    t = mo.instance(rng.normal(0, 0.7, mo.rank)) @ go.euler_to_rot(0.25, -0.15, 0.12).T + np.array([1.5, -1.0, 0.8])
    n = mo.M - mo.M // 10 if n is None else n
    return t[rng.permutation(mo.M)[:max(n, 1)]] + rng.normal(0, 0.3, (max(n, 1), 3))


def three_landmarks(mo, target):
    rng = np.random.default_rng(77)
    pids = np.array([3, mo.M // 2, mo.M - 2], dtype=np.int64)
    pts = target[:3] + rng.normal(0, 1.0, (3, 3))
    covs = []
    for _ in range(3):
        A = rng.normal(0, 1, (3, 3))
        covs.append(A @ A.T + np.diag([0.2, 1.0, 3.0]))          # anisotropic, well conditioned
    return go.Landmarks(pids=pids, points=pts, covs=np.array(covs))


# name -> (algorithm, M, r, sigma2 (None: the CPD initial value), posed, landmarks)
STATE_CASES = {
    "cpd-400x24-initial-landmarks": ("cpd", 400, 24, None, False, True),
    "cpd-400x24-s1-posed": ("cpd", 400, 24, 1.0, True, False),
    "cpd-257x100-s4": ("cpd", 257, 100, 4.0, False, False),
    "cpd-211x130-s4": ("cpd", 211, 130, 4.0, False, False),
    "icp-403x24-s1-posed": ("icp", 403, 24, 1.0, True, False),
    "icp-200x512-s1": ("icp", 200, 512, 1.0, False, False),
    "icp-200x512-s0.01": ("icp", 200, 512, 0.01, False, False),
}


def state_case(ctx, name):
    """(algo, state, oracle model, oracle observations) of a case; the oracle sees the fit the device state holds"""
    import gingr_amd as ga
    kind, M, r, s2, posed, with_lm = STATE_CASES[name]
    mo = model_of(M, r)
    target = synthetic_target(mo, seed=M + r)
    lm_o = three_landmarks(mo, target) if with_lm else None
    lm = ga.LandmarkCorrespondences(lm_o.pids.astype(np.int32), lm_o.points, lm_o.covs) if with_lm else None
    pose = POSE if posed else None
    if kind == "cpd":
        algo = ga.CpdRegistration(ctx)
        cfg = ga.CpdConfiguration(maxIterations=50, w=0.1, initialSigma=s2)
    else:
        algo = ga.IcpRegistration(ctx)
        cfg = ga.IcpConfiguration(maxIterations=50, initialSigma=s2, endSigma=min(1.0, s2), correspondenceMethod="PointcloudClosestPoint")
    state = algo.createInitialState(ga_model(mo), target, cfg, landmarks=lm, initial_pose=pose)
    st = oracle_state_of(state.general, 1)
    if kind == "cpd":
        pids, pts, var = go.cpd_observations(mo, target, st, w=0.1)
    else:
        idx, _, _ = go.icp_closest_point(st.fit, target)
        pids, pts, var = np.arange(mo.M), target[idx], np.full(mo.M, st.sigma2)
    return algo, state, mo, st, go._observations(mo, st, pids, pts, var, lm_o)


@pytest.mark.parametrize("name", list(STATE_CASES))
def test_posterior_covariance_of_a_state(ctx, name):
    from gingr_amd.helper import posteriorVarianceMaps
    algo, state, mo, st, (pids, pts, covs) = state_case(ctx, name)
    try:
        if STATE_CASES[name][4]:
            assert np.allclose(st.rotation(), go.euler_to_rot(0.3, -0.2, 0.1)) and np.allclose(st.translation, (1.0, -2.0, 0.5))
        got = algo.posteriorCovariance(state)
        a, b = posterior_routes(mo, st, pids, pts, covs)
        check(name, mats(got), a, b)
        assert_psd_blocks(got)
        # the two analytic maps are the trace and n^T C n of the oracle blocks
        n = np.random.default_rng(3).normal(0, 1, (mo.M, 3))
        n /= np.linalg.norm(n, axis=1)[:, None]
        total, normal = posteriorVarianceMaps(got, n)
        spread = block_error(b, a)
        assert np.abs(total - np.trace(a, axis1=1, axis2=2)).max() <= 3000 * spread * np.abs(a).max((1, 2)).max()
        assert np.abs(normal - np.einsum("md,mde,me->m", n, a, n)).max() <= 3000 * spread * np.abs(a).max((1, 2)).max()
    finally:
        algo.close()


def test_surface_icp_posterior_on_the_femur_with_rejected_vertices(ctx):
    ref, cells, target, tcells = femur()
    mo, algo, state = make_state(ctx, ref, cells, target, tcells, rank=24, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
    try:
        st = oracle_state_of(state.general, 1)
        ocp, ow, _ = go.surface_correspondence(st.fit, cells, target, tcells)
        assert 0 < ow.sum() < ow.shape[0]                      # accepted and rejected (zero-weight) vertices
        pids = np.flatnonzero(ow == 1.0)
        covs = np.full(pids.shape[0], st.sigma2)[:, None, None] * np.eye(3)[None]
        got = algo.posteriorCovariance(state)
        a, b = posterior_routes(mo, st, pids, ocp[pids], covs)
        check("surface-icp-femur", mats(got), a, b)
        assert_psd_blocks(got)
    finally:
        algo.close()


@pytest.mark.parametrize("name", ["cpd-400x24-s1-posed", "icp-403x24-s1-posed", "cpd-211x130-s4"])
def test_the_query_leaves_the_state_alone(ctx, name):
    algo, state, mo, st, _ = state_case(ctx, name)
    try:
        nxt = algo.update(state)
        lp0 = algo.logTransitionProbability(state, nxt)
        fit_without = algo.update(state).general.fit
        retry0 = algo.retryCounter
        first = algo.posteriorCovariance(state)
        assert algo.retryCounter == retry0
        after = algo.update(state)
        assert np.array_equal(after.general.fit, fit_without)               # bit-identical update after the query
        assert np.array_equal(after.general.modelParameters.shape, nxt.general.modelParameters.shape)
        assert after.general.sigma2 == nxt.general.sigma2
        assert algo.logTransitionProbability(state, nxt) == lp0           # the same float
        assert np.array_equal(algo.posteriorCovariance(state), first)      # and the query repeats itself
    finally:
        algo.close()


def test_failed_posterior_raises(ctx):
    import gingr_amd as ga
    mo = model_of(400, 24)
    target = np.concatenate([mo.ref + mo.mean, [[5000.0, 0, 0]]])           # a target point no template point reaches: 1 / 0 in the sums
    algo = ga.CpdRegistration(ctx)
    try:
        s0 = algo.createInitialState(ga_model(mo), target, ga.CpdConfiguration(maxIterations=10, initialSigma=1.0, w=0.0))
        assert algo.logTransitionProbability(s0, s0) == float("-inf")
        with pytest.raises(ga.GingrNativeError):
            algo.posteriorCovariance(s0)
    finally:
        algo.close()
