"""GPU tests of the posterior as a resident model (gingr_amd/csrc/posterior_model.hip): DeviceModel.posterior and
GingrAlgorithm.posteriorModel against the oracle's restatement of scalismo's regression (go.PDM.transform + posterior_model).

Dense observations make the posterior spectrum nearly degenerate, so eigenvectors are not comparable column by column: every
comparison is invariant to sign and to rotation inside an eigenspace.  Quantities, from the model downloaded off the device:
  operator   Q_p Q_p^T (3M x 3M), Q_p = U_p sqrt(lambda_p)          max |difference| / max |expected|
  variance   lambda_p, descending and positive                       max |difference| / lambda_max
  mean       the mean mesh ref + mean, per original vertex id        max |difference| / max |expected|
  basis      max |U_p^T U_p - I| of the downloaded basis             judged against the same number of route A's basis
Error rule (the one of test_gpu_posterior_covariance.py), per quantity: the spread between two CPU routes must stay below 1e-13 -- a
condition on the inputs -- and the device may differ from route A by 1000 x that spread.
  route A = the oracle (pinv / SVD), route B = numpy Cholesky: Q L^-T, the singular values of L^-1 D, Q (L L^T)^-1 rhs.
Each check prints its figures before it asserts.
"""
import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests.test_gpu_posterior_covariance import (POSE, STATE_CASES, block_error, check, ga_model, mats, model_of, state_case,
                                                 three_landmarks)
from tests.test_gpu_surface_icp import femur, make_state, oracle_state_of

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the two CPU routes
class Routes:
    """operator, variance, mean mesh by both routes and the orthonormality defect of route A's basis, for the posterior of the
    (already posed) oracle model `posed` given (pids, pts, covs)"""

    def __init__(self, posed, pids, pts, covs, factor=None):
        pids, pts, covs = np.asarray(pids, dtype=np.int64), np.asarray(pts, dtype=np.float64), np.asarray(covs, dtype=np.float64)
        self.post = post = posed.posterior_model(pids, pts, covs)                       # route A
        Qa = post.U * np.sqrt(post.lam)[None, :]
        self.op_a, self.lam_a, self.mesh_a = Qa @ Qa.T, post.lam, post.ref + post.mean
        self.ortho_a = float(np.abs(post.U.T @ post.U - np.eye(post.rank)).max())
        # route B; `factor`: a 3M x r factor of the prior covariance that need not have orthogonal columns (a posterior's Q L^-T)
        r = posed.rank
        Q = posed.U * np.sqrt(posed.lam)[None, :] if factor is None else factor
        G, rhs = np.zeros((r, r)), np.zeros(r)
        for k, pid in enumerate(pids):
            Qk = Q[3 * pid:3 * pid + 3]
            G += Qk.T @ np.linalg.solve(covs[k], Qk)
            rhs += Qk.T @ np.linalg.solve(covs[k], pts[k] - posed.ref[pid] - posed.mean[pid])
        L = np.linalg.cholesky(np.eye(r) + G)
        self.Y = np.linalg.solve(L, Q.T).T                                               # Q L^-T
        self.op_b = self.Y @ self.Y.T
        sv = np.linalg.svd(np.linalg.solve(L, np.diag(np.sqrt(posed.lam))) if factor is None else self.Y, compute_uv=False)
        self.lam_b = sv ** 2
        a = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        self.mesh_b = posed.ref + posed.mean + (Q @ a).reshape(-1, 3)


def judge(name, what, got, a, b, scale):
    spread = float(np.abs(b - a).max() / scale)
    err = float(np.abs(got - a).max() / scale)
    print(f"{name} {what}: device error {err:.3e}, CPU spread {spread:.3e}, allowed {1000 * spread:.3e}")
    assert spread <= 1e-13, (name, what, spread)
    assert err <= 1000 * spread, (name, what, err, spread)


def check_model(name, dm, routes):
    """the model `dm` (a DeviceModel) against both routes"""
    got = dm.download()
    lam, U = np.asarray(got.variance), np.asarray(got.basis)
    assert U.shape == (3 * routes.post.M, routes.post.rank) and lam.shape == (routes.post.rank,)
    assert np.isfinite(U).all() and np.isfinite(lam).all()
    Q = U * np.sqrt(lam)[None, :]
    judge(name, "operator", Q @ Q.T, routes.op_a, routes.op_b, np.abs(routes.op_a).max())
    assert (lam > 0).all() and (np.diff(lam) <= 0).all(), (name, lam)
    judge(name, "variance", lam, routes.lam_a, routes.lam_b, routes.lam_a.max())
    judge(name, "mean", got.reference + got.mean, routes.mesh_a, routes.mesh_b, np.abs(routes.mesh_a).max())
    ortho = float(np.abs(U.T @ U - np.eye(lam.shape[0])).max())
    # (route A's number is exactly 0 for the one-vertex model, whose basis is a signed permutation: the defect is measured in
    # floating point, one rounding per entry of U^T U, so nothing below the unit roundoff can be asked of anybody)
    floor_a = max(routes.ortho_a, np.finfo(float).eps)
    print(f"{name} basis: max |U^T U - I| device {ortho:.3e}, route A {routes.ortho_a:.3e}, allowed {1000 * floor_a:.3e}")
    assert ortho <= 1000 * floor_a, (name, ortho, routes.ortho_a)
    return got


# ---------------------------------------------------------------------------------------------------------------- DeviceModel.posterior
# (M, r, sigma2, posed, landmarks): one vertex and a partial tile; a partial second tile, posed; posed with anisotropic landmarks;
# rp = 112, the last narrow rank; rp = 144, the first wide one; the rank ceiling, well and badly conditioned
MODEL_CASES = [(1, 5, 1.0, False, False), (17, 5, 1.0, True, False), (400, 24, 1.0, True, True), (257, 100, 1.0, False, False),
               (211, 130, 1.0, False, False), (200, 512, 1.0, False, False), (200, 512, 0.01, False, False)]


def dense_observations(mo, sigma2, posed, with_lm, seed=0):
    """(obs (M, 3), weights (M,), pose, oracle landmarks or None, oracle (pids, pts, covs)): nine points in ten observed with
    variance sigma2 (all of them below ten points), landmark points replace their dense observation"""
    rng = np.random.default_rng(31 * mo.M + mo.rank + seed)
    euler, t = POSE if posed else ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    c = np.array([2.0, -1.0, 3.0]) if posed else np.zeros(3)
    pm = mo.transform(go.euler_to_rot(*euler), np.array(t, dtype=np.float64), c)
    obs = pm.instance(rng.normal(0, 0.7, mo.rank)) + rng.normal(0, 0.3, (mo.M, 3))
    w = np.full(mo.M, 1.0 / sigma2)
    if mo.M >= 10:
        w[rng.permutation(mo.M)[: mo.M // 10]] = 0.0
    lm = three_landmarks(mo, obs + 0.5) if with_lm else None
    seen = w > 0
    if lm is not None:
        seen &= ~np.isin(np.arange(mo.M), lm.pids)
    pids = np.flatnonzero(seen)
    pts, covs = obs[pids], (1.0 / w[pids])[:, None, None] * np.eye(3)[None]
    if lm is not None:
        pids, pts, covs = np.concatenate([pids, lm.pids]), np.concatenate([pts, lm.points]), np.concatenate([covs, lm.covs])
    return obs, w, (euler, c, t), lm, pm, (pids, pts, covs)


def ga_landmarks(lm):
    import gingr_amd as ga
    return None if lm is None else ga.LandmarkCorrespondences(lm.pids.astype(np.int32), lm.points, lm.covs)


@pytest.mark.parametrize("M,r,sigma2,posed,with_lm", MODEL_CASES)
def test_posterior_of_a_model(ctx, M, r, sigma2, posed, with_lm):
    import gingr_amd as ga
    mo = model_of(M, r)
    obs, w, (euler, c, t), lm, pm, observations = dense_observations(mo, sigma2, posed, with_lm)
    dm = ga.DeviceModel(ctx, ga_model(mo))
    post = None
    try:
        post = dm.posterior(obs, w, euler, c, t, landmarks=ga_landmarks(lm))
        assert post.rank == mo.rank and post.M_local == M and post.handle.value != dm.handle.value
        got = check_model(f"model M={M} r={r} s2={sigma2}", post, Routes(pm, *observations))
        assert np.abs(got.reference - pm.ref).max() <= 8 * np.finfo(float).eps * np.abs(pm.ref).max()   # R (ref - c) + c + t
    finally:
        if post is not None:
            post.close()
        dm.close()


def test_row_order_follows_the_new_mean(ctx):
    """A landmark-only posterior whose mean moves by about 25 units where the reference spreads over 30: the rows of the new model
    sort differently from the source's, and everything is compared per original vertex id -- a wrong gather is an O(1) error."""
    import gingr_amd as ga
    mo = model_of(400, 24)
    rng = np.random.default_rng(12)
    pids = np.array([3, 200, 398])
    step = rng.normal(0, 1, (3, 3))
    pts = (mo.ref + mo.mean)[pids] + 25.0 * step / np.linalg.norm(step, axis=1)[:, None]
    covs = np.tile(0.25 * np.eye(3), (3, 1, 1))
    routes = Routes(mo, pids, pts, covs)
    moved = np.linalg.norm(routes.mesh_a - mo.ref - mo.mean, axis=1)
    assert moved.max() > 20.0 and moved.min() < 5.0                       # a non-rigid move of the size of the cloud
    dm = ga.DeviceModel(ctx, ga_model(mo))
    post = None
    try:
        post = dm.posterior(np.zeros((mo.M, 3)), np.zeros(mo.M), landmarks=ga.LandmarkCorrespondences(pids.astype(np.int32), pts, covs))
        check_model("row order", post, routes)
    finally:
        if post is not None:
            post.close()
        dm.close()


# ---------------------------------------------------------------------------------------------------------------- posteriorModel(state)
def state_routes(mo, st, pids, pts, covs):
    return Routes(mo.transform(st.rotation(), st.translation, st.center), pids, pts, covs)


@pytest.mark.parametrize("name", list(STATE_CASES))
def test_posterior_model_of_a_state(ctx, name):
    algo, state, mo, st, (pids, pts, covs) = state_case(ctx, name)
    post = None
    try:
        post = algo.posteriorModel(state)
        check_model(name, post, state_routes(mo, st, pids, pts, covs))
    finally:
        if post is not None:
            post.close()
        algo.close()


def test_surface_icp_posterior_model_on_the_femur_with_rejected_vertices(ctx):
    ref, cells, target, tcells = femur()
    mo, algo, state = make_state(ctx, ref, cells, target, tcells, rank=24, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
    post = None
    try:
        st = oracle_state_of(state.general, 1)
        ocp, ow, _ = go.surface_correspondence(st.fit, cells, target, tcells)
        assert 0 < ow.sum() < ow.shape[0]                      # accepted and rejected (zero-weight) vertices
        pids = np.flatnonzero(ow == 1.0)
        covs = np.full(pids.shape[0], st.sigma2)[:, None, None] * np.eye(3)[None]
        post = algo.posteriorModel(state)
        check_model("surface-icp-femur", post, state_routes(mo, st, pids, ocp[pids], covs))
        assert np.array_equal(post.host.cells, cells)          # cells are carried over from the source
    finally:
        if post is not None:
            post.close()
        algo.close()


# ---------------------------------------------------------------------------------------------------------------- a first-class model
def test_the_posterior_is_an_ordinary_resident_model(ctx):
    import gingr_amd as ga
    name = "cpd-400x24-initial-landmarks"
    algo, state, mo, st, (pids, pts, covs) = state_case(ctx, name)
    post = again = short = None
    try:
        post = algo.posteriorModel(state)
        routes = state_routes(mo, st, pids, pts, covs)
        # its prior marginal is the state's posterior covariance: two device routes, the oracle blocks as the reference
        U3 = routes.post.U.reshape(mo.M, 3, -1)
        blocks_a = np.einsum("mdk,k,mek->mde", U3, routes.post.lam, U3)
        Y3 = routes.Y.reshape(mo.M, 3, -1)
        blocks_b = np.einsum("mdk,mek->mde", Y3, Y3)
        check("marginal of the posterior model", mats(post.marginalCovariance()), blocks_a, blocks_b)
        check("posteriorCovariance of the state", mats(algo.posteriorCovariance(state)), blocks_a, blocks_b)
        cross = post.crossCovariance(7)
        assert block_error(cross[7], blocks_a[7]) <= 1000 * block_error(blocks_b, blocks_a)
        # instance(0) is the posterior mean mesh
        judge(name, "instance(0)", post.instance(np.zeros(post.rank)), routes.mesh_a, routes.mesh_b, np.abs(routes.mesh_a).max())
        # coefficients(instance(alpha)) = alpha up to the 1e-5 noise of the projection: the tolerance of the oracle's round trip
        # (test_oracle_kat.py: np.allclose(mo.coefficients(mo.instance(alpha)), alpha, atol=1e-5))
        alpha = np.random.default_rng(5).normal(0, 1, post.rank)
        assert np.allclose(routes.post.coefficients(routes.post.instance(alpha)), alpha, atol=1e-5)   # (holds for the oracle's model)
        back = post.coefficients(post.instance(alpha))
        print(f"coefficients round trip: max |difference| {np.abs(back - alpha).max():.3e}")
        assert np.allclose(back, alpha, atol=1e-5)
        # conditioned again on other observations = the oracle's posterior_model applied twice
        rng = np.random.default_rng(6)
        pids2 = np.sort(rng.permutation(mo.M)[:40])
        pts2 = routes.mesh_a[pids2] + rng.normal(0, 1.0, (40, 3))
        covs2 = np.tile(0.5 * np.eye(3), (40, 1, 1))
        second_b = go.PDM(routes.post.ref, routes.mesh_b - routes.post.ref, routes.post.U, routes.post.lam)   # route B's mean so far
        routes2 = Routes(routes.post, pids2, pts2, covs2)
        routes2_b = Routes(second_b, pids2, pts2, covs2, factor=routes.Y)
        routes2.op_b, routes2.lam_b, routes2.mesh_b = routes2_b.op_b, routes2_b.lam_b, routes2_b.mesh_b      # Cholesky both times
        obs2, w2 = np.zeros((mo.M, 3)), np.zeros(mo.M)
        obs2[pids2], w2[pids2] = pts2, 2.0
        again = post.posterior(obs2, w2)
        check_model("posterior of the posterior", again, routes2)
        # truncate: the leading functions of the same model
        short = post.truncate(10)
        full, cut = post.download(), short.download()
        assert short.rank == 10 and np.array_equal(cut.variance, full.variance[:10]) and np.array_equal(cut.basis, full.basis[:, :10])
        assert np.array_equal(cut.reference, full.reference) and np.array_equal(cut.mean, full.mean)
    finally:
        for m in (short, again, post):
            if m is not None:
                m.close()
        algo.close()


@pytest.mark.parametrize("name", ["cpd-400x24-s1-posed", "icp-403x24-s1-posed", "cpd-211x130-s4"])
def test_the_model_query_leaves_the_state_alone(ctx, name):
    algo, state, mo, st, _ = state_case(ctx, name)
    try:
        nxt = algo.update(state)
        lp0 = algo.logTransitionProbability(state, nxt)
        fit_without = algo.update(state).general.fit
        cov0 = algo.posteriorCovariance(state)
        retry0 = algo.retryCounter
        first = algo.posteriorModel(state)
        assert algo.retryCounter == retry0
        after = algo.update(state)
        assert np.array_equal(after.general.fit, fit_without)               # bit-identical update after the query
        assert np.array_equal(after.general.modelParameters.shape, nxt.general.modelParameters.shape)
        assert after.general.sigma2 == nxt.general.sigma2
        assert algo.logTransitionProbability(state, nxt) == lp0           # the same float
        assert np.array_equal(algo.posteriorCovariance(state), cov0)
        second = algo.posteriorModel(state)                                # and the query repeats itself
        a, b = first.download(), second.download()
        assert np.array_equal(a.basis, b.basis) and np.array_equal(a.variance, b.variance) and np.array_equal(a.mean, b.mean)
        first.close()
        second.close()
    finally:
        algo.close()


def test_failed_posterior_model_raises(ctx):
    import gingr_amd as ga
    mo = model_of(400, 24)
    target = np.concatenate([mo.ref + mo.mean, [[5000.0, 0, 0]]])           # a target point no template point reaches: 1 / 0 in the sums
    algo = ga.CpdRegistration(ctx)
    try:
        s0 = algo.createInitialState(ga_model(mo), target, ga.CpdConfiguration(maxIterations=10, initialSigma=1.0, w=0.0))
        before = algo.update(s0)
        retry0 = algo.retryCounter
        post = None
        with pytest.raises(ga.GingrNativeError) as e:
            post = algo.posteriorModel(s0)
        assert post is None and e.value.code in (ga._native.ERR_NOT_SPD, ga._native.ERR_NONFINITE)
        assert algo.retryCounter == retry0
        after = algo.update(s0)                                             # the following update behaves as before
        assert after.general.status == before.general.status and after.general.iteration == before.general.iteration
        assert np.array_equal(after.general.fit, before.general.fit, equal_nan=True)
    finally:
        algo.close()
