"""GPU tests of the dense covariance pairs of the fitter (gingr_fitter_set_pairs_cov_dense / gingr_fitter_get_pair_precisions,
gingr_amd/csrc/fitter_pairs.hip) and of the 3 x 3-weighted Gram pass behind them (gingr_amd/csrc/gp_gram_cov.hip).

Element-wise: G and rhs are read back through the `reduce` callback of gingr_fitter_update_sharded_async with one shard (the seam of
tests/test_gpu_posterior_solve_variants.py), the isotropic list and the landmarks empty, and compared with the formula in np.longdouble
evaluated on the pass's own inputs -- the consolidated planes as the device holds them (checked on their own below), the state's pose.
Bound per entry, u = 2^-53:  G: (3 M + 32) u sum_i 3 |W_i|_2 |Q_i[:, a]|_2 |Q_i[:, b]|_2;  rhs: the same with |v_i|_2 in place of one
column norm -- the plain summation bound, for the direct and the factored form alike.  It measures against |v_i|, so the inputs keep the
residuals at the size of the coordinates (the cancellation in forming v_i from coordinates is u |x|, not u |v_i|).
Consolidation: against the restatement in np.longdouble.  The device inverts by Cholesky, accurate to cond u (svd3.h: spd3_inverse), so
Lambda_i is held to 32 u max_k cond(Sigma_k) |Lambda_i|_max and the mean of several pairs -- two chained inversions -- to
64 u max_k cond(Sigma_k) cond(Lambda_i) |x|_max; a single pair's point and the empty vertices bit for bit.
Whole updates: the bounds tests/test_gpu_template_pairs.py and tests/test_gpu_posterior_covariance.py hold the landmark route to
(rel(fit) < 1e-5, |logpdf - want| < 1e-5 |want|, spread <= 1e-13 and err <= 1000 x spread, shards rel(fit) < 1e-9).
Largest error / bound ratio seen on an MI355X: DESIGN.md section 4."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import pairs_cov_gram_restatement as pr
from tests.test_gpu_posterior_covariance import check, ga_model, mats, model_of, posterior_routes, three_landmarks
from tests.test_gpu_posterior_model import check_model, state_routes
from tests.test_gpu_surface_icp import oracle_state_of, rel
from tests.test_gpu_template_pairs import HostSum, Raw, oracle_state, spd_covariances

pytestmark = pytest.mark.gpu

POSES = {"identity": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
         "posed": ((0.3, -0.2, 0.1), (4.0, -3.0, 2.0), (1.0, -2.0, 0.5))}          # euler, centre, translation
NONE_ISO = (np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0))


class Dense(Raw):
    """Raw plus the dense covariance list and the read-back of [G, rhs] between phase 1 and phase 2."""

    def set_dense(self, pids, pts, covs, expect_ok=True):
        from gingr_amd._native import dptr, iptr
        p, x, c = np.ascontiguousarray(pids, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(covs, dtype=np.float64)
        k = p.shape[0]
        rc = self.lib.gingr_fitter_set_pairs_cov_dense(self.h, k, iptr(p) if k else None, dptr(x) if k else None, dptr(c) if k else None)
        if expect_ok:
            self.ok(rc, "set_pairs_cov_dense")
        return rc

    def precisions(self):
        from gingr_amd._native import dptr
        M = self.sf.end - self.sf.begin
        obs, p6 = np.empty((M, 3)), np.empty((M, 6))
        self.ok(self.lib.gingr_fitter_get_pair_precisions(self.h, dptr(obs), dptr(p6)), "get_pair_precisions")
        return obs, p6

    def capture(self):
        """one sharded update of the pairs flavour on this single shard -> (G [rp][rp], rhs [rp]) as phase 1 left them"""
        from gingr_amd import _native as nat
        from gingr_amd import sharded
        rp = pr.padded(self.mo.rank)
        p = ctypes.c_void_p()
        offs, cnts = (ctypes.c_int64 * nat.NUM_SEGMENTS)(), (ctypes.c_int64 * nat.NUM_SEGMENTS)()
        self.ok(self.lib.gingr_fitter_exchange(self.h, ctypes.byref(p), offs, cnts), "gingr_fitter_exchange")
        assert cnts[1] >= rp * rp + rp + 8
        seg1 = sharded.as_torch(p.value + 8 * offs[1], cnts[1], self.ctx.device)
        got, err = [], []

        def reduce(_user, seg, _ptr, _count):
            try:
                if int(seg) == 1:
                    self.ctx.synchronize()  # phase 1 has written the segment
                    h = seg1.cpu().numpy()
                    got.append((h[: rp * rp].reshape(rp, rp).copy(), h[rp * rp: rp * rp + rp].copy()))
                return 0
            except BaseException as e:  # must not propagate through the C frame
                err.append(e)
                return 1
        cb = nat.ALLREDUCE_FN(reduce)
        rc = self.lib.gingr_fitter_update_sharded_async(self.h, 3, None, None, 1, None, cb, None)
        assert not err, err
        self.ok(rc, "update_sharded_async")
        assert len(got) == 1
        return got[0]


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def random_model(M, rank):
    """ref ~ N(0, 30^2), a mean, a random basis (any rank at any M: the Gram pass does not ask for orthonormal columns)"""
    rng = np.random.default_rng(7000 * rank + M)
    ref = rng.normal(0, 30, (M, 3))
    U = rng.normal(0, 1, (3 * M, rank)) / np.sqrt(3.0 * M)
    return go.PDM(ref=ref, mean=rng.normal(0, 0.5, (M, 3)), U=np.ascontiguousarray(U), lam=400.0 * 0.985 ** np.arange(rank))


def dense_inputs(mo, seed=0):
    """Reverse pid order; every fifth vertex (i % 5 == 1) without pairs; vertex 0 three times, with different covariances; even pairs
    normal / tangent with varTangent / varNormal = 1e8, odd pairs random SPD; residuals of the size of the coordinates."""
    rng = np.random.default_rng(seed + mo.M)
    M = mo.M
    seen = np.array([i for i in range(M) if i % 5 != 1], dtype=np.int64)
    pids = np.concatenate([[0, 0], seen])[::-1].copy()
    K = pids.shape[0]
    pts = (mo.ref + mo.mean)[pids] + rng.normal(0, 20.0, (K, 3))
    covs = spd_covariances(rng, K)
    vn = 10.0 ** rng.uniform(-4, -2, K)
    nt = pr.normal_tangent(rng.normal(0, 1, (K, 3)), vn, 1e8 * vn)
    covs[::2] = nt[::2]
    return pids, np.ascontiguousarray(pts), np.ascontiguousarray(covs)


def target_of(mo):
    return np.random.default_rng(5).normal(0, 30, (200, 3))


def lambda_of(p6):
    L = np.empty((p6.shape[0], 3, 3), dtype=p6.dtype)
    for q, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        L[:, a, b] = L[:, b, a] = p6[:, q]
    return L


def reference_system(mo, pose, obs, p6, masked=None):
    """(G, rhs, bound of G, bound of rhs) of the formula in np.longdouble on the device's planes"""
    euler, center, t = pose
    ld = np.longdouble
    W, v = pr.posed_terms(mo, go.euler_to_rot(*euler), center, t, obs, lambda_of(p6), dtype=ld, masked=masked)
    Q = pr.model_basis(mo, dtype=ld)
    G, rhs = pr.system(Q, W, v)
    bG, br = pr.bounds(Q, W, v, mo.M)
    return G, rhs, bG, br


def worst_ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want).astype(np.float64)
    assert (err[bound == 0.0] == 0.0).all()
    return float((err[bound > 0.0] / bound[bound > 0.0]).max()) if (bound > 0.0).any() else 0.0


def set_pose_state(f, mo, pose, alpha=None, sigma2=1.0, iteration=1):
    euler, center, t = pose
    st = go.State(alpha=np.zeros(mo.rank) if alpha is None else np.asarray(alpha, dtype=np.float64), euler=tuple(euler),
                  center=np.asarray(center, dtype=np.float64), translation=np.asarray(t, dtype=np.float64), scale=1.0, sigma2=sigma2,
                  fit=np.zeros((mo.M, 3)), iteration=iteration)
    st.fit = go.model_instance_shape_pose_scale(mo, st)
    f.set_state(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- 1. element-wise
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("rank, M", pr.GPU_SHAPES)
def test_gram_and_rhs_element_wise(ctx, rank, M, pose):
    mo = random_model(M, rank)
    pids, pts, covs = dense_inputs(mo)
    r, rp = mo.rank, pr.padded(mo.rank)
    f = Dense(ctx, mo, target_of(mo), transform=0)
    try:
        set_pose_state(f, mo, POSES[pose], alpha=np.random.default_rng(1).normal(0, 0.3, r))
        f.set_dense(pids, pts, covs)
        obs, p6 = f.precisions()
        G, rhs = f.capture()
    finally:
        f.close()
    wantG, want_rhs, bG, br = reference_system(mo, POSES[pose], obs, p6)
    rG, rr = worst_ratio(G[:r, :r], wantG, bG), worst_ratio(rhs[:r], want_rhs, br)
    print(f"rank {rank} M {M} {pose}: slabs {pr.plan(M, rp)[2]} x patches {pr.plan(M, rp)[1]}, worst error / bound: G {rG:.3e}, rhs {rr:.3e}")
    assert np.array_equal(G, G.T)                                                      # mirrored, not computed twice
    assert not G[r:, :].any() and not G[:, r:].any() and not rhs[r:].any()             # the padding columns of the basis are zero
    assert np.abs(wantG).max() > 0 and np.abs(want_rhs).max() > 0
    assert rG <= 1.0 and rr <= 1.0, (rG, rr)


# ---------------------------------------------------------------------------------------------------------------- 2. consolidation
def consolidation_inputs(M, seed):
    rng = np.random.default_rng(seed)
    seen = np.concatenate([rng.permutation(M - 1)[: max((M - 1) // 2, 0)], [M - 1]]).astype(np.int64)   # about half the vertices, the last one
    once, multi = seen[: (seen.shape[0] + 1) // 2], seen[(seen.shape[0] + 1) // 2:]                       # one pair each / several
    pids = np.concatenate([once, multi, rng.choice(multi, 2 * M)]) if multi.shape[0] else once
    pids = pids[rng.permutation(pids.shape[0])]
    K = pids.shape[0]
    return pids, rng.normal(0, 40, (K, 3)), spd_covariances(rng, K)


@pytest.mark.parametrize("M", [1, 255, 257, 600])
def test_consolidation_equals_the_restatement(ctx, M):
    mo = random_model(M, 16)
    pids, pts, covs = consolidation_inputs(M, M)
    f = Dense(ctx, mo, target_of(mo))
    try:
        obs0, p0 = f.precisions()
        assert not obs0.any() and not p0.any()                                         # before the first list: no pair anywhere
        f.set_dense(pids, pts, covs)
        obs, p6 = f.precisions()
        u = pr.U53
        want_obs, want_L, n = pr.consolidate(M, pids, pts, covs, dtype=np.longdouble)
        cond_k = np.linalg.cond(covs)
        cmax = np.zeros(M)
        np.maximum.at(cmax, pids, cond_k)
        errL = np.abs(p6 - pr.prec6(want_L).astype(np.float64)).max(axis=1)
        tolL = 32 * u * cmax * np.abs(pr.prec6(want_L).astype(np.float64)).max(axis=1)
        assert (errL <= tolL).all(), float((errL / np.maximum(tolL, 1e-300)).max())
        one, many, none = n == 1, n > 1, n == 0
        assert one.sum() >= 1 and (M == 1 or (many.any() and none.any()))
        where = np.array([np.flatnonzero(pids == i)[0] for i in np.flatnonzero(one)], dtype=np.int64)
        assert np.array_equal(obs[one], pts[where])                                    # a single pair's point: bit for bit
        assert not obs[none].any() and not p6[none].any()
        if many.any():
            errx = np.abs(obs[many] - want_obs[many].astype(np.float64)).max(axis=1)
            tolx = 64 * u * cmax[many] * np.linalg.cond(want_L[many].astype(np.float64)) * np.abs(pts).max()
            print(f"M {M}: {int(many.sum())} vertices with several pairs, worst error / bound {float((errx / tolx).max()):.3e}")
            assert (errx <= tolx).all()
        # permuting the pairs of DIFFERENT vertices (each vertex's own pairs keep their order): the same planes, the same update
        order = np.concatenate([np.flatnonzero(pids == i) for i in np.unique(pids)[::-1]])
        assert not np.array_equal(order, np.arange(pids.shape[0])) or M == 1
        st = set_pose_state(f, mo, POSES["posed"])
        _, _, fit_a = f.update()
        f.set_dense(pids[order], pts[order], covs[order])
        obs_b, p6_b = f.precisions()
        f.set_state(st)
        _, _, fit_b = f.update()
        assert np.array_equal(obs_b, obs) and np.array_equal(p6_b, p6) and np.array_equal(fit_a, fit_b)
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 3. agreement of routes
def pair_bound(mo, pose, pids, pts, covs):
    """the summation bound of a route that adds pair by pair (the landmark pass; the isotropic pass at one pair per vertex)"""
    euler, center, t = pose
    R = go.euler_to_rot(*euler)
    Q = pr.model_basis(mo)[pids]
    W = np.einsum("ia,kij,jb->kab", R, np.linalg.inv(covs), R)
    v = (pts - np.asarray(center) - np.asarray(t)) @ R - (mo.ref - np.asarray(center) + mo.mean)[pids]
    wn, cn = np.linalg.norm(W, 2, axis=(1, 2)), np.linalg.norm(Q, axis=1)
    fac = (3 * mo.M + 32) * pr.U53 * 3.0
    return fac * np.einsum("k,ka,kb->ab", wn, cn, cn), fac * np.einsum("k,ka,k->a", wn, cn, np.linalg.norm(v, axis=1))


@pytest.mark.parametrize("rank", [24, 136])
def test_the_dense_route_agrees_with_the_landmark_and_the_isotropic_route(ctx, rank):
    mo = random_model(600, rank)
    r = mo.rank
    rng = np.random.default_rng(3)
    base = rng.permutation(mo.M)[:35]
    cp = np.concatenate([base, rng.choice(base, 15)])[rng.permutation(50)].astype(np.int64)      # 50 repeated, unordered pids
    cx = (mo.ref + mo.mean)[cp] + rng.normal(0, 20.0, (50, 3))
    cc = spd_covariances(rng, 50)
    pose = POSES["posed"]
    f = Dense(ctx, mo, target_of(mo), transform=0)
    try:
        set_pose_state(f, mo, pose)
        f.set_pairs_cov(cp, cx, cc)
        G1, r1 = f.capture()
        f.set_pairs_cov([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        set_pose_state(f, mo, pose)
        f.set_dense(cp, cx, cc)
        obs, p6 = f.precisions()
        G2, r2 = f.capture()
        _, _, bG, br = reference_system(mo, pose, obs, p6)
        pG, pr_ = pair_bound(mo, pose, cp, cx, cc)
        # (the dense route forms xbar_i first: its share of the rhs bound is measured on the consolidated terms, the landmark route's pair by pair)
        print(f"rank {rank} landmark route: worst G {float((np.abs(G1 - G2)[:r, :r] / (bG + pG)).max()):.3e}, "
              f"rhs {float((np.abs(r1 - r2)[:r] / (br + pr_)).max()):.3e} of the two bounds")
        assert np.abs(G2).max() > 0 and (np.abs(G1 - G2)[:r, :r] <= bG + pG).all() and (np.abs(r1 - r2)[:r] <= br + pr_).all()
        # cov = v_k I through the dense call against set_pairs(var = v_k), one pair per vertex
        ip = rng.permutation(mo.M)[:400].astype(np.int64)
        ix = (mo.ref + mo.mean)[ip] + rng.normal(0, 20.0, (400, 3))
        iv = 10.0 ** rng.uniform(-2, 2, 400)
        f.set_dense(ip, ix, iv[:, None, None] * np.eye(3)[None])
        set_pose_state(f, mo, pose)
        G3, r3 = f.capture()
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        f.set_pairs(ip, ix, iv)
        set_pose_state(f, mo, pose)
        G4, r4 = f.capture()
        pG, pr_ = pair_bound(mo, pose, ip, ix, iv[:, None, None] * np.eye(3)[None])
        print(f"rank {rank} isotropic route: worst G {float((np.abs(G3 - G4)[:r, :r] / (2 * pG)).max()):.3e}, "
              f"rhs {float((np.abs(r3 - r4)[:r] / (2 * pr_)).max()):.3e} of the two bounds")
        assert np.abs(G4).max() > 0 and (np.abs(G3 - G4)[:r, :r] <= 2 * pG).all() and (np.abs(r3 - r4)[:r] <= 2 * pr_).all()
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 4. whole updates
M_WHOLE = 2500


@functools.lru_cache(maxsize=None)
def whole_case(rank):
    """one pair per vertex on 2 500 points: a displaced, rotated instance seen through normal / tangent covariances of moderate
    anisotropy (sigma2 of order 1: the conditioning of the siblings' cases)"""
    mo = model_of(M_WHOLE, rank)
    rng = np.random.default_rng(rank)
    truth = mo.instance(rng.normal(0, 0.6, mo.rank)) @ go.euler_to_rot(0.05, -0.04, 0.03).T + np.array([2.0, -1.0, 1.5])
    pids = rng.permutation(mo.M).astype(np.int64)
    pts = truth[pids] + rng.normal(0, 0.5, (mo.M, 3))
    covs = pr.normal_tangent(rng.normal(0, 1, (mo.M, 3)), rng.uniform(0.5, 1.0, mo.M), rng.uniform(4.0, 10.0, mo.M))
    return mo, rng.normal(0, 30, (300, 3)), pids, np.ascontiguousarray(pts), np.ascontiguousarray(covs)


def as_landmarks(mo, st, pids, pts, covs, z=None):
    return go.update_from_observations(mo, st, *NONE_ISO, st.sigma2, landmarks=go.Landmarks(pids, pts, covs), z=z)


def logpdf_of(mo, st, pids, pts, covs, mesh):
    post = mo.transform(st.rotation(), st.translation, st.center).posterior_model(pids, pts, covs)
    return go.gp_logpdf(post.coefficients(mesh))


@pytest.mark.parametrize("rank", [100, 256])
def test_update_sampled_update_and_density_against_the_oracle(ctx, rank):
    mo, target, pids, pts, covs = whole_case(rank)
    st = oracle_state(mo, np.random.default_rng(rank + 1).normal(0, 0.3, mo.rank), 2.0, iteration=1)
    z = np.random.default_rng(11).standard_normal(mo.rank)
    f = Dense(ctx, mo, target)
    try:
        f.set_state(st)
        f.set_dense(pids, pts, covs)
        _, sc, fit = f.update()
        want = as_landmarks(mo, st, pids, pts, covs)
        print(f"rank {rank} update: rel(fit) {rel(fit, want.fit):.3e}")
        assert sc.status == want.status == 0 and sc.iteration == 2 and rel(fit, want.fit) < 1e-5 and rel(fit, st.fit) > 1e-4
        f.set_state(st)
        got = f.logpdf(st.fit)
        lp = logpdf_of(mo, st, pids, pts, covs, st.fit)
        print(f"rank {rank}: logpdf {got!r} oracle {lp!r}")
        assert np.isfinite(got) and abs(got - lp) < 1e-5 * abs(lp)
        _, scz, fitz = f.update(z)                                                     # (the memo of the query serves the proposal)
        wantz = as_landmarks(mo, st, pids, pts, covs, z=z)
        print(f"rank {rank} sampled: rel(fit) {rel(fitz, wantz.fit):.3e}")
        assert scz.status == wantz.status == 0 and rel(fitz, wantz.fit) < 1e-5 and rel(wantz.fit, want.fit) > 1e-6
    finally:
        f.close()


def gram_state(ctx, mo, target, pairs, covs, landmarks=None, sigma2=2.0):
    import gingr_amd as ga
    algo = ga.TemplateRegistration(ctx, lambda s: pairs, lambda p, s: covs, covariancePass="gram")
    lm = None if landmarks is None else ga.LandmarkCorrespondences(landmarks.pids.astype(np.int32), landmarks.points, landmarks.covs)
    state = algo.createInitialState(ga_model(mo), target, ga.TemplateConfiguration(maxIterations=1), landmarks=lm,
                                    initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)), sigma2=sigma2)
    return algo, state


@pytest.mark.parametrize("rank", [100, 256])
def test_posterior_covariance_and_model_against_the_oracle(ctx, rank):
    import gingr_amd as ga
    mo, target, pids, pts, covs = whole_case(rank)
    algo, state = gram_state(ctx, mo, target, ga.CorrespondencePairs(pids, pts), covs)
    post = None
    try:
        st = oracle_state_of(state.general, 1)
        got = algo.posteriorCovariance(state)
        a, b = posterior_routes(mo, st, pids, pts, covs)
        check(f"dense pairs r={rank}", mats(got), a, b)
        post = algo.posteriorModel(state)
        check_model(f"dense pairs r={rank}", post, state_routes(mo, st, pids, pts, covs))
        nxt = algo.update(state)                                                       # the queries left state and memo usable
        want = as_landmarks(mo, st, pids, pts, covs)
        assert nxt.general.status == 0 and rel(nxt.general.fit, want.fit) < 1e-5
    finally:
        if post is not None:
            post.close()
        algo.close()


def test_three_lists_at_once_on_overlapping_vertices(ctx):
    mo, target, pids, pts, covs = whole_case(100)
    rng = np.random.default_rng(21)
    ip = rng.choice(pids[:900], 700).astype(np.int64)                                   # isotropic, repeated, inside the dense range
    ix = (mo.ref + mo.mean)[ip] + rng.normal(0, 1.0, (700, 3))
    iv = rng.uniform(0.5, 4.0, 700)
    cp = np.concatenate([ip[:20], pids[1000:1020]]).astype(np.int64)                    # landmark-pass list: on both other lists
    cx = (mo.ref + mo.mean)[cp] + rng.normal(0, 1.0, (40, 3))
    cc = spd_covariances(rng, 40)
    dp, dx, dc = pids[:1500], pts[:1500], covs[:1500]                                   # dense
    all_p, all_x = np.concatenate([ip, cp, dp]), np.concatenate([ix, cx, dx])
    all_c = np.concatenate([iv[:, None, None] * np.eye(3)[None], cc, dc])
    st = oracle_state(mo, rng.normal(0, 0.3, mo.rank), 2.0, iteration=1)
    f = Dense(ctx, mo, target)
    try:
        f.set_state(st)
        f.set_dense(dp, dx, dc)
        f.set_pairs(ip, ix, iv)
        f.set_pairs_cov(cp, cx, cc)
        got = f.logpdf(st.fit)
        lp = logpdf_of(mo, st, all_p, all_x, all_c, st.fit)
        _, sc, fit = f.update()
        want = as_landmarks(mo, st, all_p, all_x, all_c)
        print(f"three lists: logpdf {got!r} oracle {lp!r}, rel(fit) {rel(fit, want.fit):.3e}")
        assert abs(got - lp) < 1e-5 * abs(lp) and sc.status == want.status == 0 and rel(fit, want.fit) < 1e-5
    finally:
        f.close()


def test_a_landmark_takes_the_dense_pairs_of_its_vertex(ctx):
    """set_landmarks after set_pairs_cov_dense and before it: the landmark's vertex without its dense pairs"""
    from gingr_amd._native import dptr, iptr
    mo, target, pids, pts, covs = whole_case(100)
    lm = three_landmarks(mo, target)
    keep = ~np.isin(pids, lm.pids)
    assert keep.sum() == mo.M - 3
    st = oracle_state(mo, np.zeros(mo.rank), 2.0, iteration=1)
    want = as_landmarks(mo, st, np.concatenate([pids[keep], lm.pids]), np.concatenate([pts[keep], lm.points]), np.concatenate([covs[keep], lm.covs]))
    kept = as_landmarks(mo, st, np.concatenate([pids, lm.pids]), np.concatenate([pts, lm.points]), np.concatenate([covs, lm.covs]))
    assert rel(kept.fit, want.fit) > 1e-7                                              # (the override is seen)
    lp, lx, lc = lm.pids.astype(np.int32), np.ascontiguousarray(lm.points), np.ascontiguousarray(lm.covs)
    fits = []
    for first in ("pairs", "landmarks"):
        f = Dense(ctx, mo, target)
        try:
            f.set_state(st)
            if first == "pairs":
                f.set_dense(pids, pts, covs)
            f.ok(f.lib.gingr_fitter_set_landmarks(f.h, 3, iptr(lp), dptr(lx), dptr(lc)), "set_landmarks")
            if first != "pairs":
                f.set_dense(pids, pts, covs)
            _, sc, fit = f.update()
            print(f"{first} first: rel(fit) {rel(fit, want.fit):.3e}")
            assert sc.status == want.status == 0 and rel(fit, want.fit) < 1e-5 and rel(fit, want.fit) < 0.1 * rel(kept.fit, want.fit)
            fits.append(fit)
        finally:
            f.close()
    assert np.array_equal(fits[0], fits[1])


def test_two_row_shards_equal_the_single_shard():
    import torch
    import gingr_amd as ga
    from gingr_amd._native import dptr
    mo, target, pids, pts, covs = whole_case(100)
    st = oracle_state(mo, np.random.default_rng(6).normal(0, 0.3, mo.rank), 2.0, iteration=1)
    z = np.random.default_rng(7).standard_normal(mo.rank)
    world = 2
    c1 = ga.Context(0)
    one = Dense(c1, mo, target)
    ctxs = [ga.Context(0) for _ in range(world)]
    shards = [Dense(ctxs[r], mo, target, rank=r, world=world, defer=True) for r in range(world)]
    try:
        def load(f):
            f.set_state(st)
            f.set_dense(pids, pts, covs)                                                # the WHOLE list on every shard
        load(one)
        lp1 = one.logpdf(st.fit)
        _, sc1, fit1 = one.update()
        one.set_state(st)
        _, _, fit1z = one.update(z)
        mom = None
        for f in shards:                                                               # the model's moments, summed once (tests/test_gpu_group.py)
            g = f.sf.gram_tensor()
            f.ctx.synchronize()
            mom = g.clone() if mom is None else mom + g
        for f in shards:
            f.sf.gram_tensor().copy_(mom)
            torch.cuda.synchronize()
            f.sf.finish_setup()
            load(f)
        # a shard keeps the pairs of its own rows
        obs1, p1 = one.precisions()
        parts = [f.precisions() for f in shards]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), obs1) and np.array_equal(np.concatenate([p[1] for p in parts]), p1)
        hs = HostSum(shards)
        zz, mesh = np.ascontiguousarray(z), np.ascontiguousarray(st.fit)
        outs = [ctypes.c_double() for _ in shards]
        rcs = hs.run(lambda r, cb: shards[r].lib.gingr_fitter_posterior_logpdf_sharded(shards[r].h, 3, None, None, dptr(mesh), cb, None,
                                                                                       ctypes.byref(outs[r])))
        assert rcs == [0] * world
        for o in outs:
            assert abs(o.value - lp1) <= 1e-9 * abs(lp1), (o.value, lp1)
        rcs = hs.run(lambda r, cb: shards[r].lib.gingr_fitter_update_sharded_async(shards[r].h, 3, None, None, 1, None, cb, None))
        assert rcs == [0] * world
        states = [f.sf.get_state() for f in shards]
        fit = np.concatenate([s[2] for s in states])
        print(f"{world} shards: rel(fit) {rel(fit, fit1):.3e}")
        assert all(s[1].status == 0 and s[1].iteration == 2 for s in states) and sc1.status == 0 and rel(fit, fit1) < 1e-9
        for f in shards:
            f.set_state(st)
        rcs = hs.run(lambda r, cb: shards[r].lib.gingr_fitter_update_sharded_async(shards[r].h, 3, None, None, 1, dptr(zz), cb, None))
        assert rcs == [0] * world
        fitz = np.concatenate([f.sf.get_state()[2] for f in shards])
        print(f"{world} shards, sampled: rel(fit) {rel(fitz, fit1z):.3e}")
        assert rel(fitz, fit1z) < 1e-9 and rel(fit1z, fit1) > 1e-6
    finally:
        for f in shards + [one]:
            f.close()
        for c in ctxs + [c1]:
            c.close()


# ---------------------------------------------------------------------------------------------------------------- 5. state rules
@pytest.mark.parametrize("kind", ["non-finite", "negative-eigenvalue"])
def test_failure_rules(ctx, kind):
    mo = random_model(600, 24)
    pids, pts, covs = dense_inputs(mo)
    bad = covs.copy()
    if kind == "non-finite":
        bad[5, 0, 0] = np.nan
    else:
        bad[5] = np.diag([1.0, -0.5, 2.0])
    alpha0 = np.random.default_rng(2).normal(0, 0.3, mo.rank)
    f = Dense(ctx, mo, target_of(mo))
    try:
        f.set_dense(pids, pts, bad)
        f.set_state(oracle_state(mo, alpha0, 2.0, iteration=0))                        # iteration 0: the state stays as it is
        alpha, sc, _ = f.update()
        assert sc.status == 0 and sc.iteration == 1 and np.array_equal(alpha, alpha0) and sc.sigma2 == 2.0
        st1 = oracle_state(mo, alpha0, 2.0, iteration=1)
        f.set_state(st1)                                                               # later: ModelFlexibilityError
        alpha, sc, _ = f.update()
        assert sc.status == go.STATUS_MODEL_FLEXIBILITY_ERROR and np.array_equal(alpha, alpha0)
        f.set_state(st1)                                                               # sampled: unchanged, one retry used up
        assert f.retry() == 10
        alpha, sc, fit = f.update(np.random.default_rng(0).standard_normal(mo.rank))
        assert sc.status == 0 and sc.iteration == 2 and np.array_equal(alpha, alpha0) and f.retry() == 9
        f.set_dense(pids, pts, covs)                                                   # the same list with a covariance in its place: fine
        f.set_state(st1)
        _, sc, _ = f.update()
        assert sc.status == 0
    finally:
        f.close()


def test_clear_memo_and_bad_pid(ctx):
    mo = random_model(600, 24)
    pids, pts, covs = dense_inputs(mo)
    st = oracle_state(mo, np.random.default_rng(3).normal(0, 0.3, mo.rank), 4.0, iteration=1)
    f, fresh = Dense(ctx, mo, target_of(mo)), Dense(ctx, mo, target_of(mo))
    try:
        f.set_state(st)
        f.set_dense(pids, pts, covs)
        a1 = f.logpdf(st.fit)
        f.set_state(st)
        a2 = f.logpdf(st.fit)                                                          # from the memo
        assert abs(a2 - a1) <= 1e-9 * abs(a1)
        # a pid out of range is refused and nothing is changed: planes, memo'd density and the next update
        before = f.precisions()
        for bad_pid in (-1, mo.M):
            rc = f.set_dense(np.concatenate([pids[:5], [bad_pid]]), pts[:6], covs[:6], expect_ok=False)
            assert rc == 1, rc                                                         # GINGR_ERR_BAD_ARGUMENT
        after = f.precisions()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # other points, the same state: the memo is forgotten, another posterior
        other = pts + np.random.default_rng(9).normal(0, 5.0, pts.shape)
        f.set_dense(pids, other, covs)
        b1 = f.logpdf(st.fit)
        fresh.set_state(st)
        fresh.set_dense(pids, other, covs)
        assert b1 == fresh.logpdf(st.fit) and abs(b1 - a1) > 1e-6 * abs(a1)
        # K = 0 clears the list: the update without observations, bit for bit that of a fitter that never had a list
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        obs, p6 = f.precisions()
        assert not obs.any() and not p6.any()
        never = Dense(ctx, mo, target_of(mo))
        try:
            f.set_state(st)
            never.set_state(st)
            al_f, sc_f, fit_f = f.update()
            al_n, sc_n, fit_n = never.update()
            assert sc_f.status == sc_n.status == 0 and np.array_equal(fit_f, fit_n) and np.array_equal(al_f, al_n)
        finally:
            never.close()
    finally:
        f.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("rank", [100, 256])
def test_two_fitters_and_two_runs_give_the_same_bits(ctx, rank):
    mo, target, pids, pts, covs = whole_case(rank)
    st = oracle_state(mo, np.random.default_rng(4).normal(0, 0.3, mo.rank), 2.0, iteration=1)
    a, b = Dense(ctx, mo, target), Dense(ctx, mo, target)
    try:
        outs = []
        for f in (a, b, a):
            f.set_state(st)
            f.set_dense(pids, pts, covs)
            G, rhs = f.capture()
            alpha, _, fit = f.sf.get_state()
            outs.append((G, rhs, alpha, fit))
        for o in outs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(o, outs[0]))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 7. nothing else moved
def test_set_then_cleared_leaves_the_isotropic_update_as_it_was(ctx):
    mo, target, pids, pts, covs = whole_case(100)
    rng = np.random.default_rng(8)
    ip = rng.choice(mo.M, 3000).astype(np.int64)
    ix = (mo.ref + mo.mean)[ip] + rng.normal(0, 1.0, (3000, 3))
    iv = 10.0 ** rng.uniform(-1, 1, 3000)
    st = oracle_state(mo, rng.normal(0, 0.3, mo.rank), 2.0, iteration=1)
    f, never = Dense(ctx, mo, target), Dense(ctx, mo, target)
    try:
        f.set_state(st)
        f.set_pairs(ip, ix, iv)
        f.set_dense(pids, pts, covs)
        _, _, moved = f.update()
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        f.set_state(st)
        G_f, r_f = f.capture()
        al_f, sc_f, fit_f = f.sf.get_state()
        never.set_state(st)
        never.set_pairs(ip, ix, iv)
        G_n, r_n = never.capture()
        al_n, sc_n, fit_n = never.sf.get_state()
        assert sc_f.status == sc_n.status == 0 and not np.array_equal(moved, fit_n)
        assert np.array_equal(G_f, G_n) and np.array_equal(r_f, r_n) and np.array_equal(al_f, al_n) and np.array_equal(fit_f, fit_n)
    finally:
        f.close()
        never.close()


# ---------------------------------------------------------------------------------------------------------------- 8. leaks
def test_create_set_update_destroy_gives_the_memory_back(ctx):
    import torch
    mo, target, pids, pts, covs = whole_case(100)
    st = oracle_state(mo, np.zeros(mo.rank), 2.0, iteration=1)

    def free_bytes():
        torch.cuda.synchronize(0)
        return torch.cuda.mem_get_info(0)[0]

    def cycle():
        f = Dense(ctx, mo, target)
        try:
            f.set_state(st)
            f.set_dense(pids[:1000], pts[:1000], covs[:1000])
            f.set_dense(pids, pts, covs)                                               # grows the list
            _, sc, _ = f.update()
            assert sc.status == 0
            f.precisions()
        finally:
            f.close()

    cycle()                                                                            # warm-up: code objects, allocator pools
    gc.collect()
    before = free_bytes()
    for _ in range(4):
        cycle()
    gc.collect()
    after = free_bytes()
    assert before - after < 16 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"


# ---------------------------------------------------------------------------------------------------------------- 9. Python
def test_covariance_pass_of_template_registration(ctx):
    import gingr_amd as ga
    mo = model_of(600, 24)
    rng = np.random.default_rng(12)
    target = rng.normal(0, 30, (300, 3))
    base = rng.permutation(mo.M)[:45]
    pids = np.concatenate([base, rng.choice(base, 15)])[rng.permutation(60)].astype(np.int64)     # 60 pairs
    pts = (mo.ref + mo.mean)[pids] + rng.normal(0, 2.0, (60, 3))
    covs = ga.normalTangentCovariances(rng.normal(0, 1, (60, 3)), rng.uniform(0.2, 1.0, 60), rng.uniform(3.0, 9.0, 60))
    pairs = ga.CorrespondencePairs(pids, pts)
    with pytest.raises(ValueError):
        ga.TemplateRegistration(ctx, covariancePass="mfma")
    assert ga.TemplateRegistration(ctx).covariancePass == "landmark"
    fits = {}
    for route in ("landmark", "gram"):
        algo = ga.TemplateRegistration(ctx, lambda s: pairs, lambda p, s: covs, covariancePass=route)
        try:
            state = algo.createInitialState(ga_model(mo), target, ga.TemplateConfiguration(maxIterations=1),
                                            initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)), sigma2=2.0)
            st = oracle_state_of(state.general, 1)
            obs, prec = algo.pairPrecisions(state)
            assert prec.any() == (route == "gram") and obs.any() == (route == "gram")
            nxt = algo.update(state)
            want = as_landmarks(mo, st, pids, pts, covs)
            print(f"covariancePass={route}: rel(fit) {rel(nxt.general.fit, want.fit):.3e}")
            assert nxt.general.status == 0 and rel(nxt.general.fit, want.fit) < 1e-5
            fits[route] = nxt.general.fit
        finally:
            algo.close()
    # agreement to rounding, not bit for bit: within the sum of the two routes' bounds against the oracle
    print(f"gram against landmark: rel(fit) {rel(fits['gram'], fits['landmark']):.3e}")
    assert rel(fits["gram"], fits["landmark"]) < 2e-5
