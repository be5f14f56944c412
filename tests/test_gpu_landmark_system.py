"""landmarks_kernel (gingr_amd/csrc/gp_obs.hip) element by element: G [r r] and rhs [r] of every observation that carries a full 3 x 3
covariance, copied out of exchange segment 1 by a read-only reduce callback (the seam of test_gpu_posterior_solve_variants.py) and held
against the extended-precision reference of tests/landmark_system_cases.py.

Flavour: pairs given (Template) without isotropic pairs, so that the dense part of G and rhs is zero and the segment holds the kernel's
sums alone (test_nothing_observed_leaves_a_zero_system pins that on the same seam).  Lists of up to three entries go through
gingr_fitter_set_landmarks, longer ones through gingr_fitter_set_pairs_cov, the concatenated case through both.  Short landmark lists run
once more through the point-cloud ICP flavour, the dense part removed by capturing the same state twice, with and without the list.

Bound, per case and computed on the host: max |G_dev - G_ref| / max Gabs <= 1 000 x the same figure of the float64 route (np.linalg.inv,
float64 sums), and likewise for rhs; G symmetric to twice that.  No bound depends on device output.

Measured on an MI355X.  Every test prints its rows (deviation | float64 route | bound, G then rhs, and G's asymmetry); the table was
collated from the prints of one run of this file.  `before`: the same run against the library built from the parent commit, whose
kernel inverted the covariance by cofactors -- the six needle / graded rows, the ICP row of needle and the posterior mean missed
their bounds there, everything else passed with either inverse:

    case                           before G  G         float64   bound      before rhs  rhs       float64   bound
    r24-L257-needle-skew           1.66e-07  8.74e-13  1.09e-12  1.09e-09   1.73e-07    1.96e-12  1.88e-12  1.88e-09
    r264-L600-needle-skew          1.34e-07  1.59e-12  9.33e-13  9.33e-10   1.23e-07    2.39e-12  1.41e-12  1.41e-09
    r264-L3-needle-skew            1.63e-06  1.44e-11  7.40e-12  7.40e-09   1.48e-06    1.99e-11  1.01e-11  1.01e-08
    r512-L257-needle-skew          1.99e-07  2.81e-12  3.46e-12  3.46e-09   5.24e-07    3.32e-12  2.56e-12  2.56e-09
    r24-L257-graded-skew           5.16e-07  6.23e-11  1.03e-10  1.03e-07   1.19e-07    1.89e-10  1.90e-10  1.90e-07
    r264-L257-graded-skew          4.05e-07  3.29e-10  1.32e-10  1.32e-07   2.99e-07    3.40e-10  1.35e-10  1.35e-07
    r24-L257-pancake-skew          2.76e-10  2.19e-10  1.13e-10  1.13e-07   2.65e-10    2.97e-10  3.31e-10  3.31e-07
    r264-L257-pancake-skew         4.99e-10  5.25e-10  3.27e-10  3.27e-07   4.01e-10    4.55e-10  2.84e-10  2.84e-07
    well, iso (14 cases), largest  2.01e-15  2.01e-15  4.13e-16  4.13e-13   4.37e-15    3.96e-15  4.37e-15  4.37e-12   (r512-L600, r512-L1)
    -1 rows (r264-L600-override)   1.06e-15  1.06e-15  4.27e-16  4.27e-13   1.51e-16    1.49e-16  2.44e-16  2.44e-13
    two shards, either partial     2.02e-16  3.87e-16  7.23e-16  7.23e-13   2.07e-16    3.15e-16  4.22e-16  4.22e-13
    two shards, the sum            8.15e-17  2.30e-16  2.30e-16  2.30e-13   1.60e-16    2.10e-16  2.56e-16  2.56e-13
    ICP flavour r264-L3-needle     1.63e-06  1.44e-11  7.40e-12  7.40e-09   1.48e-06    1.99e-11  1.01e-11  1.01e-08
    posterior_mean, error in a     5.23e-08  7.77e-12  4.23e-12  4.23e-09
    asymmetry of G, largest        2.10e-16  2.10e-16            2 x bound

No case is within a factor 100 of its bound with the Cholesky inverse; before, `graded` missed by a factor 2 to 5 (the rhs of r24 passed),
`needle` by 90 to 220.
"""
import ctypes

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import landmark_system_cases as lc
from tests import posterior_solve_cases as pc
from tests.test_gpu_template_pairs import HostSum, oracle_state_of, rel, template_state

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")]

PAIRS, ICP = 3, 1          # flavours of gingr_fitter_update_sharded_async


class Capture:
    """One model of lc.model_parts(r), one fitter on rows [begin, end) of it, and the read-only copy of segment 1 after phase 1."""

    def __init__(self, ctx, r, rank=0, world=1, target=None):
        import gingr_amd as ga
        from gingr_amd import _native as nat
        from gingr_amd import sharded
        self.nat, self.ctx, self.r, self.rp, self.world = nat, ctx, r, pc.rp_of(r), world
        ref, mean, U, lam = (np.array(a) for a in lc.model_parts(r))
        if target is None:
            target = ref + mean + 1.0
        self.sf = sharded.ShardedFitter(ctx, ga.PointDistributionModel(ref, mean, U, lam), target, rank=rank, world=world,
                                        all_reduce=(lambda t: None) if world > 1 else None, defer_setup=world > 1)
        self.seg1 = None
        self.captured = None
        self.cb_error = None
        self.cb = nat.ALLREDUCE_FN(self._reduce)

    def segment1(self):
        if self.seg1 is None:
            from gingr_amd import sharded
            nat = self.nat
            p = ctypes.c_void_p()
            offs, cnts = (ctypes.c_int64 * nat.NUM_SEGMENTS)(), (ctypes.c_int64 * nat.NUM_SEGMENTS)()
            assert self.sf._lib.gingr_fitter_exchange(self.sf.handle, ctypes.byref(p), offs, cnts) == 0
            assert cnts[1] >= self.rp * self.rp + self.rp + 8
            self.seg1 = sharded.as_torch(p.value + 8 * offs[1], cnts[1], self.ctx.device)
        return self.seg1

    def copy_out(self):
        """(G [r r], rhs [r]) of the segment as it stands; the padding up to rp must be zero (the basis is zero padded) unless the system is
        not finite (0 x NaN)"""
        r, rp = self.r, self.rp
        self.ctx.synchronize()
        h = self.segment1().cpu().numpy()
        G, rhs = h[: rp * rp].reshape(rp, rp), h[rp * rp: rp * rp + rp]
        if np.isfinite(G[:r, :r]).all() and np.isfinite(rhs[:r]).all():
            assert not G[r:, :].any() and not G[:, r:].any() and not rhs[r:].any(), "padding of the system is not zero"
        return G[:r, :r].copy(), rhs[:r].copy()

    def _reduce(self, _user, seg, _ptr, _count):
        try:
            if int(seg) == 1:
                self.captured = self.copy_out()
            return 0
        except BaseException as e:  # must not propagate through the C frame
            self.cb_error = e
            return 1

    def ok(self, rc, what):
        from gingr_amd.api import _check
        _check(self.ctx.handle, rc, what)

    def set_lists(self, li):
        nat = self.nat
        p, x, c = (np.ascontiguousarray(li.pair_pids, dtype=np.int32), np.ascontiguousarray(li.pair_points), np.ascontiguousarray(li.pair_covs))
        k = p.shape[0]
        self.ok(self.sf._lib.gingr_fitter_set_pairs_cov(self.sf.handle, k, nat.iptr(p) if k else None, nat.dptr(x) if k else None,
                                                        nat.dptr(c) if k else None), "set_pairs_cov")
        self.set_landmarks(li.lm_pids, li.lm_points, li.lm_covs)

    def set_landmarks(self, pids, points, covs):
        nat = self.nat
        p, x, c = np.ascontiguousarray(pids, dtype=np.int32), np.ascontiguousarray(points), np.ascontiguousarray(covs)
        n = p.shape[0]
        self.ok(self.sf._lib.gingr_fitter_set_landmarks(self.sf.handle, n, nat.iptr(p) if n else None, nat.dptr(x) if n else None,
                                                        nat.dptr(c) if n else None), "set_landmarks")

    def set_state(self, pose, alpha=None, sigma2=2.0, iteration=1):
        euler, t, c = pose
        self.alpha0 = np.zeros(self.r) if alpha is None else np.asarray(alpha, dtype=np.float64)
        self.sf.set_state(self.alpha0, sigma2, euler=euler, center=c, translation=t, iteration=iteration)

    def update_args(self, flavour):
        ip = self.nat.IcpParams(1.0, 0.5, 100)
        return (self.sf.handle, flavour, None, ctypes.byref(ip) if flavour == ICP else None, 1, None), ip

    def update(self, flavour=PAIRS):
        """one update with the capture callback -> ((G, rhs), alpha, status)"""
        self.captured = None
        args, _keep = self.update_args(flavour)
        rc = self.sf._lib.gingr_fitter_update_sharded_async(*args, self.cb, None)
        if self.cb_error is not None:
            raise self.cb_error
        assert rc == 0 and self.captured is not None, rc
        alpha, s, _ = self.sf.get_state()
        return self.captured, alpha, int(s.status)

    def close(self):
        self.sf.close()


def judge(tag, name, got, ref, figures, r, failures):
    """print and record deviation | float64 figure | bound for G and rhs, and G's asymmetry against twice the bound"""
    dG, dr = lc.deviation(got, ref)
    bG, br = lc.bounds_of(figures, r)
    asym = float(np.abs(got[0] - got[0].T).max() / float(ref[2].max()))
    print("    %-10s %-34s G %.2e | %.2e | %.2e   rhs %.2e | %.2e | %.2e   asym %.2e" % (tag, name, dG, figures[0], bG, dr, figures[1], br, asym))
    if not dG <= bG:
        failures.append((tag, name, "G", dG, bG))
    if not dr <= br:
        failures.append((tag, name, "rhs", dr, br))
    if not asym <= 2.0 * bG:
        failures.append((tag, name, "asymmetry", asym, 2.0 * bG))


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", [c.name for c in lc.CASES])
def test_system_element_by_element(ctx, name):
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    lc.check_guard(case, li)
    ref, _, figures = lc.reference_of(name)
    cap = Capture(ctx, case.r)
    failures = []
    try:
        cap.set_state(case.pose, alpha=np.random.default_rng(case.r).normal(0, 0.1, case.r))   # (the system does not depend on alpha)
        cap.set_lists(li)
        got, alpha, status = cap.update()
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), name
        judge("pairs", name, got, ref, figures, case.r, failures)
        assert status == 0 and np.isfinite(alpha).all() and not np.array_equal(alpha, cap.alpha0), (name, status)
    finally:
        cap.close()
    assert not failures, failures


def test_nothing_observed_leaves_a_zero_system(ctx):
    """the pairs flavour without any pair: G = 0, rhs = 0 exactly -- what lets the cases above read the kernel's sums alone"""
    cap = Capture(ctx, 24)
    try:
        cap.set_state(lc.SKEW)
        (G, rhs), _, status = cap.update()
        assert status == 0 and not G.any() and not rhs.any()
    finally:
        cap.close()


@pytest.mark.parametrize("name", lc.SHORT_LANDMARK_CASES)
def test_landmarks_in_the_icp_flavour(ctx, name):
    """Point-cloud ICP: the dense part is captured without the list and subtracted.  With the list the landmarks' vertices drop out of
    the dense part (lm_mask), so the difference is the list's terms minus those vertices' own: weight 1 / sigma2 towards their closest
    target point -- the target is the posed mean shape, vertex by vertex, so that this point is known without a search."""
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    parts = lc.model_parts(case.r)
    sigma2 = 1.0e6
    target = lc.posed_point(parts, case.pose, np.arange(lc.M_POINTS))
    d = np.linalg.norm(target[:, None, :] - target[None, :, :], axis=2) + 1e9 * np.eye(lc.M_POINTS)
    assert d.min() > 1.0                                                        # every vertex's closest target point is its own
    ref, _, figures = lc.reference_of(name)
    own = lc.reference(parts, case.pose, li.lm_pids, target[li.lm_pids], np.tile(sigma2 * np.eye(3), (case.L, 1, 1)))
    want = (ref[0] - own[0], ref[1] - own[1], ref[2] + own[2], ref[3] + own[3])
    cap = Capture(ctx, case.r, target=target)
    failures = []
    try:
        cap.set_state(case.pose, sigma2=sigma2)
        (G0, rhs0), _, _ = cap.update(ICP)
        cap.set_state(case.pose, sigma2=sigma2)
        cap.set_landmarks(li.lm_pids, li.lm_points, li.lm_covs)
        (G1, rhs1), _, status = cap.update(ICP)
        # the dense part is there, and no larger than the list's own terms: its rounding, which the subtraction leaves behind, is of
        # order 2^-53 of it and far inside any bound
        assert status == 0 and 0 < np.abs(G0).max() < float(ref[2].max()), (np.abs(G0).max(), float(ref[2].max()))
        judge("icp", name, (G1 - G0, rhs1 - rhs0), want, figures, case.r, failures)
    finally:
        cap.close()
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- row shards
class CapturingSum(HostSum):
    """HostSum that keeps every shard's partial segment 1 as it was before the sum, and the total after it"""

    def __init__(self, shards):
        super().__init__(shards)
        self.partials = [None] * len(shards)
        self.total = None

    def _reduce(self, r, _user, seg, _ptr, _count):
        try:
            if int(seg) == 1:
                self.shards[r].ctx.synchronize()
                self.partials[r] = self.shards[r].sf._segment(1).cpu().numpy().copy()
        except BaseException as e:  # must not propagate through the C frame
            self.errors.append(e)
            self.barrier.abort()
            return 1
        rc = super()._reduce(r, _user, seg, _ptr, _count)
        if rc == 0 and int(seg) == 1 and r == 0:
            self.total = self.shards[0].sf._segment(1).cpu().numpy().copy()
        return rc


def test_two_row_shards_in_one_process():
    """L = 257 covariance pairs alternating between the rows of two shards: each shard's partial is the reference restricted to its rows
    (the other shard's entries are rows -1 in the middle of both chunks), and the two sum to the whole."""
    import torch
    import gingr_amd as ga
    from gingr_amd.sharded import shard_rows
    r, L, world = 24, 257, 2
    rp = pc.rp_of(r)
    parts = lc.model_parts(r)
    rng = np.random.default_rng(5)
    ranges = [shard_rows(lc.M_POINTS, world, k) for k in range(world)]
    pids = np.array([rng.integers(*ranges[k % 2]) for k in range(L)], dtype=np.int64)
    assert np.unique(pids).shape[0] < L
    covs = lc.covariances("well", L, 99)
    points = lc.posed_point(parts, lc.SKEW, pids) + rng.normal(0, 2.0, (L, 3))
    li = lc.Lists(pids, points, covs, pids[:0], points[:0], covs[:0], pids, points, covs)
    ctxs = [ga.Context(0) for _ in range(world)]
    shards = [Capture(ctxs[k], r, rank=k, world=world) for k in range(world)]
    failures = []
    try:
        mom = None
        for f in shards:                                                       # the model's moments, summed once (tests/test_gpu_group.py)
            g = f.sf.gram_tensor()
            f.ctx.synchronize()
            mom = g.clone() if mom is None else mom + g
        for f in shards:
            f.sf.gram_tensor().copy_(mom)
            torch.cuda.synchronize()
            f.sf.finish_setup()
            f.set_state(lc.SKEW)
            f.set_lists(li)
        hs = CapturingSum(shards)
        keep = [f.update_args(PAIRS) for f in shards]
        rcs = hs.run(lambda k, cb: shards[k].sf._lib.gingr_fitter_update_sharded_async(*keep[k][0], cb, None))
        assert rcs == [0] * world

        def split(h):
            G, rhs = h[: rp * rp].reshape(rp, rp), h[rp * rp: rp * rp + rp]
            assert not G[r:, :].any() and not G[:, r:].any() and not rhs[r:].any()
            return G[:r, :r], rhs[:r]

        for k, (b, e) in enumerate(ranges):
            rows = np.where((pids >= b) & (pids < e), pids, -1)
            assert (rows[:lc.K_CHUNK] < 0).sum() > 100 and rows[lc.K_CHUNK] == (pids[lc.K_CHUNK] if k == 0 else -1)
            ref = lc.reference(parts, lc.SKEW, rows, points, covs)
            fig = lc.deviation(lc.reference(parts, lc.SKEW, rows, points, covs, dtype=np.float64), ref)
            judge("shard", f"rows [{b}, {e}) of L257-well-skew", split(hs.partials[k]), ref, fig, r, failures)
        ref = lc.reference(parts, lc.SKEW, pids, points, covs)
        fig = lc.deviation(lc.reference(parts, lc.SKEW, pids, points, covs, dtype=np.float64), ref)
        judge("shard", "sum of the two partials", split(hs.total), ref, fig, r, failures)
        assert all(f.sf.get_state()[1].status == 0 for f in shards)
    finally:
        for f in shards:
            f.close()
        for c in ctxs:
            c.close()
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- user-visible
def test_posterior_mean_of_three_needle_landmarks(ctx):
    """DeviceModel.posterior_mean (gingr_model_posterior_mean -> model_observation_system) with zero dense weights: the coefficients
    against the extended-precision solve of (I + G_ref) a = rhs_ref, at 1 000 x the error the float64 route leaves in a."""
    import gingr_amd as ga
    name = "r264-L3-needle-skew"
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    ref, f64, _ = lc.reference_of(name)
    r = case.r

    def solve(G, rhs, dtype, chol):
        Lc = chol(np.eye(r, dtype=dtype) + 0.5 * (G + G.T))
        return pc.backward_sub_t(Lc, pc.forward_sub(Lc, rhs))

    a_ref = solve(ref[0], ref[1], lc.LD, pc.cholesky_left)
    a_64 = solve(f64[0], f64[1], np.float64, np.linalg.cholesky)
    norm = lambda v: float(np.sqrt(np.sum(np.asarray(v, dtype=lc.LD) ** 2)))
    figure = norm(a_64.astype(lc.LD) - a_ref) / norm(a_ref)
    rf, mean, U, lam = (np.array(a) for a in lc.model_parts(r))
    dm = ga.DeviceModel(ctx, ga.PointDistributionModel(rf, mean, U, lam))
    try:
        euler, t, c = case.pose
        lm = ga.LandmarkCorrespondences(li.lm_pids.astype(np.int32), np.array(li.lm_points), np.array(li.lm_covs))
        mesh, a = dm.posterior_mean(np.zeros((lc.M_POINTS, 3)), np.zeros(lc.M_POINTS), euler=euler, center=c, translation=t, landmarks=lm)
    finally:
        dm.close()
    dev = norm(a.astype(lc.LD) - a_ref) / norm(a_ref)
    print(f"    posterior_mean {name}: a dev {dev:.2e} | float64 {figure:.2e} | bound {1000 * figure:.2e}")
    assert figure > 0 and np.isfinite(mesh).all() and dev <= 1000.0 * figure, (dev, figure)


def test_template_plugin_with_one_covariance_per_vertex(ctx):
    """getUncertainty returning K = 300 matrices of shape (3, 3), none a multiple of the identity: two chunks of the covariance list
    arrive (this shows no more than that; the element-wise cases above carry the accuracy)."""
    import gingr_amd as ga
    r = 24
    ref, mean, U, lam = (np.array(a) for a in lc.model_parts(r))
    mo = go.PDM(ref, mean, U, lam)
    rng = np.random.default_rng(12)
    K = lc.M_POINTS
    assert K > lc.K_CHUNK
    pids = rng.permutation(K).astype(np.int64)
    truth = mo.instance(rng.normal(0, 0.6, r)) + np.array([2.0, -1.0, 1.5])
    pts = truth[pids] + rng.normal(0, 0.5, (K, 3))
    covs = np.array(lc.covariances("well", K, 7))
    pairs = ga.CorrespondencePairs(pids, pts)
    algo, state = template_state(ctx, mo, truth + 1.0, lambda s: pairs, lambda p, s: covs)
    try:
        st = oracle_state_of(state.general, 1)
        s1 = algo.update(state)
        want = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2,
                                           landmarks=go.Landmarks(pids, pts, covs))
        print(f"    template, K = {K} covariances: rel(fit) {rel(s1.general.fit, want.fit):.3e}")
        assert s1.general.status == want.status == 0 and rel(s1.general.fit, want.fit) < 1e-5
        assert rel(s1.general.fit, st.fit) > 1e-4
    finally:
        algo.close()


# ---------------------------------------------------------------------------------------------------------------- no covariance
NOT_A_COVARIANCE = {
    "rank 2": np.array([[1.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 1.0]]),       # exactly singular: (1,1,0)(1,1,0)^T + (0,1,1)(0,1,1)^T
    "indefinite": np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),   # eigenvalues 3, -1, 1
    # eigenvalues 1001, -999, 1: a negative weight so small that I + G stays positive definite -- the inverse of any non-singular matrix
    # (the reference's route, and the cofactor formula) gives a finite posterior here; asserted below on the float64 route
    "indefinite, weak": np.array([[1.0, 1000.0, 0.0], [1000.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
    "nan": np.array([[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]]),
}


def test_a_matrix_that_is_no_covariance_fails_the_update(ctx):
    """Rank 2, indefinite, NaN -- as a covariance pair and as a landmark: the posterior fails by the reference's rule for a failed
    posterior (deterministic update after iteration 0: ModelFlexibilityError, state unchanged), nothing finite is committed, and the same
    handle gives the right system for a good list afterwards.  A NaN weight is ordinary arithmetic on the device.  (The cofactor formula
    left a finite G for the indefinite matrices: measured on the parent commit's kernel.)"""
    import gingr_amd as ga
    name = "r24-L3-well-skew"
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    ref, _, figures = lc.reference_of(name)
    alpha0 = np.random.default_rng(3).normal(0, 0.3, case.r)
    cap = Capture(ctx, case.r)
    failures = []
    try:
        for what, C in NOT_A_COVARIANCE.items():
            covs = np.array(li.lm_covs)
            covs[1] = C
            if what == "indefinite, weak":
                G64 = lc.reference(lc.model_parts(case.r), case.pose, li.rows, li.points, covs, dtype=np.float64)[0]
                assert np.linalg.eigvalsh(np.eye(case.r) + 0.5 * (G64 + G64.T)).min() > 0.5
            for route in ("pair", "landmark"):
                cap.set_state(case.pose, alpha=alpha0)
                if route == "pair":
                    bad = lc.Lists(li.lm_pids, li.lm_points, covs, li.lm_pids[:0], li.lm_points[:0], covs[:0], li.rows, li.points, covs)
                else:
                    bad = lc.Lists(li.lm_pids[:0], li.lm_points[:0], covs[:0], li.lm_pids, li.lm_points, covs, li.rows, li.points, covs)
                cap.set_lists(bad)
                (G, rhs), alpha, status = cap.update()
                print(f"    {what} as a {route}: status {status}, finite G {bool(np.isfinite(G).all())}")
                assert status == go.STATUS_MODEL_FLEXIBILITY_ERROR and np.array_equal(alpha, alpha0), (what, route, status)
                assert not np.isfinite(G).all(), (what, route)
        cap.set_state(case.pose, alpha=alpha0)
        cap.set_lists(li)
        got, alpha, status = cap.update()
        judge("after", name, got, ref, figures, case.r, failures)
        assert status == 0 and np.isfinite(alpha).all() and not np.array_equal(alpha, alpha0)
        # the stateless entry reports it through its return code
        rf, mean, U, lam = (np.array(a) for a in lc.model_parts(case.r))
        dm = ga.DeviceModel(ctx, ga.PointDistributionModel(rf, mean, U, lam))
        try:
            covs = np.array(li.lm_covs)
            covs[1] = NOT_A_COVARIANCE["rank 2"]
            lm = ga.LandmarkCorrespondences(li.lm_pids.astype(np.int32), np.array(li.lm_points), covs)
            with pytest.raises(ga.GingrNativeError):
                dm.posterior_mean(np.zeros((lc.M_POINTS, 3)), np.zeros(lc.M_POINTS), landmarks=lm)
        finally:
            dm.close()
    finally:
        cap.close()
    assert not failures, failures
