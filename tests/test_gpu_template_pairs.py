"""GPU tests of the "pairs given" flavour of the fitter (gingr_amd/csrc/fitter_pairs.hip, flavour 3 of run_phase) and of
TemplateRegistration on top of it: correspondences and uncertainties come from the caller, everything `update` does around the
posterior runs on the device.

References and bounds -- every bound is the one the sibling flavour's test holds against the same oracle function:
  one update          go.update_from_observations          rel(fit) < 1e-5                  tests/test_gpu_surface_icp.py:264
  sampled update      the same, with z                      rel(fit) < 1e-5                  tests/test_gpu_probabilistic.py:144
  transition density  go.posterior_logpdf_of_mesh           |got - want| < 1e-5 |want|       tests/test_gpu_probabilistic.py:147
  covariance maps     PDM.posterior_model, two CPU routes   spread <= 1e-13, err <= 1000 x   tests/test_gpu_posterior_covariance.py:63-64
  posterior model     the same                              spread <= 1e-13, err <= 1000 x   tests/test_gpu_posterior_model.py:58-59
  shards              the single shard's fit                rel(fit) < 1e-9                  tests/test_gpu_group.py:545
  memo / shard density  the value computed from scratch     |got - want| <= 1e-9 |want|      tests/test_gpu_probabilistic.py:238
The consolidation is compared with a plain numpy loop that adds in the same order: the weights must be equal bit for bit, the observed
points agree to 4e-16 relative (one more division than the loop's quotient can differ by: the kernel and the loop divide the same sums).
Models: go.build_gaussian_gpmm(ref, 60, 20, rel_tol=1e-9, max_rank=r) on a sub-sample of the femur fixture (600 vertices), ranks 24 and
136 -- the narrow and the wide family of the Gram pass."""
import ctypes
import functools
import threading

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests.test_gpu_posterior_covariance import check, ga_model, mats, model_of, posterior_routes, three_landmarks
from tests.test_gpu_posterior_model import check_model, state_routes
from tests.test_gpu_surface_icp import femur, oracle_state_of, rel

pytestmark = pytest.mark.gpu

M_FEMUR = 600
EULER, TRANSLATION = (0.02, -0.03, 0.01), (1.0, -2.0, 0.5)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def femur_case(rank):
    """(oracle model over 600 femur vertices, 800 target vertices)"""
    ref, _, target, _ = femur()
    ref = np.ascontiguousarray(ref[::2][:M_FEMUR])
    return go.build_gaussian_gpmm(ref, 60.0, 20.0, rel_tol=1e-9, max_rank=rank), np.ascontiguousarray(target[::2][:800])


@functools.lru_cache(maxsize=None)
def pair_lists(rank, seed=5):
    """Repeated, shuffled pids over two thirds of the vertices (vertex M - 1 among them), variances over four decades."""
    mo, target = femur_case(rank)
    rng = np.random.default_rng(seed)
    M = mo.M
    seen = np.concatenate([rng.permutation(M - 1)[: 2 * M // 3 - 1], [M - 1]])
    pids = np.concatenate([seen, rng.choice(seen, 300)])
    pids = pids[rng.permutation(pids.shape[0])]
    truth = mo.instance(rng.normal(0, 0.6, mo.rank)) @ go.euler_to_rot(0.05, -0.04, 0.03).T + np.array([2.0, -1.0, 1.5])
    var = 10.0 ** rng.uniform(-2, 2, pids.shape[0])
    pts = truth[pids] + rng.normal(0, 1, (pids.shape[0], 3)) * np.minimum(np.sqrt(var), 2.0)[:, None]
    return pids.astype(np.int64), np.ascontiguousarray(pts), var


def oracle_state(mo, alpha, sigma2, iteration=0, transform=1, step=1.0, euler=EULER, translation=TRANSLATION):
    st = go.State(alpha=np.asarray(alpha, dtype=np.float64).copy(), euler=tuple(euler), center=np.zeros(3),
                  translation=np.asarray(translation, dtype=np.float64), scale=1.0, sigma2=float(sigma2), fit=np.zeros((mo.M, 3)),
                  iteration=iteration, global_transformation=transform, step_length=step)
    st.fit = go.model_instance_shape_pose_scale(mo, st)
    return st


class Raw:
    """One fitter behind the C ABI (a single shard unless world > 1)."""

    def __init__(self, ctx, mo, target, transform=1, step=1.0, rank=0, world=1, defer=False):
        from gingr_amd.sharded import ShardedFitter
        self.sf = ShardedFitter(ctx, ga_model(mo), target, rank=rank, world=world, all_reduce=(lambda t: None) if world > 1 else None,
                                global_transform=transform, step_length=step, defer_setup=defer)
        self.ctx, self.mo = ctx, mo

    @property
    def lib(self):
        return self.sf._lib

    @property
    def h(self):
        return self.sf.handle

    def ok(self, rc, what):
        from gingr_amd.api import _check
        _check(self.ctx.handle, rc, what)

    def set_state(self, st):
        self.sf.set_state(st.alpha, st.sigma2, euler=st.euler, center=st.center, translation=st.translation, scale=st.scale,
                          iteration=st.iteration, status=st.status)

    def set_pairs(self, pids, pts, var):
        from gingr_amd._native import dptr, iptr
        p, x, v = np.ascontiguousarray(pids, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
        k = p.shape[0]
        self.ok(self.lib.gingr_fitter_set_pairs(self.h, k, iptr(p) if k else None, dptr(x) if k else None, dptr(v) if k else None), "set_pairs")

    def set_pairs_cov(self, pids, pts, covs):
        from gingr_amd._native import dptr, iptr
        p, x, c = np.ascontiguousarray(pids, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(covs, dtype=np.float64)
        k = p.shape[0]
        self.ok(self.lib.gingr_fitter_set_pairs_cov(self.h, k, iptr(p) if k else None, dptr(x) if k else None, dptr(c) if k else None), "set_pairs_cov")

    def planes(self):
        from gingr_amd._native import dptr
        M = self.sf.end - self.sf.begin
        obs, w = np.empty((M, 3)), np.empty(M)
        self.ok(self.lib.gingr_fitter_get_pair_observations(self.h, dptr(obs), dptr(w)), "get_pair_observations")
        return obs, w

    def update(self, z=None):
        from gingr_amd._native import dptr
        if z is None:
            self.ok(self.lib.gingr_fitter_update_pairs_async(self.h, 1), "update_pairs_async")
        else:
            zz = np.ascontiguousarray(z, dtype=np.float64)
            self.ok(self.lib.gingr_fitter_update_pairs_sample_async(self.h, dptr(zz)), "update_pairs_sample_async")
        return self.sf.get_state()

    def logpdf(self, mesh):
        from gingr_amd._native import dptr
        m = np.ascontiguousarray(mesh, dtype=np.float64)
        out = ctypes.c_double()
        self.ok(self.lib.gingr_fitter_posterior_logpdf_pairs(self.h, dptr(m), ctypes.byref(out)), "posterior_logpdf_pairs")
        return out.value

    def retry(self):
        v = ctypes.c_int32()
        self.ok(self.lib.gingr_fitter_retry_counter(self.h, -1, ctypes.byref(v)), "retry_counter")
        return v.value

    def close(self):
        self.sf.close()


# ---------------------------------------------------------------------------------------------------------------- 1. consolidation
def loop_consolidation(M, pids, pts, var):
    """the definition: per vertex, in ascending pair position"""
    w, s = np.zeros(M), np.zeros((M, 3))
    for k in range(pids.shape[0]):
        i = pids[k]
        w[i] += 1.0 / var[k]
        s[i] += pts[k] / var[k]
    obs = np.zeros((M, 3))
    has = w != 0.0
    obs[has] = s[has] / w[has][:, None]
    return obs, w


def consolidation_pids(M, K, layout, rng):
    if K == 0:
        return np.zeros(0, dtype=np.int64)
    if layout == "one-vertex":
        return np.full(K, M // 2, dtype=np.int64)
    seen = np.concatenate([rng.permutation(M - 1)[: max((M - 1) // 2, 0)], [M - 1]])      # about half the vertices have no pair
    pids = rng.choice(seen, K)
    pids[0] = M - 1                                                                       # the last vertex is observed
    if K >= 600:
        pids[rng.permutation(K)[:300]] = seen[0]                                          # one vertex with (at least) 300 pairs
    return pids[rng.permutation(K)].astype(np.int64)


@pytest.mark.parametrize("M", [1, 255, 257, 600])
def test_consolidation_equals_the_numpy_loop(ctx, M):
    mo = model_of(M, 5)
    raw = Raw(ctx, mo, mo.ref + 1.0)
    try:
        # (descending K last-but-one, then a longer list again: the working memory is reused, then grown)
        for K, layout in [(3 * M + 5, "mixed"), (1, "mixed"), (0, "mixed"), (M, "mixed"), (3 * M + 5, "one-vertex"), (4 * M + 9, "mixed")]:
            rng = np.random.default_rng(1000 * M + K + len(layout))
            pids = consolidation_pids(M, K, layout, rng)
            pts = rng.normal(0, 30, (K, 3))
            var = 10.0 ** rng.uniform(-2, 2, K)
            raw.set_pairs(pids, pts, var)
            obs, w = raw.planes()
            want_obs, want_w = loop_consolidation(M, pids, pts, var)
            err = float(np.abs(obs - want_obs).max() / max(np.abs(want_obs).max(), 1e-300)) if K else 0.0
            per = np.abs(obs - want_obs) / np.maximum(np.abs(want_obs), 1e-300)
            print(f"M={M} K={K} {layout}: weights equal {np.array_equal(w, want_w)}, obs rel err max {float(per.max()):.3e} (overall {err:.3e})")
            assert np.array_equal(w, want_w), (M, K, layout)
            assert (np.abs(obs - want_obs) <= 4e-16 * np.abs(want_obs)).all(), (M, K, layout, float(per.max()))
            if K >= 600 and layout == "mixed":
                assert np.bincount(pids).max() >= 300 and (want_w == 0).any() and want_w[M - 1] > 0
        with pytest.raises(Exception) as e:                                    # a pid outside the model, checked on the host
            raw.set_pairs([0, M], np.zeros((2, 3)), np.ones(2))
        assert getattr(e.value, "code", None) == 1                            # GINGR_ERR_BAD_ARGUMENT
        obs2, w2 = raw.planes()
        assert np.array_equal(w2, w) and np.array_equal(obs2, obs)            # ... and nothing was changed
    finally:
        raw.close()


# ---------------------------------------------------------------------------------------------------------------- 2. one update
@pytest.mark.parametrize("step", [1.0, 0.5])
@pytest.mark.parametrize("transform", [0, 1, 2])
@pytest.mark.parametrize("rank", [24, 136])
def test_one_update_against_the_oracle(ctx, rank, transform, step):
    mo, target = femur_case(rank)
    pids, pts, var = pair_lists(rank)
    assert np.bincount(pids).max() > 1 and np.unique(pids).shape[0] <= 2 * mo.M // 3 and var.max() / var.min() > 1e3
    alpha0 = np.random.default_rng(rank).normal(0, 0.3, mo.rank)
    st = oracle_state(mo, alpha0, 3.0, iteration=2, transform=transform, step=step)
    raw = Raw(ctx, mo, target, transform, step)
    try:
        raw.set_state(st)
        raw.set_pairs(pids, pts, var)
        alpha, sc, fit = raw.update()
        want = go.update_from_observations(mo, st, pids, pts, var, st.sigma2)
        print(f"rank {rank} transform {transform} step {step}: rel(fit) {rel(fit, want.fit):.3e}")
        assert sc.status == want.status == 0 and sc.iteration == want.iteration == 3
        assert rel(fit, want.fit) < 1e-5, rel(fit, want.fit)
        assert sc.sigma2 == 3.0                                                # the trait's default updateSigma2: unchanged
        assert rel(fit, st.fit) > 1e-4                                         # (the update moved the shape)
    finally:
        raw.close()


# ---------------------------------------------------------------------------------------------------------------- 3. probabilistic
@pytest.mark.parametrize("rank", [24, 136])
def test_sampled_update_and_transition_density(ctx, rank):
    mo, target = femur_case(rank)
    pids, pts, var = pair_lists(rank)
    st = oracle_state(mo, np.random.default_rng(rank + 1).normal(0, 0.3, mo.rank), 2.0, iteration=1)
    z = np.random.default_rng(11).standard_normal(mo.rank)
    raw = Raw(ctx, mo, target)
    try:
        raw.set_state(st)
        raw.set_pairs(pids, pts, var)
        got = raw.logpdf(st.fit)
        want = go.posterior_logpdf_of_mesh(mo, st, pids, pts, var, mesh=st.fit)
        print(f"rank {rank}: logpdf {got!r} oracle {want!r}")
        assert np.isfinite(got) and abs(got - want) < 1e-5 * abs(want), (got, want)
        alpha, sc, fit = raw.update(z)                                         # (the memo of the query serves the proposal)
        st2 = go.update_from_observations(mo, st, pids, pts, var, st.sigma2, None, z)
        mean = go.update_from_observations(mo, st, pids, pts, var, st.sigma2)
        print(f"rank {rank}: sampled rel(fit) {rel(fit, st2.fit):.3e}, distance from the mean proposal {rel(st2.fit, mean.fit):.3e}")
        assert sc.status == st2.status == 0 and rel(fit, st2.fit) < 1e-5
        assert rel(st2.fit, mean.fit) > 1e-6
    finally:
        raw.close()


# ---------------------------------------------------------------------------------------------------------------- 4 / 5. TemplateRegistration
def template_state(ctx, mo, target, getCorrespondence=None, getUncertainty=None, updateSigma2=None, landmarks=None, use_lm=True,
                   sigma2=2.0, iters=1, transform=1):
    import gingr_amd as ga
    algo = ga.TemplateRegistration(ctx, getCorrespondence, getUncertainty, updateSigma2)
    lm = None if landmarks is None else ga.LandmarkCorrespondences(landmarks.pids.astype(np.int32), landmarks.points, landmarks.covs)
    cfg = ga.TemplateConfiguration(maxIterations=iters, useLandmarkCorrespondence=use_lm)
    state = algo.createInitialState(ga_model(mo), target, cfg, transform=transform, landmarks=lm, initial_pose=(EULER, TRANSLATION), sigma2=sigma2)
    return algo, state


def test_landmarks_override_their_pairs_or_not(ctx):
    import gingr_amd as ga
    mo, target = femur_case(24)
    pids, pts, var = pair_lists(24)
    lm = three_landmarks(mo, target)
    assert np.isin(lm.pids, pids).any()                                        # a landmark sits on a vertex that has pairs
    pairs = ga.CorrespondencePairs(pids, pts)
    for use_lm in (True, False):
        algo, state = template_state(ctx, mo, target, lambda s: pairs, lambda p, s: var, landmarks=lm, use_lm=use_lm)
        try:
            st = oracle_state_of(state.general, 1)
            s1 = algo.update(state)
            want = go.update_from_observations(mo, st, pids, pts, var, st.sigma2, lm if use_lm else None)
            other = go.update_from_observations(mo, st, pids, pts, var, st.sigma2, None if use_lm else lm)
            print(f"useLandmarkCorrespondence={use_lm}: rel(fit) {rel(s1.general.fit, want.fit):.3e}; the other answer is {rel(other.fit, want.fit):.3e} away")
            assert s1.general.status == want.status == 0 and rel(s1.general.fit, want.fit) < 1e-5
            assert rel(other.fit, want.fit) > 1e-4                             # (the two settings are told apart by the bound)
        finally:
            algo.close()
    # landmarks only: the reference's default getCorrespondence (no pairs) = the oracle with empty lists
    algo, state = template_state(ctx, mo, target, landmarks=lm)
    try:
        st = oracle_state_of(state.general, 1)
        s1 = algo.update(state)
        want = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2, lm)
        print(f"landmarks only: rel(fit) {rel(s1.general.fit, want.fit):.3e}")
        assert s1.general.status == want.status == 0 and rel(s1.general.fit, want.fit) < 1e-5
        assert rel(s1.general.fit, st.fit) > 1e-4
    finally:
        algo.close()
    # nothing at all: G = 0, rhs = 0 -- the posterior mean is the prior mean, and the update proceeds
    algo, state = template_state(ctx, mo, target)
    try:
        st = oracle_state_of(state.general, 1)
        s1 = algo.update(state)
        want = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2)
        print(f"no observation: rel(fit) {rel(s1.general.fit, want.fit):.3e}")
        assert s1.general.status == want.status == 0 and s1.general.iteration == 1 and rel(s1.general.fit, want.fit) < 1e-5
    finally:
        algo.close()


def spd_covariances(rng, n):
    A = rng.normal(0, 1, (n, 3, 3))
    return A @ np.swapaxes(A, 1, 2) + np.diag([0.2, 1.0, 3.0])[None]


@pytest.mark.parametrize("rank", [24, 136])
def test_covariance_pairs(ctx, rank):
    import gingr_amd as ga
    mo, target = femur_case(rank)
    rng = np.random.default_rng(3)
    base = rng.permutation(mo.M)[:35]
    cp = np.concatenate([base, rng.choice(base, 15)])[rng.permutation(50)].astype(np.int64)      # 50 repeated, unordered pids
    truth = mo.instance(rng.normal(0, 0.6, mo.rank)) + np.array([2.0, -1.0, 1.5])
    cx = truth[cp] + rng.normal(0, 0.5, (50, 3))
    cc = spd_covariances(rng, 50)
    st = oracle_state(mo, rng.normal(0, 0.2, mo.rank), 2.0, iteration=1)
    raw = Raw(ctx, mo, target)
    try:
        raw.set_state(st)
        raw.set_pairs_cov(cp, cx, cc)
        alpha, sc, fit = raw.update()
        want = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2,
                                           landmarks=go.Landmarks(cp, cx, cc))
        print(f"rank {rank} covariance pairs: rel(fit) {rel(fit, want.fit):.3e}")
        assert sc.status == want.status == 0 and rel(fit, want.fit) < 1e-5
        assert rel(fit, st.fit) > 1e-4
        # K = 0 clears the list: the next update is the one without observations
        raw.set_state(st)
        raw.set_pairs_cov([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        _, sc0, fit0 = raw.update()
        none = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2)
        assert sc0.status == 0 and rel(fit0, none.fit) < 1e-5
    finally:
        raw.close()
    # mixed, through getUncertainty's (K, 3, 3) answer: exact multiples of the identity go to the isotropic list, the rest to the
    # covariance list (vertices disjoint from the isotropic ones: the oracle's landmark argument would drop those)
    ipids, ipts, ivar = pair_lists(rank)
    keep = ~np.isin(ipids, cp)
    ipids, ipts, ivar = ipids[keep], ipts[keep], ivar[keep]
    order = np.random.default_rng(8).permutation(ipids.shape[0] + 50)
    pids = np.concatenate([ipids, cp])[order]
    pts = np.concatenate([ipts, cx])[order]
    covs = np.concatenate([ivar[:, None, None] * np.eye(3)[None], cc])[order]
    pairs = ga.CorrespondencePairs(pids, pts)
    algo, state = template_state(ctx, mo, target, lambda s: pairs, lambda p, s: covs)
    try:
        st = oracle_state_of(state.general, 1)
        s1 = algo.update(state)
        iso = order < ipids.shape[0]
        want = go.update_from_observations(mo, st, pids[iso], pts[iso], covs[iso][:, 0, 0], st.sigma2,
                                           landmarks=go.Landmarks(pids[~iso], pts[~iso], covs[~iso]))
        print(f"rank {rank} mixed lists: rel(fit) {rel(s1.general.fit, want.fit):.3e}")
        assert s1.general.status == want.status == 0 and rel(s1.general.fit, want.fit) < 1e-5
    finally:
        algo.close()


def test_a_landmark_takes_the_covariance_pairs_of_its_vertex(ctx):
    """set_landmarks after set_pairs_cov and before it: the same list, the landmark's vertex without its covariance pairs."""
    from gingr_amd._native import dptr, iptr
    mo, target = femur_case(24)
    rng = np.random.default_rng(4)
    lm = three_landmarks(mo, target)
    cp = np.concatenate([lm.pids[:2], rng.permutation(mo.M)[:10]]).astype(np.int64)
    cx = (mo.ref + mo.mean)[cp] + rng.normal(0, 2.0, (cp.shape[0], 3))
    cc = spd_covariances(rng, cp.shape[0])
    st = oracle_state(mo, np.zeros(mo.rank), 2.0, iteration=1)
    keep = ~np.isin(cp, lm.pids)
    both = go.Landmarks(np.concatenate([cp[keep], lm.pids]), np.concatenate([cx[keep], lm.points]), np.concatenate([cc[keep], lm.covs]))
    want = go.update_from_observations(mo, st, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0), st.sigma2, landmarks=both)
    lp, lx, lc = lm.pids.astype(np.int32), np.ascontiguousarray(lm.points), np.ascontiguousarray(lm.covs)
    for first in ("pairs", "landmarks"):
        raw = Raw(ctx, mo, target)
        try:
            raw.set_state(st)
            if first == "pairs":
                raw.set_pairs_cov(cp, cx, cc)
            raw.ok(raw.lib.gingr_fitter_set_landmarks(raw.h, 3, iptr(lp), dptr(lx), dptr(lc)), "set_landmarks")
            if first != "pairs":
                raw.set_pairs_cov(cp, cx, cc)
            _, sc, fit = raw.update()
            print(f"{first} first: rel(fit) {rel(fit, want.fit):.3e}")
            assert sc.status == want.status == 0 and rel(fit, want.fit) < 1e-5
        finally:
            raw.close()


# ---------------------------------------------------------------------------------------------------------------- 6. cross-checks
def test_pairs_of_the_icp_correspondence_give_the_icp_update(ctx):
    import gingr_amd as ga
    mo, target = femur_case(24)
    icp = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=30, initialSigma=20.0, endSigma=1.0, correspondenceMethod="PointcloudClosestPoint")
    s0 = icp.createInitialState(ga_model(mo), target, cfg, initial_pose=(EULER, TRANSLATION))
    pairs = icp.getCorrespondence(s0)
    assert np.array_equal(pairs.pids, np.arange(mo.M))
    want = icp.update(s0)
    algo, state = template_state(ctx, mo, target, lambda s: pairs, lambda p, s: s.general.sigma2,
                                 lambda s: max(s.general.sigma2 - cfg.sigmaStep, cfg.endSigma), sigma2=20.0)
    try:
        got = algo.update(state)
        print(f"ICP cross-check: rel(fit) {rel(got.general.fit, want.general.fit):.3e}")
        assert got.general.status == want.general.status == 0 and rel(got.general.fit, want.general.fit) < 1e-5
        assert got.general.sigma2 == want.general.sigma2
    finally:
        algo.close()
        icp.close()


def test_pairs_of_the_cpd_statistics_give_the_cpd_update(ctx):
    import gingr_amd as ga
    from gingr_amd._native import dptr
    mo, target = femur_case(24)
    cpd = ga.CpdRegistration(ctx)
    cfg = ga.CpdConfiguration(maxIterations=30, w=0.1, lambda_=1.5)
    s0 = cpd.createInitialState(ga_model(mo), target, cfg, initial_pose=(EULER, TRANSLATION))
    want = cpd.update(s0)
    P1, PX = np.empty(mo.M), np.empty((mo.M, 3))                               # the statistics that update was made from
    assert cpd._lib.gingr_fitter_get_cpd_stats(cpd._fitter, dptr(P1), dptr(PX), None, None) == 0
    assert (P1 > 0).all()
    y = np.asarray(s0.general.fit)
    pairs = ga.CorrespondencePairs(np.arange(mo.M), y + (PX / P1[:, None] - y))             # CPD.scala:44-46
    var = s0.general.sigma2 * cfg.lambda_ / P1                                              # CPD.scala:126
    algo, state = template_state(ctx, mo, target, lambda s: pairs, lambda p, s: var, sigma2=s0.general.sigma2)
    try:
        got = algo.update(state)
        print(f"CPD cross-check: rel(fit) {rel(got.general.fit, want.general.fit):.3e}")
        assert got.general.status == want.general.status == 0 and rel(got.general.fit, want.general.fit) < 1e-5
        assert got.general.sigma2 == s0.general.sigma2 != want.general.sigma2               # ... up to sigma2
    finally:
        algo.close()
        cpd.close()


# ---------------------------------------------------------------------------------------------------------------- 7. failure rules
def test_failure_rules_of_update(ctx):
    mo, target = femur_case(24)
    pids, pts, var = pair_lists(24)
    bad = pts.copy()
    bad[7, 1] = np.nan
    alpha0 = np.random.default_rng(2).normal(0, 0.3, mo.rank)
    raw = Raw(ctx, mo, target)
    try:
        raw.set_pairs(pids, bad, var)
        # iteration 0: the state stays as it is
        raw.set_state(oracle_state(mo, alpha0, 2.0, iteration=0))
        alpha, sc, fit = raw.update()
        assert sc.status == 0 and sc.iteration == 1 and np.array_equal(alpha, alpha0) and sc.sigma2 == 2.0
        # iteration 1, deterministic: ModelFlexibilityError
        st1 = oracle_state(mo, alpha0, 2.0, iteration=1)
        raw.set_state(st1)
        alpha, sc, fit = raw.update()
        assert sc.status == go.STATUS_MODEL_FLEXIBILITY_ERROR and np.array_equal(alpha, alpha0)
        # iteration 1, sampled: unchanged, one retry used up
        raw.set_state(st1)
        assert raw.retry() == 10
        alpha, sc, fit = raw.update(np.random.default_rng(0).standard_normal(mo.rank))
        assert sc.status == 0 and sc.iteration == 2 and np.array_equal(alpha, alpha0) and raw.retry() == 9
        assert rel(fit, st1.fit) < 1e-12
        # ... and the transition density of such a state cannot be computed
        with pytest.raises(Exception) as e:
            raw.logpdf(st1.fit)
        assert getattr(e.value, "code", None) in (3, 4)                       # GINGR_ERR_NONFINITE / GINGR_ERR_NOT_SPD
        # var = +inf drops a pair: the list plus one such pair far away = the list
        raw.set_state(st1)
        raw.set_pairs(pids, pts, var)
        _, sc_a, fit_a = raw.update()
        raw.set_state(st1)
        raw.set_pairs(np.concatenate([pids, [5]]), np.concatenate([pts, [[1e3, -1e3, 1e3]]]), np.concatenate([var, [np.inf]]))
        _, sc_b, fit_b = raw.update()
        assert sc_a.status == sc_b.status == 0 and np.array_equal(fit_a, fit_b)
        # a non-finite covariance fails the same way
        raw.set_pairs([], np.zeros((0, 3)), np.zeros(0))
        cc = np.tile(np.eye(3), (2, 1, 1))
        cc[1, 0, 0] = np.nan
        raw.set_pairs_cov([3, 9], (mo.ref + mo.mean)[[3, 9]], cc)
        raw.set_state(st1)
        alpha, sc, fit = raw.update()
        assert sc.status == go.STATUS_MODEL_FLEXIBILITY_ERROR and np.array_equal(alpha, alpha0)
    finally:
        raw.close()


# ---------------------------------------------------------------------------------------------------------------- 8. memo
def test_memo_is_reused_and_forgotten(ctx):
    mo, target = femur_case(24)
    pids, pts, var = pair_lists(24)
    st = oracle_state(mo, np.random.default_rng(3).normal(0, 0.3, mo.rank), 4.0, iteration=1)
    other_pts = pts + np.random.default_rng(9).normal(0, 1.5, pts.shape)
    want_a = go.posterior_logpdf_of_mesh(mo, st, pids, pts, var, mesh=st.fit)
    want_b = go.posterior_logpdf_of_mesh(mo, st, pids, other_pts, var, mesh=st.fit)
    assert abs(want_a - want_b) > 1e-3 * abs(want_a)                           # (a stale memo would be seen)
    raw = Raw(ctx, mo, target)
    fresh = Raw(ctx, mo, target)
    try:
        raw.set_state(st)
        raw.set_pairs(pids, pts, var)
        a1 = raw.logpdf(st.fit)
        # the same state again, pairs untouched: [G, rhs] and the factors left by the first query answer the second one -- another
        # route through the arithmetic, the same value to 1e-9 (tests/test_gpu_probabilistic.py:238)
        raw.set_state(st)
        a2 = raw.logpdf(st.fit)
        print(f"memo: first {a1!r}, from the memo {a2!r}")
        assert abs(a2 - a1) <= 1e-9 * abs(a1) and abs(a1 - want_a) < 1e-5 * abs(want_a)
        # other points, the same state: another posterior
        raw.set_pairs(pids, other_pts, var)
        b1 = raw.logpdf(st.fit)
        print(f"memo: {a1!r} (oracle {want_a!r}) -> other pairs {b1!r} (oracle {want_b!r})")
        assert abs(b1 - want_b) < 1e-5 * abs(want_b)
        # other covariance pairs, the same state: another posterior, too (a covariance pair does not override the isotropic pairs of
        # its vertex: only a landmark does)
        lx = (mo.ref + mo.mean)[[11]] + 3.0
        raw.set_pairs_cov([11], lx, 0.01 * np.eye(3)[None])
        c1 = raw.logpdf(st.fit)
        want_c = _logpdf_both(mo, st, pids, other_pts, var, np.array([11]), lx, 0.01 * np.eye(3)[None])
        assert abs(want_c - want_b) > 1e-3 * abs(want_b) and abs(c1 - want_c) < 1e-5 * abs(want_c), (c1, want_c, want_b)
        raw.set_pairs_cov([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        # set_sigma2 = set_state with that sigma2: the density (memo forgotten) and the next update, bit for bit
        st25 = oracle_state(mo, st.alpha, 2.5, iteration=1)
        fresh.set_state(st25)
        fresh.set_pairs(pids, other_pts, var)
        d_fresh = fresh.logpdf(st.fit)
        raw.ok(raw.lib.gingr_fitter_set_sigma2(raw.h, 2.5), "set_sigma2")
        d_raw = raw.logpdf(st.fit)
        assert d_raw == d_fresh
        al_f, sc_f, fit_f = fresh.update()
        al_r, sc_r, fit_r = raw.update()
        assert np.array_equal(fit_r, fit_f) and np.array_equal(al_r, al_f) and sc_r.sigma2 == sc_f.sigma2 == 2.5
    finally:
        raw.close()
        fresh.close()


def _logpdf_both(mo, st, pids, pts, var, cpids, cpts, ccovs):
    """go.posterior_logpdf_of_mesh for an isotropic and a covariance list that may share vertices (no override)"""
    posed = mo.transform(st.rotation(), st.translation, st.center)
    covs = np.concatenate([np.asarray(var)[:, None, None] * np.eye(3)[None], ccovs])
    post = posed.posterior_model(np.concatenate([pids, cpids]), np.concatenate([pts, cpts]), covs)
    return go.gp_logpdf(post.coefficients(st.fit))


# ---------------------------------------------------------------------------------------------------------------- 9. posterior products
@pytest.mark.parametrize("rank", [24, 136])
def test_posterior_covariance_and_model_of_a_pairs_state(ctx, rank):
    import gingr_amd as ga
    mo, target = femur_case(rank)
    pids, pts, _ = pair_lists(rank)
    var = 0.5 + 3.5 * np.random.default_rng(1).uniform(0, 1, pids.shape[0])    # (conditioning as in the siblings' cases: sigma2 of order 1)
    pairs = ga.CorrespondencePairs(pids, pts)
    algo, state = template_state(ctx, mo, target, lambda s: pairs, lambda p, s: var)
    post = None
    try:
        st = oracle_state_of(state.general, 1)
        covs = var[:, None, None] * np.eye(3)[None]
        got = algo.posteriorCovariance(state)
        a, b = posterior_routes(mo, st, pids, pts, covs)
        check(f"pairs r={rank}", mats(got), a, b)
        post = algo.posteriorModel(state)
        check_model(f"pairs r={rank}", post, state_routes(mo, st, pids, pts, covs))
        nxt = algo.update(state)                                               # the queries left state and memo usable
        want = go.update_from_observations(mo, st, pids, pts, var, st.sigma2)
        assert nxt.general.status == 0 and rel(nxt.general.fit, want.fit) < 1e-5
        lp = algo.logTransitionProbability(state, nxt)
        lp_want = go.posterior_logpdf_of_mesh(mo, st, pids, pts, var, mesh=st.fit)
        assert abs(lp - lp_want) < 1e-5 * abs(lp_want)
    finally:
        if post is not None:
            post.close()
        algo.close()


# ---------------------------------------------------------------------------------------------------------------- 10. row shards
class HostSum:
    """gingr_allreduce_fn of `world` logical shards in one process, one thread per shard: everybody waits for everybody's partial
    sums, shard 0 adds them up on the host side (torch) and hands the total to all."""

    def __init__(self, shards):
        from gingr_amd import _native as nat
        self.shards = shards
        self.barrier = threading.Barrier(len(shards), timeout=60)
        self.cbs = [nat.ALLREDUCE_FN(functools.partial(self._reduce, r)) for r in range(len(shards))]
        self.errors = []

    def _reduce(self, r, _user, seg, _ptr, _count):
        import torch
        try:
            self.shards[r].ctx.synchronize()
            self.barrier.wait()
            if r == 0:
                views = [s.sf._segment(int(seg)) for s in self.shards]
                tot = sum(v.clone() for v in views)
                for v in views:
                    v.copy_(tot)
                torch.cuda.synchronize()
            self.barrier.wait()
            return 0
        except BaseException as e:  # must not propagate through the C frame
            self.errors.append(e)
            self.barrier.abort()
            return 1

    def run(self, call):
        """call(shard index, callback) on every shard at once; the return codes"""
        rcs = [None] * len(self.shards)

        def work(r):
            rcs[r] = call(r, self.cbs[r])
        threads = [threading.Thread(target=work, args=(r,)) for r in range(len(self.shards))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not self.errors, self.errors
        return rcs


@pytest.mark.parametrize("world", [2, 3])
def test_row_shards_equal_the_single_shard(world):
    import torch
    import gingr_amd as ga
    from gingr_amd._native import dptr
    from gingr_amd.sharded import shard_rows
    mo, target = femur_case(24)
    ipids, ipts, ivar = pair_lists(24)
    # every pair on the rows of the shards 0 .. world - 2, crossing their borders: the last shard owns none
    last_begin = shard_rows(mo.M, world, world - 1)[0]
    keep = ipids < last_begin
    ipids, ipts, ivar = ipids[keep], ipts[keep], ivar[keep]
    if world == 3:
        b1 = shard_rows(mo.M, world, 1)[0]
        assert (ipids < b1).any() and (ipids >= b1).any()
    rng = np.random.default_rng(6)
    cp = rng.permutation(last_begin)[:12].astype(np.int64)
    cx = (mo.ref + mo.mean)[cp] + rng.normal(0, 2.0, (12, 3))
    cc = spd_covariances(rng, 12)
    st = oracle_state(mo, rng.normal(0, 0.3, mo.rank), 2.0, iteration=1)
    z = rng.standard_normal(mo.rank)
    c1 = ga.Context(0)
    one = Raw(c1, mo, target)
    ctxs = [ga.Context(0) for _ in range(world)]
    shards = [Raw(ctxs[r], mo, target, rank=r, world=world, defer=True) for r in range(world)]
    try:
        def load(f):
            f.set_state(st)
            f.set_pairs(ipids, ipts, ivar)
            f.set_pairs_cov(cp, cx, cc)
        load(one)
        lp1 = one.logpdf(st.fit)
        _, sc1, fit1 = one.update()
        one.set_state(st)
        _, sc1z, fit1z = one.update(z)
        mom = None
        for f in shards:                                                       # the model's moments, summed once (tests/test_gpu_group.py)
            g = f.sf.gram_tensor()
            f.ctx.synchronize()
            mom = g.clone() if mom is None else mom + g
        for f in shards:
            f.sf.gram_tensor().copy_(mom)
            torch.cuda.synchronize()
            f.sf.finish_setup()
            load(f)
        hs = HostSum(shards)
        zz = np.ascontiguousarray(z)
        mesh = np.ascontiguousarray(st.fit)
        outs = [ctypes.c_double() for _ in shards]
        rcs = hs.run(lambda r, cb: shards[r].lib.gingr_fitter_posterior_logpdf_sharded(shards[r].h, 3, None, None, dptr(mesh), cb, None,
                                                                                       ctypes.byref(outs[r])))
        assert rcs == [0] * world
        for o in outs:
            assert abs(o.value - lp1) <= 1e-9 * abs(lp1), (o.value, lp1)     # tests/test_gpu_probabilistic.py:238
        rcs = hs.run(lambda r, cb: shards[r].lib.gingr_fitter_update_sharded_async(shards[r].h, 3, None, None, 1, None, cb, None))
        assert rcs == [0] * world
        states = [f.sf.get_state() for f in shards]
        fit = np.concatenate([s[2] for s in states])
        print(f"{world} shards: rel(fit) {rel(fit, fit1):.3e}")
        assert all(s[1].status == 0 and s[1].iteration == 2 for s in states) and sc1.status == 0
        assert rel(fit, fit1) < 1e-9
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


# ---------------------------------------------------------------------------------------------------------------- 11. a run
def test_a_template_run_equals_the_oracle_loop(ctx):
    """A closest-vertex rule with distance-dependent noise and a sigma2 decay, written here: 15 updates, state by state."""
    import gingr_amd as ga
    mo, target = femur_case(24)
    tau2, decay, floor = 25.0, 0.8, 0.5
    calls = {"corr": 0, "unc": 0, "s2": 0}

    def closest(fit):
        idx, _, _ = go.icp_closest_point(np.asarray(fit), target)
        d2 = ((target[idx] - np.asarray(fit)) ** 2).sum(1)
        return idx, d2

    def corr(state):
        calls["corr"] += 1
        idx, _ = closest(state.general.fit)
        return ga.CorrespondencePairs(np.arange(mo.M), target[idx])

    def unc(pids, state):
        calls["unc"] += 1
        _, d2 = closest(state.general.fit)
        return state.general.sigma2 * (1.0 + d2 / tau2)

    def s2(state):
        calls["s2"] += 1
        return max(state.general.sigma2 * decay, floor)

    algo, state = template_state(ctx, mo, target, corr, unc, s2, sigma2=9.0, iters=16)
    try:
        seen = []
        final = algo.run(state, callBackLogger=seen.append)
        assert len(seen) == 16 and calls == {"corr": 15, "unc": 15, "s2": 15}
        assert final.general.status == ga.FittingStatuses.MaxIteration and final.general.iteration == 15
        st = oracle_state_of(state.general, 1)
        worst = 0.0
        for k in range(1, 16):
            idx, d2 = closest(st.fit)
            st = go.update_from_observations(mo, st, np.arange(mo.M), target[idx], st.sigma2 * (1.0 + d2 / tau2), max(st.sigma2 * decay, floor))
            g = seen[k].general
            worst = max(worst, rel(g.fit, st.fit))
            assert g.status == st.status == 0 and g.iteration == st.iteration == k
            assert rel(g.fit, st.fit) < 1e-5, (k, rel(g.fit, st.fit))
            assert abs(g.sigma2 - st.sigma2) < 1e-12
        print(f"15 updates: worst rel(fit) {worst:.3e}, sigma2 {st.sigma2:.4f}")
        assert st.sigma2 < 9.0 * decay ** 10                                   # the user's updateSigma2 was applied at every step
        # without a logger the run takes the same path (the callbacks run on the host every iteration)
        again = algo.run(state)
        assert np.array_equal(again.general.fit, final.general.fit) and again.general.sigma2 == final.general.sigma2
    finally:
        algo.close()
