"""GPU tests of point-to-plane ICP with its correspondence on the device (gingr_fitter_set_pairs_plane_async /
gingr_fitter_update_plane_async, gingr_amd/csrc/fitter_pairs.hip: plane_pairs_kernel, plane_schedule_kernel) and of
PointToPlaneIcpRegistration on top of them.

Planes, element-wise: xbar against gingr_fitter_get_surface_correspondence bit for bit, the rejected set against the oracle's weights,
Lambda_i per entry against the restatement in np.longdouble (tests/plane_pairs_restatement.py) within 32 u kappa_t / v_n, u = 2^-53 and
kappa_t = |e1| |e2| / |e1 x e2| of the vertex's own triangle: the plain rounding bound of cross product, normalisation and outer product
(tests/test_plane_pairs_host.py asserts kappa_t <= 1.5 on the grids and <= 22 on the femur target).  A closest point on an edge or a
corner belongs to several triangles whose distances differ in the last bits; the restatement lists them and the device's plane must be
the one of one of them.
Whole updates: the bounds of the sibling flavours -- rel(fit) < 1e-5 against the oracle (alpha and pose likewise), sigma2 of the next
state equal to the schedule's value bit for bit.
Two routes of one update on the same device -- the native call against closest points + normalTangentCovariances + the dense list, and
ratio 1 against the surface ICP -- rel(fit) < 1e-9, the bound the project holds two summation orders of one update to (row shards).  The
two routes that existed before, landmark pass against dense pass on these inputs, are measured by the same test; see ROUTE_BOUND.
Largest error / bound ratio seen on an MI355X: DESIGN.md section 4."""
import ctypes
import dataclasses
import functools
import gc

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import plane_pairs_restatement as pp
from tests.test_gpu_pairs_cov_gram import POSES, Dense, lambda_of
from tests.test_gpu_posterior_covariance import check, ga_model, mats, posterior_routes, three_landmarks
from tests.test_gpu_posterior_model import check_model, state_routes
from tests.test_gpu_surface_icp import femur, grid_mesh, oracle_state_of, rel
from tests.test_gpu_template_pairs import spd_covariances

pytestmark = pytest.mark.gpu

ERR_BAD_ARGUMENT, ERR_STATE = 1, 6
SCHEDULE = (2.0, 0.5, 10)                          # initial sigma, end sigma, max iterations: sigma2 2.0 -> 1.85 -> ...
# Two routes of one update on the same device.  The two routes the library had before this flavour -- the landmark pass against the
# dense pass, both fed the host's closest points and covariances of these very inputs -- differ by what
# test_native_call_equals_the_host_route prints as "spread": at most 1.2e-15 on an MI355X (2026-10-21; grids 4.3e-16 and 8.5e-16, femur
# 1.2e-15), far below the 1e-10 from which on the bound would have to follow the spread.
ROUTE_BOUND = 1e-9


class Plane(Dense):
    """Dense plus the meshes and the two point-to-plane entry points."""

    def __init__(self, ctx, mo, cells, target, tcells, transform=1, meshes=True):
        super().__init__(ctx, mo, target, transform=transform)
        self.cells, self.tcells = cells, tcells
        if meshes:
            self.sf.set_meshes(cells, tcells)

    @staticmethod
    def params(ratio, reject):
        from gingr_amd import _native as nat
        return nat.PlaneParams(float(ratio), int(reject))

    def plane(self, ratio, reject, expect_ok=True):
        p = self.params(ratio, reject)
        rc = self.lib.gingr_fitter_set_pairs_plane_async(self.h, ctypes.byref(p))
        if expect_ok:
            self.ok(rc, "set_pairs_plane_async")
        return rc

    def update_plane(self, ratio, reject, sched=SCHEDULE, n=1, expect_ok=True):
        from gingr_amd import _native as nat
        p, s = self.params(ratio, reject), nat.IcpParams(float(sched[0]), float(sched[1]), int(sched[2]))
        rc = self.lib.gingr_fitter_update_plane_async(self.h, ctypes.byref(p), ctypes.byref(s), int(n))
        if expect_ok:
            self.ok(rc, "update_plane_async")
            return self.sf.get_state()
        return rc

    def update_icp_surface(self, sched=SCHEDULE, n=1):
        from gingr_amd import _native as nat
        s = nat.IcpParams(float(sched[0]), float(sched[1]), int(sched[2]))
        self.ok(self.lib.gingr_fitter_update_icp_surface_async(self.h, ctypes.byref(s), int(n)), "update_icp_surface_async")
        return self.sf.get_state()

    def surface(self):
        from gingr_amd._native import dptr
        M = self.mo.M
        cp, w = np.empty((M, 3)), np.empty(M)
        self.ok(self.lib.gingr_fitter_get_surface_correspondence(self.h, dptr(cp), dptr(w)), "get_surface_correspondence")
        return cp, w

    def set_sigma2(self, s2):
        self.ok(self.lib.gingr_fitter_set_sigma2(self.h, float(s2)), "set_sigma2")

    def set_landmarks(self, lm):
        from gingr_amd._native import dptr, iptr
        lp, lx, lc = lm.pids.astype(np.int32), np.ascontiguousarray(lm.points), np.ascontiguousarray(lm.covs)
        self.ok(self.lib.gingr_fitter_set_landmarks(self.h, lp.shape[0], iptr(lp), dptr(lx), dptr(lc)), "set_landmarks")


# ---------------------------------------------------------------------------------------------------------------- inputs
TARGETS = {"grid17": (17, 40.0, 6.0, 3), "grid24": (24, 40.0, 6.0, 1)}      # 512 triangles = two triangle tiles; 1 058 triangles


@functools.lru_cache(maxsize=None)
def grid_case(n_template, target, rank):
    """(oracle model over an n x n template sheet, its cells, target vertices, target cells): the template lies over the open target and
    reaches past its rim, so the boundary rule rejects some vertices"""
    tv, tt = grid_mesh(*TARGETS[target])
    sv, sc = grid_mesh(n_template, 43.0, 5.0, 2)
    sv = sv + np.array([1.0, -0.5, 3.0])
    return go.build_gaussian_gpmm(sv, 60.0, 20.0, rel_tol=1e-9, max_rank=rank), sc, tv, tt


@functools.lru_cache(maxsize=None)
def femur_case(rank=24):
    ref, cells, target, tcells = femur()
    return go.build_gaussian_gpmm(ref, 60.0, 20.0, rel_tol=1e-9, max_rank=rank), cells, target, tcells


def pose_state(mo, pose, sigma2=2.0, seed=1, iteration=1, transform=1):
    euler, center, t = POSES[pose]
    st = go.State(alpha=np.random.default_rng(seed).normal(0, 0.2, mo.rank), euler=tuple(euler), center=np.asarray(center, dtype=np.float64),
                  translation=np.asarray(t, dtype=np.float64), scale=1.0, sigma2=sigma2, fit=np.zeros((mo.M, 3)), iteration=iteration,
                  global_transformation=transform)
    st.fit = go.model_instance_shape_pose_scale(mo, st)
    return st


def pose_vector(sc):
    return np.concatenate([list(sc.euler), list(sc.translation), [sc.scale]])


def oracle_pose_vector(st):
    return np.concatenate([list(st.euler), list(st.translation), [st.scale]])


def same_state(a, b):
    """alpha, scalars and fit of two gingr_fitter_get_state results, bit for bit"""
    (al_a, sc_a, fit_a), (al_b, sc_b, fit_b) = a, b
    return (np.array_equal(al_a, al_b) and np.array_equal(fit_a, fit_b) and bytes(sc_a) == bytes(sc_b))


def plane_errors(p6, cands, normals_ld, kap, v_n, ratio, rows):
    """per vertex of `rows`: the smallest, over the triangles its closest point belongs to, of max |Lambda - restatement| / bound"""
    L = lambda_of(p6).astype(np.longdouble)
    out = np.empty(len(rows))
    for k, i in enumerate(rows):
        want = pp.closed_form(normals_ld[cands[i]], v_n, ratio, np.longdouble)
        bound = 32 * pp.U53 * kap[cands[i]] / v_n
        out[k] = float((np.abs(want - L[i][None]).max(axis=(1, 2)) / bound).min())
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. planes
@pytest.mark.parametrize("reject", [0, 1])
@pytest.mark.parametrize("ratio", [1.0, 100.0, 1e8])
@pytest.mark.parametrize("n_template, target, rank", [(16, "grid17", 12), (17, "grid24", 30)])
def test_planes_element_wise(ctx, n_template, target, rank, ratio, reject):
    mo, cells, tv, tt = grid_case(n_template, target, rank)
    st = pose_state(mo, "posed")
    f = Plane(ctx, mo, cells, tv, tt)
    try:
        f.set_state(st)
        _, _, fit = f.sf.get_state()                                                       # the fit the device scans
        f.plane(ratio, reject)
        cp, w = f.surface()
        obs, p6 = f.precisions()
    finally:
        f.close()
    ocp, ow, win, cands = pp.correspondence(fit, cells, tv, tt)
    assert np.abs(cp - ocp).max() < 1e-10 * 40.0
    seen = np.ones(mo.M, bool) if not reject else ow == 1.0
    assert np.array_equal(w, ow if reject else np.ones(mo.M))                              # the weights that were used
    assert 0 < (ow == 0).sum() < mo.M
    assert np.array_equal(obs[seen], cp[seen])                                             # the scan's point, bit for bit
    assert not obs[~seen].any() and not p6[~seen].any()                                    # rejected: no observation
    ratios = plane_errors(p6, cands, pp.unit_normals(tv, tt), pp.kappa(tv, tt), st.sigma2, ratio, np.flatnonzero(seen))
    other = sum(1 for i in np.flatnonzero(seen) if len(cands[i]) > 1)
    print(f"{n_template}^2 on {target} ratio {ratio:g} reject {reject}: worst error / bound {ratios.max():.3e}, "
          f"{other} closest points on an edge or corner")
    assert ratios.max() <= 1.0
    if ratio == 1.0:                                                                       # isotropic: exactly (1 / sigma2) I
        assert np.array_equal(p6[seen], np.broadcast_to(np.array([1, 0, 0, 1, 0, 1]) / st.sigma2, (int(seen.sum()), 6)))


# ---------------------------------------------------------------------------------------------------------------- 2. degenerate triangle
@functools.lru_cache(maxsize=None)
def degenerate_case():
    """grid_case(17, "grid17", 12) with one zero-area triangle (a, b, b) at index 0 of the target, on an edge a -> b of a live triangle
    onto which a vertex of the state's fit projects.  The point-triangle routine serves the edge region of (a, b, b) by the expressions
    it uses for that edge of the live triangle, so the two distances tie exactly and the lowest index -- the degenerate one -- wins."""
    mo, cells, tv, tt = grid_case(17, "grid17", 12)
    st = pose_state(mo, "identity")
    cp, _, win, _ = pp.closest_triangles(st.fit, tv, tt)
    tried = 0
    for i in range(mo.M):
        for k in (1, 2):                                                                   # the edges A -> B and A -> C of the winner
            p, q = tv[tt[win[i], 0]], tv[tt[win[i], k]]
            s = float((cp[i] - p) @ (q - p) / ((q - p) @ (q - p)))
            if not (0.05 < s < 0.95 and np.linalg.norm(cp[i] - (p + s * (q - p))) < 1e-9) or tried >= 6:
                continue
            tried += 1
            tt2 = np.concatenate([np.array([[tt[win[i], 0], tt[win[i], k], tt[win[i], k]]], dtype=np.int32), tt]).astype(np.int32)
            if (pp.closest_triangles(st.fit, tv, tt2)[2] == 0).any():
                return mo, cells, tv, tt2, st
    raise AssertionError("no vertex projects onto an edge of its triangle")


@pytest.mark.parametrize("reject", [0, 1])
def test_degenerate_target_triangle(ctx, reject):
    mo, cells, tv, tt2, st = degenerate_case()
    ratio = 100.0
    f = Plane(ctx, mo, cells, tv, tt2)
    try:
        f.set_state(st)
        _, _, fit = f.sf.get_state()
        f.plane(ratio, reject)
        _, w = f.surface()
        obs, p6 = f.precisions()
        _, sc, fit1 = f.update_plane(ratio, reject)
    finally:
        f.close()
    assert np.isfinite(p6).all() and np.isfinite(obs).all() and np.isfinite(fit1).all() and sc.status == 0
    _, _, win, cands = pp.closest_triangles(fit, tv, tt2)
    nrm, kap = pp.unit_normals(tv, tt2), pp.kappa(tv, tt2)
    flat = np.array([1, 0, 0, 1, 0, 1]) / (ratio * st.sigma2)
    assigned = []
    for i in np.flatnonzero(w == 1.0):
        if np.array_equal(p6[i], flat):                                                    # Lambda = I / v_t: only on the degenerate triangle
            assert 0 in cands[i], i
            assigned.append(int(i))
        else:
            live = [t for t in cands[i] if t != 0]
            assert plane_errors(p6, {i: np.array(live)}, nrm, kap, st.sigma2, ratio, [i])[0] <= 1.0, i
    print(f"reject {reject}: vertices {assigned} assigned to the degenerate triangle, numpy's scan: {np.flatnonzero(win == 0).tolist()}")
    assert (win == 0).any() and assigned == [i for i in np.flatnonzero(win == 0) if w[i] == 1.0]
    assert reject == 1 or len(assigned) >= 1


# ---------------------------------------------------------------------------------------------------------------- 3. whole update
def with_device_fit(f, st):
    """`st` with the fit the device instantiated for it (f holds st): the same state to 1e-16, in the bits the device scans.  The
    rejection rules are discontinuous in the fit -- the self-intersection test of an open sheet looks at segments that leave the
    template at one of its own vertices -- so the oracle must start from the same bits, as tests/test_gpu_surface_icp.py's does
    (oracle_state_of takes the fit the device returned)."""
    _, _, fit = f.sf.get_state()
    assert rel(fit, st.fit) < 1e-14
    return dataclasses.replace(st, fit=fit)


@pytest.mark.parametrize("landmarks", [False, True])
@pytest.mark.parametrize("pose", list(POSES))
def test_one_update_against_the_oracle(ctx, pose, landmarks):
    mo, cells, tv, tt = grid_case(17, "grid24", 30)
    st = pose_state(mo, pose)
    lm = three_landmarks(mo, tv) if landmarks else None
    f = Plane(ctx, mo, cells, tv, tt)
    try:
        if lm is not None:
            f.set_landmarks(lm)
        f.set_state(st)
        st = with_device_fit(f, st)
        alpha, sc, fit = f.update_plane(100.0, 1)
    finally:
        f.close()
    want, (_, ow, _) = pp.oracle_update(mo, cells, tv, tt, st, 100.0, 1, SCHEDULE, landmarks=lm)
    print(f"{pose} landmarks {landmarks}: rel(fit) {rel(fit, want.fit):.3e}, rel(alpha) {rel(alpha, want.alpha):.3e}, "
          f"rel(pose) {rel(pose_vector(sc), oracle_pose_vector(want)):.3e}")
    assert sc.status == want.status == 0 and sc.iteration == 2 and 0 < ow.sum() < mo.M
    assert rel(fit, want.fit) < 1e-5 and rel(alpha, want.alpha) < 1e-5 and rel(pose_vector(sc), oracle_pose_vector(want)) < 1e-5
    assert rel(fit, st.fit) > 1e-4
    assert sc.sigma2 == pp.schedule(st.sigma2, *SCHEDULE) == want.sigma2
    if landmarks:                                                                          # (the override is seen)
        without, _ = pp.oracle_update(mo, cells, tv, tt, st, 100.0, 1, SCHEDULE)
        assert rel(without.fit, want.fit) > 1e-7


# ---------------------------------------------------------------------------------------------------------------- 4. the route it replaces
def host_route(f, ctx, ratio, sched):
    """closest points and covariances on the host (the Template route of examples/demo_point_to_plane.py), then the dense list"""
    import gingr_amd as ga
    _, sc, fit = f.sf.get_state()
    tv, tt = f.sf._target, f.tcells
    cp, _, tid, _ = ctx.mesh_closest_points(fit, tv, tt)
    a, b, c = (tv[tt[:, k]] for k in range(3))
    covs = ga.normalTangentCovariances(np.cross(b - a, c - a)[tid], sc.sigma2, ratio * sc.sigma2)
    return np.arange(f.mo.M), cp, covs, sc.sigma2


@pytest.mark.parametrize("case", ["grid16", "grid17", "femur"])
def test_native_call_equals_the_host_route(ctx, case):
    mo, cells, tv, tt = femur_case() if case == "femur" else grid_case(int(case[4:]), "grid24" if case == "grid17" else "grid17", 24)
    st = pose_state(mo, "identity", seed=3)
    ratio = 100.0
    f = Plane(ctx, mo, cells, tv, tt)
    try:
        f.set_state(st)
        pids, cp, covs, s2 = host_route(f, ctx, ratio, SCHEDULE)
        f.set_dense(pids, cp, covs)
        f.update()
        f.set_sigma2(pp.schedule(s2, *SCHEDULE))
        host = f.sf.get_state()
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        f.set_pairs_cov(pids, cp, covs)                                                    # the landmark pass on the same inputs
        f.set_state(st)
        _, _, fit_lm = f.update()
        f.set_pairs_cov([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        f.set_state(st)
        native = f.update_plane(ratio, 0)
    finally:
        f.close()
    spread = rel(fit_lm, host[2])
    print(f"{case}: native against host route rel(fit) {rel(native[2], host[2]):.3e}, rel(alpha) {rel(native[0], host[0]):.3e}; "
          f"spread of the landmark and the dense pass {spread:.3e}")
    assert native[1].status == host[1].status == 0 and rel(host[2], st.fit) > 1e-4
    assert rel(native[2], host[2]) < ROUTE_BOUND
    assert native[1].sigma2 == host[1].sigma2 and native[1].iteration == host[1].iteration


# ---------------------------------------------------------------------------------------------------------------- 5. ratio 1
@pytest.mark.parametrize("case", ["grid17", "femur"])
def test_ratio_one_is_the_surface_icp(ctx, case):
    mo, cells, tv, tt = femur_case() if case == "femur" else grid_case(17, "grid24", 24)
    st = pose_state(mo, "identity", seed=4)
    f = Plane(ctx, mo, cells, tv, tt)
    try:
        f.set_state(st)
        plane = f.update_plane(1.0, 1)
        _, w = f.surface()
        f.set_state(st)
        icp = f.update_icp_surface()
    finally:
        f.close()
    print(f"{case}: ratio 1 against surface ICP rel(fit) {rel(plane[2], icp[2]):.3e}")
    assert plane[1].status == icp[1].status == 0 and 0 < w.sum() < mo.M
    assert rel(plane[2], icp[2]) < ROUTE_BOUND and rel(icp[2], st.fit) > 1e-4
    assert plane[1].sigma2 == icp[1].sigma2 == pp.schedule(st.sigma2, *SCHEDULE) and plane[1].iteration == icp[1].iteration


# ---------------------------------------------------------------------------------------------------------------- 6. the loop
def test_the_loop_is_the_sum_of_its_steps(ctx):
    mo, cells, tv, tt = grid_case(17, "grid24", 24)
    st = pose_state(mo, "posed", seed=5)
    ratio, reject = 100.0, 1
    outs = []
    for how in ("n=5", "n=5", "5 x n=1", "5 rounds"):                                      # (a fresh fitter each: the first two must agree too)
        f = Plane(ctx, mo, cells, tv, tt)
        try:
            f.set_state(st)
            if how == "n=5":
                out = f.update_plane(ratio, reject, n=5)
            elif how == "5 x n=1":
                for _ in range(5):
                    out = f.update_plane(ratio, reject, n=1)
            else:
                s2 = st.sigma2
                for _ in range(5):
                    f.plane(ratio, reject)
                    f.update()
                    s2 = pp.schedule(s2, *SCHEDULE)
                    f.set_sigma2(s2)
                out = f.sf.get_state()
            outs.append(out)
        finally:
            f.close()
    assert outs[0][1].status == 0 and outs[0][1].iteration == st.iteration + 5 and rel(outs[0][2], st.fit) > 1e-4
    s2 = st.sigma2
    for _ in range(5):
        s2 = pp.schedule(s2, *SCHEDULE)
    assert outs[0][1].sigma2 == s2
    for o in outs[1:]:
        assert same_state(o, outs[0])


# ---------------------------------------------------------------------------------------------------------------- 7. ownership, memo
def test_list_ownership_and_memo(ctx):
    mo, cells, tv, tt = grid_case(16, "grid17", 16)
    rng = np.random.default_rng(8)
    st, other = pose_state(mo, "identity", seed=6), pose_state(mo, "posed", seed=7)
    hp = rng.permutation(mo.M)[:150].astype(np.int64)                                       # a host list for the dense call
    hx = (mo.ref + mo.mean)[hp] + rng.normal(0, 1.0, (150, 3))
    hc = spd_covariances(rng, 150)
    ip = rng.choice(mo.M, 200).astype(np.int64)                                             # an isotropic list
    ix = (mo.ref + mo.mean)[ip] + rng.normal(0, 1.0, (200, 3))
    iv = rng.uniform(0.5, 4.0, 200)
    f, fresh = Plane(ctx, mo, cells, tv, tt), Plane(ctx, mo, cells, tv, tt)
    try:
        f.set_state(st)
        fresh.set_state(st)
        f.plane(100.0, 1)
        planes = f.precisions()
        assert planes[1].any()
        f.set_dense(hp, hx, hc)                                                            # replaces the planes ...
        fresh.set_dense(hp, hx, hc)
        host = fresh.precisions()
        assert all(np.array_equal(x, y) for x, y in zip(f.precisions(), host)) and not np.array_equal(host[1], planes[1])
        f.plane(100.0, 1)                                                                  # ... and is replaced in turn
        assert all(np.array_equal(x, y) for x, y in zip(f.precisions(), planes))
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))                             # K = 0 clears
        assert not f.precisions()[0].any() and not f.precisions()[1].any()
        # an isotropic list set beforehand still adds
        f.set_pairs(ip, ix, iv)
        f.set_state(st)
        st = with_device_fit(f, st)
        _, sc, fit = f.update_plane(100.0, 1)
        cp, w, win, _ = pp.correspondence(st.fit, cells, tv, tt)
        keep = np.flatnonzero(w == 1.0)
        covs = pp.covariances(pp.unit_normals(tv, tt, np.float64)[win], st.sigma2, 100.0)
        lm = go.Landmarks(np.concatenate([keep, ip]), np.concatenate([cp[keep], ix]), np.concatenate([covs[keep], iv[:, None, None] * np.eye(3)[None]]))
        want = go.update_from_observations(mo, st, *pp.NONE_ISO, pp.schedule(st.sigma2, *SCHEDULE), landmarks=lm)
        only, _ = pp.oracle_update(mo, cells, tv, tt, st, 100.0, 1, SCHEDULE)
        print(f"isotropic list + planes: rel(fit) {rel(fit, want.fit):.3e}")
        assert sc.status == want.status == 0 and rel(fit, want.fit) < 1e-5 and rel(only.fit, want.fit) > 1e-6
        f.set_pairs([], np.zeros((0, 3)), np.zeros(0))
        # the memo: a density asked after the planes were refreshed from ANOTHER state is that of a fitter that never saw the first
        f.set_state(st)
        f.plane(100.0, 1)
        first = f.logpdf(st.fit)
        f.set_state(other)
        f.plane(100.0, 1)
        got = f.logpdf(other.fit)
        fresh.set_state(other)
        fresh.plane(100.0, 1)
        assert got == fresh.logpdf(other.fit) and np.isfinite(got) and got != first
    finally:
        f.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the Python class
def template_route(ctx, tv, tt, ratio, schedule):
    """TemplateRegistration with the callbacks of examples/demo_point_to_plane.py and ICP's linear schedule"""
    import gingr_amd as ga
    a, b, c = (tv[tt[:, k]] for k in range(3))
    normals = np.cross(b - a, c - a)
    memo = {}

    def closest(state):
        if memo.get("state") is not state:
            memo["state"], memo["cp"] = state, ctx.mesh_closest_points(state.general.fit, tv, tt)
        return memo["cp"][0], memo["cp"][2]

    def corr(state):
        return ga.CorrespondencePairs(np.arange(state.general.model.numberOfPoints), closest(state)[0])

    def unc(pids, state):
        s2 = state.general.sigma2
        return ga.normalTangentCovariances(normals[closest(state)[1][pids]], s2, ratio * s2)

    step = (schedule[0] - schedule[1]) / float(schedule[2])
    return ga.TemplateRegistration(ctx, corr, unc, updateSigma2=lambda s: max(s.general.sigma2 - step, schedule[1]), covariancePass="gram"), corr, unc


def test_python_class_on_the_femur_pair(ctx):
    import gingr_amd as ga
    mo, cells, tv, tt = femur_case()
    model = ga_model(mo, cells)
    sched = (20.0, 1.0, 11)
    cfg = ga.PointToPlaneConfiguration(maxIterations=11, initialSigma=sched[0], endSigma=sched[1], tangentOverNormal=100.0)
    algo, stepper = ga.PointToPlaneIcpRegistration(ctx), ga.PointToPlaneIcpRegistration(ctx)
    tmpl, corr, unc = template_route(ctx, tv, tt, 100.0, sched)
    post = None
    try:
        with pytest.raises(ValueError):
            algo.createInitialState(ga_model(mo), tv, cfg, targetCells=tt)                  # no model cells
        with pytest.raises(ValueError):
            algo.createInitialState(model, tv, cfg)                                        # no target cells
        state = algo.createInitialState(model, tv, cfg, targetCells=tt, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
        assert state.general.sigma2 == sched[0]
        done = algo.run(state)                                                             # one enqueue of ten iterations
        s = stepper.createInitialState(model, tv, cfg, targetCells=tt, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
        tcfg = ga.TemplateConfiguration(maxIterations=1)
        for it in range(10):
            if it < 3:                                                                     # the route it replaces, from the same state
                t_next = tmpl.update(ga.TemplateRegistrationState(s.general, tcfg))
            s = stepper.update(s)
            if it < 3:
                d = rel(s.general.fit, t_next.general.fit)
                print(f"iteration {it + 1}: native against Template rel(fit) {d:.3e}")
                assert d < ROUTE_BOUND and s.general.sigma2 == t_next.general.sigma2
        g, h = done.general, s.general
        assert g.iteration == h.iteration == 10 and g.status == ga.FittingStatuses.MaxIteration and h.status == 0
        assert np.array_equal(g.fit, h.fit) and np.array_equal(g.modelParameters.shape, h.modelParameters.shape) and g.sigma2 == h.sigma2
        assert rel(g.fit, state.general.fit) > 1e-4
        # what the device used
        pairs = stepper.getCorrespondence(s)
        cp, w = stepper.surfaceCorrespondence(s)
        assert np.array_equal(pairs.pids, np.arange(mo.M)) and np.array_equal(pairs.points, cp) and (w == 1.0).all()
        want_unc = unc(np.array([5, 700]), s)
        for k, pid in enumerate((5, 700)):
            assert np.abs(stepper.getUncertainty(pid, s) - want_unc[k]).max() < 1e-9 * np.abs(want_unc[k]).max()
        # the queries of the pairs flavour, from the planes of the queried state
        ts = ga.TemplateRegistrationState(s.general, tcfg)
        nxt, t_nxt = stepper.update(s), tmpl.update(ts)
        lp, t_lp = stepper.logTransitionProbability(s, nxt), tmpl.logTransitionProbability(ts, t_nxt)
        print(f"logTransitionProbability {lp!r}, Template {t_lp!r}")
        assert np.isfinite(lp) and abs(lp - t_lp) < 1e-5 * abs(t_lp)
        st = oracle_state_of(s.general, 1)
        pids = np.arange(mo.M)
        cps, covs = corr(ts).points, unc(pids, ts)
        a, b = posterior_routes(mo, st, pids, cps, covs)
        check("point-to-plane femur", mats(stepper.posteriorCovariance(s)), a, b)
        post = stepper.posteriorModel(s)
        check_model("point-to-plane femur", post, state_routes(mo, st, pids, cps, covs))
    finally:
        if post is not None:
            post.close()
        for x in (algo, stepper, tmpl):
            x.close()


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_change_nothing(ctx):
    from gingr_amd import _native as nat
    import gingr_amd as ga
    mo, cells, tv, tt = grid_case(16, "grid17", 12)
    st = pose_state(mo, "identity")
    good, sched = nat.PlaneParams(100.0, 1), nat.IcpParams(*SCHEDULE)

    def both(f, p, s=sched, n=1):
        pp_ = None if p is None else ctypes.byref(p)
        return (f.lib.gingr_fitter_set_pairs_plane_async(f.h, pp_),
                f.lib.gingr_fitter_update_plane_async(f.h, pp_, None if s is None else ctypes.byref(s), n))

    # no target: a bare fitter
    dm = ga.DeviceModel(ctx, ga_model(mo, cells))
    h = ctypes.c_void_p()
    assert ctx._lib.gingr_fitter_create(ctx.handle, dm.handle, ctypes.byref(h)) == 0
    try:
        assert ctx._lib.gingr_fitter_set_pairs_plane_async(h, ctypes.byref(good)) == ERR_STATE
        assert ctx._lib.gingr_fitter_update_plane_async(h, ctypes.byref(good), ctypes.byref(sched), 1) == ERR_STATE
    finally:
        ctx._lib.gingr_fitter_destroy(h)
        dm.close()
    f = Plane(ctx, mo, cells, tv, tt, meshes=False)
    try:
        assert both(f, good) == (ERR_STATE, ERR_STATE)                                      # no state
        f.set_state(st)
        assert both(f, good) == (ERR_STATE, ERR_STATE)                                      # no meshes
    finally:
        f.close()
    shard = Dense(ctx, mo, tv, rank=0, world=2, defer=True)                                # a row shard (its moments are never used)
    try:
        shard.sf.finish_setup()
        shard.set_state(st)
        shard.sf.set_meshes(cells, tt)
        assert both(shard, good) == (ERR_STATE, ERR_STATE)
    finally:
        shard.close()
    f = Plane(ctx, mo, cells, tv, tt)
    try:
        f.set_state(st)
        f.plane(100.0, 1)
        before = (f.precisions(), f.sf.get_state())

        def unchanged():
            now = (f.precisions(), f.sf.get_state())
            return all(np.array_equal(x, y) for x, y in zip(now[0], before[0])) and same_state(now[1], before[1])

        f.ok(f.lib.gingr_fitter_set_surface_method(f.h, 1), "set_surface_method")
        assert both(f, good) == (ERR_STATE, ERR_STATE) and unchanged()                      # the along-normal method
        f.ok(f.lib.gingr_fitter_set_surface_method(f.h, 0), "set_surface_method")
        f.ok(f.lib.gingr_fitter_set_correspondence_direction(f.h, 1), "set_correspondence_direction")
        assert both(f, good) == (ERR_STATE, ERR_STATE) and unchanged()                      # the reversed direction
        f.ok(f.lib.gingr_fitter_set_correspondence_direction(f.h, 0), "set_correspondence_direction")
        assert both(f, None) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged()
        for ratio in (0.5, 0.0, -1.0, np.nan, np.inf):
            assert both(f, nat.PlaneParams(ratio, 1)) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged(), ratio
        for rj in (2, -1):
            assert both(f, nat.PlaneParams(100.0, rj)) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged(), rj
        for n in (0, -3):
            assert both(f, good, n=n)[1] == ERR_BAD_ARGUMENT and unchanged()
        assert both(f, good, s=None)[1] == ERR_BAD_ARGUMENT and unchanged()
        assert both(f, good, s=nat.IcpParams(2.0, 0.5, 0))[1] == ERR_BAD_ARGUMENT and unchanged()
        assert ctx._lib.gingr_fitter_set_pairs_plane_async(None, ctypes.byref(good)) == ERR_BAD_ARGUMENT
        assert ctx._lib.gingr_fitter_update_plane_async(None, ctypes.byref(good), ctypes.byref(sched), 1) == ERR_BAD_ARGUMENT
        _, sc, _ = f.update_plane(100.0, 1)                                                # and the fitter still works
        assert sc.status == 0 and sc.iteration == st.iteration + 1
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 10. leaks
def test_create_run_destroy_gives_the_memory_back(ctx):
    import torch
    mo, cells, tv, tt = grid_case(17, "grid24", 24)
    st = pose_state(mo, "identity")

    def free_bytes():
        torch.cuda.synchronize(0)
        return torch.cuda.mem_get_info(0)[0]

    def cycle():
        f = Plane(ctx, mo, cells, tv, tt)
        try:
            f.set_state(st)
            _, sc, _ = f.update_plane(100.0, 1, n=3)
            assert sc.status == 0
            f.precisions()
        finally:
            f.close()

    cycle()                                                                                # warm-up: code objects, allocator pools
    gc.collect()
    before = free_bytes()
    for _ in range(20):
        cycle()
    gc.collect()
    after = free_bytes()
    assert before - after < 16 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
