"""GPU tests of point-to-plane ICP against a point cloud (gingr_fitter_set_target_normals / _estimate_target_normals /
_get_target_normals, gingr_fitter_set_pairs_plane_cloud_async / gingr_fitter_update_plane_cloud_async, gingr_amd/csrc/fitter_pairs.hip:
plane_cloud_pairs_kernel) and of PointToPlaneIcpRegistration's cloud route.  The template sheets and the femur model are those of
tests/test_gpu_plane_pairs.py; the targets are used as vertices only.

Planes, element-wise: the matches of gingr_fitter_get_icp_idx equal the restatement's brute-force argmin (tests/
cloud_normals_restatement.py) and their d2 its bits; xbar is target[idx] bit for bit; Lambda_i per entry against the closed form in
np.longdouble on the normals the device holds, within 32 u / v_n, u = 2^-53: the bound of tests/test_gpu_plane_pairs.py with kappa = 1 for
a normal that is already unit.  Whole updates: rel(fit) < 1e-5 against the oracle on the device's normals (alpha and pose likewise),
sigma2 equal to the schedule's value bit for bit.  Two routes of one update on the same device: rel(fit) < 1e-9 (ROUTE_BOUND of
tests/test_gpu_plane_pairs.py)."""
import ctypes

import numpy as np
import pytest

from tests import cloud_normals_restatement as cr
from tests import plane_pairs_restatement as pp
from tests.test_gpu_pairs_cov_gram import POSES, Dense, lambda_of
from tests.test_gpu_plane_pairs import (ROUTE_BOUND, SCHEDULE, femur_case, grid_case, oracle_pose_vector, pose_state, pose_vector,
                                        same_state)
from tests.test_gpu_posterior_covariance import check, ga_model, mats, posterior_routes, three_landmarks
from tests.test_gpu_posterior_model import check_model, state_routes
from tests.test_gpu_surface_icp import oracle_state_of, rel

pytestmark = pytest.mark.gpu

ERR_BAD_ARGUMENT, ERR_NONFINITE, ERR_STATE = 1, 3, 6
NEIGHBOURS = 12


class Cloud(Dense):
    """Dense plus the target normals and the two point-cloud entry points; no meshes."""

    @staticmethod
    def params(ratio, max_distance=0.0):
        from gingr_amd import _native as nat
        return nat.PlaneCloudParams(float(ratio), float(max_distance))

    def estimate(self, k=NEIGHBOURS, viewpoint=None, expect_ok=True):
        from gingr_amd import _native as nat
        from gingr_amd._native import dptr
        info = nat.CloudKnnInfo()
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64)
        rc = self.lib.gingr_fitter_estimate_target_normals(self.h, int(k), dptr(v), ctypes.byref(info))
        if expect_ok:
            self.ok(rc, "estimate_target_normals")
            return info
        return rc

    def set_normals(self, normals, expect_ok=True):
        from gingr_amd._native import dptr
        n = np.ascontiguousarray(normals, dtype=np.float64)
        rc = self.lib.gingr_fitter_set_target_normals(self.h, dptr(n))
        if expect_ok:
            self.ok(rc, "set_target_normals")
        return rc

    def normals(self):
        from gingr_amd._native import dptr
        out = np.empty((self.sf._target.shape[0], 3))
        self.ok(self.lib.gingr_fitter_get_target_normals(self.h, dptr(out)), "get_target_normals")
        return out

    def plane(self, ratio, max_distance=0.0, expect_ok=True):
        p = self.params(ratio, max_distance)
        rc = self.lib.gingr_fitter_set_pairs_plane_cloud_async(self.h, ctypes.byref(p))
        if expect_ok:
            self.ok(rc, "set_pairs_plane_cloud_async")
        return rc

    def update_plane(self, ratio, max_distance=0.0, sched=SCHEDULE, n=1):
        from gingr_amd import _native as nat
        p, s = self.params(ratio, max_distance), nat.IcpParams(float(sched[0]), float(sched[1]), int(sched[2]))
        self.ok(self.lib.gingr_fitter_update_plane_cloud_async(self.h, ctypes.byref(p), ctypes.byref(s), int(n)), "update_plane_cloud_async")
        return self.sf.get_state()

    def update_icp(self, sched=SCHEDULE, n=1):
        from gingr_amd import _native as nat
        s = nat.IcpParams(float(sched[0]), float(sched[1]), int(sched[2]))
        self.ok(self.lib.gingr_fitter_update_icp_async(self.h, ctypes.byref(s), int(n)), "update_icp_async")
        return self.sf.get_state()

    def matches(self):
        from gingr_amd._native import dptr, iptr
        idx, d2 = np.empty(self.mo.M, dtype=np.int32), np.empty(self.mo.M)
        self.ok(self.lib.gingr_fitter_get_icp_idx(self.h, iptr(idx), dptr(d2)), "get_icp_idx")
        return idx, d2

    def set_sigma2(self, s2):
        self.ok(self.lib.gingr_fitter_set_sigma2(self.h, float(s2)), "set_sigma2")

    def set_landmarks(self, lm):
        from gingr_amd._native import dptr, iptr
        lp, lx, lc = lm.pids.astype(np.int32), np.ascontiguousarray(lm.points), np.ascontiguousarray(lm.covs)
        self.ok(self.lib.gingr_fitter_set_landmarks(self.h, lp.shape[0], iptr(lp), dptr(lx), dptr(lc)), "set_landmarks")


def case(name):
    """(oracle model, target vertices)"""
    if name == "femur24":
        mo, _, tv, _ = femur_case()
    else:
        mo, _, tv, _ = grid_case(16, "grid17", 12) if name == "grid12" else grid_case(17, "grid24", 30)
    return mo, np.ascontiguousarray(tv)


def plane_ratio(p6, normals_ld, v_n, ratio):
    """per vertex max |Lambda - closed form in longdouble| / (32 u / v_n)"""
    want = pp.closed_form(normals_ld, v_n, ratio, np.longdouble)
    return (np.abs(want - lambda_of(p6).astype(np.longdouble)).max(axis=(1, 2)) / (32 * pp.U53 / v_n)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- 1. planes
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("ratio", [1.0, 100.0, 1e8])
@pytest.mark.parametrize("name", ["grid12", "grid30"])
def test_planes_element_wise(ctx, name, ratio, far):
    mo, tv = case(name)
    st = pose_state(mo, "posed")
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        _, _, fit = f.sf.get_state()                                                       # the fit the device searches from
        f.estimate()
        tn = f.normals()
        nn, want_d2 = cr.nearest(fit, tv)
        max_distance = float(np.sqrt(np.quantile(want_d2, 0.7))) if far else 0.0           # about 30 % rejected
        f.plane(ratio, max_distance)
        idx, d2 = f.matches()
        obs, p6 = f.precisions()
    finally:
        f.close()
    assert np.array_equal(idx, nn) and np.array_equal(d2.view(np.uint64), want_d2.view(np.uint64))
    seen = ~(d2 > max_distance * max_distance) if far else np.ones(mo.M, bool)
    if far:
        assert 0.05 * mo.M <= (~seen).sum() <= 0.5 * mo.M
    assert np.array_equal(obs[seen], tv[idx[seen]])                                        # the target point, bit for bit
    assert not obs[~seen].any() and not p6[~seen].any()                                    # rejected: no observation
    assert np.abs(np.linalg.norm(tn, axis=1) - 1.0).max() <= 8 * pp.U53 and seen.any()
    ratios = plane_ratio(p6[seen], tn[idx[seen]].astype(np.longdouble), st.sigma2, ratio)
    print(f"{name} ratio {ratio:g} far {far}: worst error / bound {ratios.max():.3e}, {int((~seen).sum())} of {mo.M} rejected")
    assert ratios.max() <= 1.0
    if ratio == 1.0:                                                                       # isotropic: exactly (1 / sigma2) I
        assert np.array_equal(p6[seen], np.broadcast_to(np.array([1, 0, 0, 1, 0, 1]) / st.sigma2, (int(seen.sum()), 6)))
    else:
        assert np.abs(p6[seen][:, [1, 2, 4]]).max() > 0


def test_zero_and_supplied_normals(ctx):
    mo, tv = case("grid12")
    st = pose_state(mo, "identity")
    rng = np.random.default_rng(2)
    raw = rng.normal(0, 3.0, tv.shape)                                                     # any length: normalised on upload
    raw[::3] = 0.0                                                                         # every third target point without a normal
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        f.set_normals(raw)
        tn = f.normals()
        f.plane(100.0)
        idx, _ = f.matches()
        _, p6 = f.precisions()
    finally:
        f.close()
    length = np.linalg.norm(raw, axis=1)
    assert not tn[::3].any() and np.abs(tn[length > 0] - (raw / np.where(length > 0, length, 1)[:, None])[length > 0]).max() <= 8 * pp.U53
    flat = idx % 3 == 0
    assert flat.any() and (~flat).any()
    assert np.array_equal(p6[flat], np.broadcast_to(np.array([1, 0, 0, 1, 0, 1]) / (100.0 * st.sigma2), (int(flat.sum()), 6)))
    assert plane_ratio(p6[~flat], tn[idx[~flat]].astype(np.longdouble), st.sigma2, 100.0).max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. whole updates
@pytest.mark.parametrize("landmarks", [False, True])
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("name", ["grid12", "grid30", "femur24"])
def test_one_update_against_the_oracle(ctx, name, pose, landmarks):
    mo, tv = case(name)
    st = pose_state(mo, pose)
    lm = three_landmarks(mo, tv) if landmarks else None
    f = Cloud(ctx, mo, tv)
    try:
        if lm is not None:
            f.set_landmarks(lm)
        f.set_state(st)
        f.estimate()
        tn = f.normals()
        alpha, sc, fit = f.update_plane(100.0)
    finally:
        f.close()
    want, _ = cr.oracle_update_cloud(mo, tv, tn, st, 100.0, SCHEDULE, landmarks=lm)
    print(f"{name} {pose} landmarks {landmarks}: rel(fit) {rel(fit, want.fit):.3e}, rel(alpha) {rel(alpha, want.alpha):.3e}, "
          f"rel(pose) {rel(pose_vector(sc), oracle_pose_vector(want)):.3e}")
    assert sc.status == want.status == 0 and sc.iteration == 2
    assert rel(fit, want.fit) < 1e-5 and rel(alpha, want.alpha) < 1e-5 and rel(pose_vector(sc), oracle_pose_vector(want)) < 1e-5
    assert rel(fit, st.fit) > 1e-4
    assert sc.sigma2 == pp.schedule(st.sigma2, *SCHEDULE) == want.sigma2
    if landmarks:                                                                          # (the override is seen)
        without, _ = cr.oracle_update_cloud(mo, tv, tn, st, 100.0, SCHEDULE)
        assert rel(without.fit, want.fit) > 1e-7


def test_rejection_in_a_whole_update(ctx):
    mo, tv = case("grid30")
    st = pose_state(mo, "posed")
    max_distance = float(np.sqrt(np.quantile(cr.nearest(st.fit, tv)[1], 0.7)))
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        f.estimate()
        tn = f.normals()
        alpha, sc, fit = f.update_plane(100.0, max_distance)
    finally:
        f.close()
    want, (_, _, seen) = cr.oracle_update_cloud(mo, tv, tn, st, 100.0, SCHEDULE, max_distance=max_distance)
    every, _ = cr.oracle_update_cloud(mo, tv, tn, st, 100.0, SCHEDULE)
    print(f"max_distance {max_distance:.3f}: {int((~seen).sum())} rejected, rel(fit) {rel(fit, want.fit):.3e}")
    assert sc.status == 0 and rel(fit, want.fit) < 1e-5 and rel(alpha, want.alpha) < 1e-5 and rel(every.fit, want.fit) > 1e-6


@pytest.mark.parametrize("name", ["grid30", "femur24"])
def test_the_loop_is_the_sum_of_its_steps(ctx, name):
    mo, tv = case(name)
    st = pose_state(mo, "posed", seed=5)
    outs = []
    for how in ("n=3", "3 x n=1"):
        f = Cloud(ctx, mo, tv)
        try:
            f.set_state(st)
            f.estimate()
            if how == "n=3":
                out = f.update_plane(100.0, n=3)
            else:
                for _ in range(3):
                    out = f.update_plane(100.0, n=1)
            outs.append(out)
        finally:
            f.close()
    s2 = st.sigma2
    for _ in range(3):
        s2 = pp.schedule(s2, *SCHEDULE)
    assert outs[0][1].status == 0 and outs[0][1].iteration == st.iteration + 3 and outs[0][1].sigma2 == s2
    assert rel(outs[0][2], st.fit) > 1e-4 and same_state(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- 3. two routes
@pytest.mark.parametrize("name", ["grid12", "grid30", "femur24"])
def test_native_call_equals_the_dense_list(ctx, name):
    import gingr_amd as ga
    mo, tv = case(name)
    st = pose_state(mo, "identity", seed=3)
    ratio = 100.0
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        f.estimate()
        tn = f.normals()
        f.plane(ratio)
        idx, _ = f.matches()
        f.set_dense(np.arange(mo.M), tv[idx], ga.normalTangentCovariances(tn[idx], st.sigma2, ratio * st.sigma2))
        f.update()
        f.set_sigma2(pp.schedule(st.sigma2, *SCHEDULE))
        host = f.sf.get_state()
        f.set_dense([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
        f.set_state(st)
        native = f.update_plane(ratio)
    finally:
        f.close()
    print(f"{name}: native against the dense list rel(fit) {rel(native[2], host[2]):.3e}, rel(alpha) {rel(native[0], host[0]):.3e}")
    assert native[1].status == host[1].status == 0 and rel(host[2], st.fit) > 1e-4
    assert rel(native[2], host[2]) < ROUTE_BOUND
    assert native[1].sigma2 == host[1].sigma2 and native[1].iteration == host[1].iteration


@pytest.mark.parametrize("name", ["grid30", "femur24"])
def test_ratio_one_is_the_point_cloud_icp(ctx, name):
    mo, tv = case(name)
    st = pose_state(mo, "identity", seed=4)
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        f.estimate()
        plane = f.update_plane(1.0)
        f.set_state(st)
        icp = f.update_icp()
    finally:
        f.close()
    print(f"{name}: ratio 1 against point-cloud ICP rel(fit) {rel(plane[2], icp[2]):.3e}")
    assert plane[1].status == icp[1].status == 0
    assert rel(plane[2], icp[2]) < ROUTE_BOUND and rel(icp[2], st.fit) > 1e-4
    assert plane[1].sigma2 == icp[1].sigma2 == pp.schedule(st.sigma2, *SCHEDULE) and plane[1].iteration == icp[1].iteration


# ---------------------------------------------------------------------------------------------------------------- 4. normals
@pytest.mark.parametrize("name", ["grid30", "femur24"])
def test_estimated_and_supplied_normals(ctx, name):
    mo, tv = case(name)
    st = pose_state(mo, "posed")
    below = tv.mean(0) - np.array([0.0, 0.0, 500.0])                                      # (the canonical sign of a sheet's normals is up)
    f = Cloud(ctx, mo, tv)
    try:
        f.set_state(st)
        info = f.estimate()
        tn = f.normals()
        want, _ = ctx.cloud_normals(tv, NEIGHBOURS)
        assert np.array_equal(tn.view(np.uint64), want.view(np.uint64))                     # the bits of the stateless call
        assert info.flagged == 0 and info.cell_size > 0 and min(info.grid) >= 1
        f.plane(100.0)
        planes = f.precisions()
        f.set_normals(tn)                                                                  # the same normals, supplied
        assert np.array_equal(f.normals().view(np.uint64), tn.view(np.uint64))
        f.plane(100.0)
        assert all(np.array_equal(x, y) for x, y in zip(f.precisions(), planes)) and planes[1].any()
        f.estimate(viewpoint=below)
        turned = f.normals()
        want_v, _ = ctx.cloud_normals(tv, NEIGHBOURS, viewpoint=below)
        assert np.array_equal(turned.view(np.uint64), want_v.view(np.uint64)) and not np.array_equal(turned, tn)
        f.plane(100.0)                                                                     # n n^T is even in n: the same planes
        assert all(np.array_equal(x, y) for x, y in zip(f.precisions(), planes))
        f.estimate(k=16)
        assert not np.array_equal(f.normals(), tn)
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 5. states, errors
def test_refusals_change_nothing(ctx):
    from gingr_amd import _native as nat
    import gingr_amd as ga
    mo, tv = case("grid12")
    st = pose_state(mo, "identity")
    good, sched = nat.PlaneCloudParams(100.0, 0.0), nat.IcpParams(*SCHEDULE)

    def both(f, p, s=sched, n=1):
        pp_ = None if p is None else ctypes.byref(p)
        return (f.lib.gingr_fitter_set_pairs_plane_cloud_async(f.h, pp_),
                f.lib.gingr_fitter_update_plane_cloud_async(f.h, pp_, None if s is None else ctypes.byref(s), n))

    dm = ga.DeviceModel(ctx, ga_model(mo))                                                 # no target: a bare fitter
    h = ctypes.c_void_p()
    assert ctx._lib.gingr_fitter_create(ctx.handle, dm.handle, ctypes.byref(h)) == 0
    try:
        from gingr_amd._native import dptr
        assert ctx._lib.gingr_fitter_set_pairs_plane_cloud_async(h, ctypes.byref(good)) == ERR_STATE
        assert ctx._lib.gingr_fitter_estimate_target_normals(h, 12, None, None) == ERR_STATE
        assert ctx._lib.gingr_fitter_set_target_normals(h, dptr(np.zeros((4, 3)))) == ERR_STATE
        assert ctx._lib.gingr_fitter_get_target_normals(h, dptr(np.zeros((4, 3)))) == ERR_STATE
    finally:
        ctx._lib.gingr_fitter_destroy(h)
        dm.close()
    shard = Dense(ctx, mo, tv, rank=0, world=2, defer=True)                                # a row shard
    try:
        shard.sf.finish_setup()
        shard.set_state(st)
        Cloud.estimate(shard)
        assert both(shard, good) == (ERR_STATE, ERR_STATE)
    finally:
        shard.close()
    f = Cloud(ctx, mo, tv)
    try:
        assert both(f, good) == (ERR_STATE, ERR_STATE)                                      # no state
        f.set_state(st)
        assert both(f, good) == (ERR_STATE, ERR_STATE)                                      # no normals
        assert "no target normals" in (f.lib.gingr_last_error(ctx.handle) or b"").decode()
        for k in (2, 65, tv.shape[0] + 1):
            assert f.estimate(k=k, expect_ok=False) == ERR_BAD_ARGUMENT and both(f, good) == (ERR_STATE, ERR_STATE)
        bad = np.zeros(tv.shape)
        bad[5, 2] = np.nan
        assert f.set_normals(bad, expect_ok=False) == ERR_NONFINITE and both(f, good) == (ERR_STATE, ERR_STATE)
        f.estimate()
        f.plane(100.0)
        before = (f.precisions(), f.sf.get_state(), f.normals())

        def unchanged():
            now = (f.precisions(), f.sf.get_state(), f.normals())
            return (all(np.array_equal(x, y) for x, y in zip(now[0], before[0])) and same_state(now[1], before[1]) and
                    np.array_equal(now[2], before[2]))

        assert both(f, None) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged()
        for ratio in (0.5, 0.0, -1.0, np.nan, np.inf):
            assert both(f, nat.PlaneCloudParams(ratio, 0.0)) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged(), ratio
        assert both(f, nat.PlaneCloudParams(100.0, np.nan)) == (ERR_BAD_ARGUMENT, ERR_BAD_ARGUMENT) and unchanged()
        for n in (0, -3):
            assert both(f, good, n=n)[1] == ERR_BAD_ARGUMENT and unchanged()
        assert both(f, good, s=None)[1] == ERR_BAD_ARGUMENT and unchanged()
        assert both(f, good, s=nat.IcpParams(2.0, 0.5, 0))[1] == ERR_BAD_ARGUMENT and unchanged()
        assert f.set_normals(bad, expect_ok=False) == ERR_NONFINITE and f.estimate(k=2, expect_ok=False) == ERR_BAD_ARGUMENT and unchanged()
        assert ctx._lib.gingr_fitter_set_pairs_plane_cloud_async(None, ctypes.byref(good)) == ERR_BAD_ARGUMENT
        assert ctx._lib.gingr_fitter_update_plane_cloud_async(None, ctypes.byref(good), ctypes.byref(sched), 1) == ERR_BAD_ARGUMENT
        _, sc, _ = f.update_plane(100.0)                                                   # and the fitter still works
        assert sc.status == 0 and sc.iteration == st.iteration + 1
        # a new target drops the normals
        x = np.ascontiguousarray(tv[::-1] + 0.25)
        from gingr_amd._native import dptr
        f.ok(f.lib.gingr_fitter_set_target(f.h, x.shape[0], dptr(x)), "set_target")
        assert both(f, good) == (ERR_STATE, ERR_STATE)
        assert f.lib.gingr_fitter_get_target_normals(f.h, dptr(np.empty(tv.shape))) == ERR_STATE
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the class
def test_python_class_on_the_femur_vertices(ctx):
    import gingr_amd as ga
    mo, tv = case("femur24")
    model = ga_model(mo)                                                                   # no cells: the cloud route needs none
    sched = (20.0, 1.0, 11)
    cfg = ga.PointToPlaneConfiguration(maxIterations=11, initialSigma=sched[0], endSigma=sched[1], tangentOverNormal=100.0)
    pose = ((0.02, -0.03, 0.01), (1.0, -2.0, 0.5))
    algo, stepper = ga.PointToPlaneIcpRegistration(ctx), ga.PointToPlaneIcpRegistration(ctx)
    post = None
    try:
        with pytest.raises(ValueError, match=r"point-to-plane ICP needs the triangulations \(model.cells and targetCells\)"):
            algo.createInitialState(model, tv, cfg)                                        # neither cells nor normals
        with pytest.raises(ValueError, match="reject=True"):
            algo.createInitialState(model, tv, ga.PointToPlaneConfiguration(reject=True), targetNormals="estimate")
        with pytest.raises(ValueError, match="targetNormals"):
            algo.createInitialState(model, tv, cfg, targetNormals=np.zeros((5, 3)))
        state = algo.createInitialState(model, tv, cfg, initial_pose=pose, targetNormals="estimate", targetNeighbours=NEIGHBOURS)
        assert state.general.sigma2 == sched[0] and state.general.targetCells is None
        done = algo.run(state)                                                             # one enqueue of ten iterations
        s = stepper.createInitialState(model, tv, cfg, initial_pose=pose, targetNormals="estimate", targetNeighbours=NEIGHBOURS)
        for _ in range(10):
            s = stepper.update(s)
        g, h = done.general, s.general
        assert g.iteration == h.iteration == 10 and g.status == ga.FittingStatuses.MaxIteration and h.status == 0
        assert np.array_equal(g.fit, h.fit) and np.array_equal(g.modelParameters.shape, h.modelParameters.shape) and g.sigma2 == h.sigma2
        assert rel(g.fit, state.general.fit) > 1e-4
        # what the device used, against the C calls
        tn = stepper.targetNormals(s)
        want_n, _ = ctx.cloud_normals(tv, NEIGHBOURS)
        assert np.array_equal(tn.view(np.uint64), want_n.view(np.uint64))
        cp, w = stepper.surfaceCorrespondence(s)
        nn, _ = cr.nearest(h.fit, tv)
        assert np.array_equal(cp, tv[nn]) and (w == 1.0).all()
        pairs = stepper.getCorrespondence(s)
        assert np.array_equal(pairs.pids, np.arange(mo.M)) and np.array_equal(pairs.points, cp)
        prec = stepper.pairPrecisions(s)
        assert plane_ratio(prec, tn[nn].astype(np.longdouble), h.sigma2, 100.0).max() <= 1.0
        covs = ga.normalTangentCovariances(tn[nn], h.sigma2, 100.0 * h.sigma2)
        for pid in (5, 700):
            assert np.abs(stepper.getUncertainty(pid, s) - covs[pid]).max() < 1e-9 * np.abs(covs[pid]).max()
        # supplied normals: the same run
        supplied = algo.run(algo.createInitialState(model, tv, cfg, initial_pose=pose, targetNormals=tn))
        assert np.array_equal(supplied.general.fit, g.fit)
        # maxDistance reaches the device
        far = float(np.sqrt(np.quantile(cr.nearest(state.general.fit, tv)[1], 0.6)))
        far_cfg = ga.PointToPlaneConfiguration(maxIterations=11, initialSigma=sched[0], endSigma=sched[1], maxDistance=far)
        fs = algo.createInitialState(model, tv, far_cfg, initial_pose=pose, targetNormals=tn)
        _, fw = algo.surfaceCorrespondence(fs)
        _, fd2 = cr.nearest(fs.general.fit, tv)
        assert np.array_equal(fw, np.where(fd2 > far * far, 0.0, 1.0)) and 0 < fw.sum() < mo.M
        assert not algo.pairPrecisions(fs)[fw == 0].any() and algo.pairPrecisions(fs)[fw == 1].any()
        # the queries of the pairs flavour, from the planes of the queried state
        nxt = stepper.update(s)
        lp = stepper.logTransitionProbability(s, nxt)
        assert np.isfinite(lp)
        st = oracle_state_of(h, 1)
        pids = np.arange(mo.M)
        a, b = posterior_routes(mo, st, pids, cp, covs)
        check("point-to-plane cloud femur", mats(stepper.posteriorCovariance(s)), a, b)
        post = stepper.posteriorModel(s)
        check_model("point-to-plane cloud femur", post, state_routes(mo, st, pids, cp, covs))
    finally:
        if post is not None:
            post.close()
        for x in (algo, stepper):
            x.close()
