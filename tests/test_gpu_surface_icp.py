"""GPU tests of ICP with the surface correspondence (the reference's default ICP method,
ICP.scala:63 TriangularClosestPoint -> ClosestPointRegistrator.scala:75-100) against the oracle's restatement."""
import os

import numpy as np
import pytest

from oracle import gingr_oracle as go

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def femur():
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    m = np.load(os.path.join(HERE, "golden", "femur_mesh.npz"))
    return (d["femur"].astype(np.float64), m["femur_cells"].astype(np.int32), d["femur_target"].astype(np.float64),
            m["femur_target_cells"].astype(np.int32))


def grid_mesh(n, size, height, seed):
    """Open height-field surface: (n*n vertices, 2(n-1)^2 triangles) with a boundary."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-size, size, n)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    Z = height * np.sin(X / size * 2.0) * np.cos(Y / size * 1.5) + rng.normal(0, 0.05, X.shape)
    v = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return v, tris


def model_over(ref, cells, rank=24, seed=0):
    mo = go.build_gaussian_gpmm(ref, 60.0, 20.0, rel_tol=1e-9, max_rank=rank)
    return mo


def make_state(ctx, ref, cells, target, tcells, rank=24, initial_pose=None, sigma=(20.0, 1.0), iters=30):
    import gingr_amd as ga
    mo = model_over(ref, cells, rank)
    model = ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=iters, initialSigma=sigma[0], endSigma=sigma[1],
                              correspondenceMethod="TriangularClosestPoint")
    state = algo.createInitialState(model, target, cfg, targetCells=tcells, initial_pose=initial_pose)
    return mo, algo, state


def test_surface_correspondence_femur(ctx):
    ref, cells, target, tcells = femur()
    mo, algo, state = make_state(ctx, ref, cells, target, tcells, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
    cp, w = algo.surfaceCorrespondence(state)
    ocp, ow, _ = go.surface_correspondence(np.asarray(state.general.fit), cells, target, tcells)
    assert np.array_equal(w, ow), (int((w != ow).sum()), w.shape)
    assert np.abs(cp - ocp).max() < 1e-10 * np.abs(target).max()
    assert 0 < w.sum() < w.shape[0]          # the femur pair produces accepted and rejected pairs
    pairs = algo.getCorrespondence(state)
    assert np.array_equal(pairs.pids, np.flatnonzero(ow == 1.0)) and np.abs(pairs.points - ocp[ow == 1.0]).max() < 1e-9
    algo.close()


def test_rejections_boundary_normals_selfintersection(ctx):
    """Open target (boundary vertices), a template facing the wrong way (opposite normals) and a folded template (the
    closest-point line crosses its own second sheet): every rejection rule fires and matches the oracle."""
    tv, tt = grid_mesh(24, 40.0, 6.0, 1)
    # template: a patch reaching past the target's rim, plus a second sheet folded back underneath part of it
    sv, st_ = grid_mesh(14, 46.0, 4.0, 2)
    sv = sv + np.array([3.0, -2.0, 5.0])
    fold = sv.copy()
    fold[:, 2] -= 2.5                                   # second sheet between the first one and the target
    fold_t = st_[:, [0, 2, 1]] + sv.shape[0]            # facing down
    tmpl = np.concatenate([sv, fold[: sv.shape[0] // 2]])
    keep = (fold_t < tmpl.shape[0]).all(1)
    tmpl_t = np.concatenate([st_, fold_t[keep]]).astype(np.int32)
    used = np.zeros(tmpl.shape[0], bool)
    used[tmpl_t.ravel()] = True
    assert used.all()
    mo, algo, state = make_state(ctx, tmpl, tmpl_t, tv, tt, rank=12)
    cp, w = algo.surfaceCorrespondence(state)
    ocp, ow, _ = go.surface_correspondence(np.asarray(state.general.fit), tmpl_t, tv, tt)
    assert np.array_equal(w, ow), int((w != ow).sum())
    assert np.abs(cp - ocp).max() < 1e-10 * 40.0
    # all three rules are exercised
    nn_idx, _, _ = go.icp_closest_point(ocp, tv)
    bnd = go.boundary_vertices(tv.shape[0], tt)
    nt, ng = go.vertex_normals(np.asarray(state.general.fit), tmpl_t), go.vertex_normals(tv, tt)
    opposite = (nt * ng[nn_idx]).sum(1) < 0
    assert bnd[nn_idx].any() and (opposite & ~bnd[nn_idx]).any()
    assert ((ow == 0) & ~bnd[nn_idx] & ~opposite).any()         # rejected by the self-intersection rule only
    assert (ow == 1).any()
    algo.close()


def oracle_state_of(g, transform):
    mp = g.modelParameters
    return go.State(alpha=np.asarray(mp.shape, dtype=np.float64).copy(), euler=(mp.rotation.phi, mp.rotation.theta, mp.rotation.psi),
                    center=np.asarray(mp.center, dtype=np.float64), translation=np.asarray(mp.translation, dtype=np.float64),
                    scale=float(mp.scale), sigma2=float(g.sigma2), fit=np.asarray(g.fit, dtype=np.float64).copy(),
                    iteration=int(g.iteration), status=int(g.status), global_transformation=transform, step_length=g.stepLength)


@pytest.mark.parametrize("transform,rank", [(0, 30), (1, 30), (1, 130)])
def test_icp_surface_updates_match_oracle(ctx, transform, rank):
    """Every update is checked against the oracle's update of the SAME input state: the accept / reject decisions are
    discontinuous in the fit, so two trajectories that differ by 1e-10 may legitimately part ways after a borderline pair flips;
    what must hold is that one update maps identical states to identical states."""
    import gingr_amd as ga
    ref, cells, target, tcells = femur()
    mo, algo, state = make_state(ctx, ref, cells, target, tcells, rank=rank)   # (rank 130: 0 / 1 weights through the wide Gram pass)
    if transform != 1:
        state = algo.createInitialState(ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells), target, state.config,
                                        transform=transform, targetCells=tcells)
    for it in range(4):
        st_in = oracle_state_of(state.general, transform)
        state = algo.update(state)
        st, (ocp, ow) = go.icp_surface_update(mo, cells, target, tcells, st_in, 20.0, 1.0, 30)
        assert state.general.status == st.status == 0
        assert rel(state.general.fit, st.fit) < 1e-5, (it, rel(state.general.fit, st.fit))
        assert abs(state.general.sigma2 - st.sigma2) < 1e-12
        assert 0 < ow.sum() < ow.shape[0]
    # and the registration actually moves towards the target surface
    _, d2_first = go.mesh_closest_point(mo.mean_mesh()[::10], target, tcells)
    _, d2_last = go.mesh_closest_point(np.asarray(state.general.fit)[::10], target, tcells)
    assert np.sqrt(d2_last).mean() < np.sqrt(d2_first).mean()
    algo.close()


def test_surface_icp_argument_errors(ctx):
    import gingr_amd as ga
    ref, cells, target, tcells = femur()
    mo = model_over(ref[:200], None, 6)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(correspondenceMethod="TriangularClosestPoint")
    with pytest.raises(ValueError):                                     # no triangulations
        algo.createInitialState(ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam), target, cfg)
    bad = np.array([[0, 1, 5000]], dtype=np.int32)                      # vertex id out of range
    state = algo.createInitialState(ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=bad), target, cfg, targetCells=tcells)
    with pytest.raises(ga.GingrNativeError):
        algo.update(state)
    algo.close()


def test_probabilistic_surface_icp(ctx):
    """update(probabilistic = true) and logTransitionProbability with the surface correspondence."""
    ref, cells, target, tcells = femur()
    mo, algo, state = make_state(ctx, ref, cells, target, tcells, rank=20)
    s1 = algo.update(state)
    st_in = oracle_state_of(s1.general, 1)
    z = np.random.default_rng(11).standard_normal(mo.rank)
    s2 = algo.update(s1, probabilistic=True, rnd=np.random.default_rng(11))
    st2, (ocp, ow) = go.icp_surface_update(mo, cells, target, tcells, st_in, 20.0, 1.0, 30, z=z)
    assert s2.general.status == st2.status == 0
    assert rel(s2.general.fit, st2.fit) < 1e-5
    got = algo.logTransitionProbability(s1, s2)
    pids = np.flatnonzero(ow == 1.0)
    want = go.posterior_logpdf_of_mesh(mo, st_in, pids, ocp[pids], np.full(pids.shape[0], st_in.sigma2), mesh=st_in.fit)
    assert np.isfinite(got) and abs(got - want) < 1e-5 * abs(want), (got, want)
    algo.close()


def test_along_normal_flavour(ctx):
    """AlongNormalClosestPoint (ClosestPointRegistrator.scala:102-131): correspondences and one update against the oracle, on the
    femur pair (closed meshes) and on the open / folded synthetic pair (misses, boundary, opposite normals, self-intersection)."""
    import gingr_amd as ga
    for case in ("femur", "synthetic"):
        if case == "femur":
            ref, cells, target, tcells = femur()
            rank, pose = 20, ((0.02, -0.01, 0.015), (0.8, -1.0, 0.4))
        else:
            target, tcells = grid_mesh(24, 40.0, 6.0, 1)
            sv, st_ = grid_mesh(14, 46.0, 4.0, 2)
            sv = sv + np.array([3.0, -2.0, 5.0])
            fold = sv.copy()
            fold[:, 2] -= 2.5
            fold_t = st_[:, [0, 2, 1]] + sv.shape[0]
            ref = np.concatenate([sv, fold[: sv.shape[0] // 2]])
            cells = np.concatenate([st_, fold_t[(fold_t < ref.shape[0]).all(1)]]).astype(np.int32)
            rank, pose = 12, None
        mo = model_over(ref, cells, rank)
        model = ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells)
        algo = ga.IcpRegistration(ctx)
        cfg = ga.IcpConfiguration(maxIterations=30, initialSigma=20.0, endSigma=1.0, correspondenceMethod="AlongNormalClosestPoint")
        state = algo.createInitialState(model, target, cfg, targetCells=tcells, initial_pose=pose)
        cp, w = algo.surfaceCorrespondence(state)
        ocp, ow, _ = go.along_normal_correspondence(np.asarray(state.general.fit), cells, target, tcells)
        assert np.array_equal(w, ow), (case, int((w != ow).sum()))
        assert np.abs(cp - ocp).max() < 1e-9 * max(1.0, np.abs(target).max()), case
        assert 0 < w.sum() < w.shape[0], case
        # one update from the same state
        st_in = oracle_state_of(state.general, 1)
        s1 = algo.update(state)
        pids = np.flatnonzero(ow == 1.0)
        st1 = go.update_from_observations(mo, st_in, pids, ocp[pids], np.full(pids.shape[0], st_in.sigma2),
                                          go.icp_update_sigma2(st_in.sigma2, 20.0, 1.0, 30), None, None)
        assert s1.general.status == st1.status == 0 and rel(s1.general.fit, st1.fit) < 1e-5, case
        algo.close()


@pytest.mark.parametrize("case", ["inside", "offset", "flat"])
def test_along_normal_search_orders_and_culls_exactly(ctx, case):
    """The along-normal search visits the target's triangle tiles in shells round a workgroup's points and culls by the hits found so
    far (surface_line.hip line_nearest_kernel): a template well INSIDE the target (no hit in the first shells, both sides of the closed
    target pierced), one offset so that lines leave the target on one side only, and an exactly flat template (vertex normals exactly
    (0, 0, 1): the lines are parallel to an axis, the slab test's zero-direction branch) -- all against the oracle's exhaustive search."""
    import gingr_amd as ga
    rng = np.random.default_rng(7)
    if case == "flat":
        ref, cells = grid_mesh(40, 30.0, 0.0, 3)
        ref[:, 2] = 0.0
        target, tcells = grid_mesh(48, 45.0, 5.0, 4)
        target = target + np.array([0.7, -0.4, 3.0])
        rank = 10
    else:
        v, f = _icosphere(4)                      # 2 562 vertices, 5 120 triangles: 20 tiles, two groups of tile boxes
        bump = 1.0 + 0.1 * np.sin(3 * v[:, 0]) * np.cos(2 * v[:, 1]) + 0.05 * np.sin(5 * v[:, 2])
        target, tcells = v * 80.0 * bump[:, None], f
        ref, cells = (v * 35.0 if case == "inside" else v * 60.0 + np.array([30.0, -12.0, 8.0])), f
        rank = 12
    from gingr_amd import _native as nat
    mo = model_over(ref, cells, rank)
    model = ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells)
    ocp = ow = None
    for tri_grid in (1, 2):   # 1: these meshes are below the grid's size threshold -> the tile scan; 2: the walk over the triangle grid
        c = ga.Context(0)
        c.set_option(nat.OPT_TRI_GRID, tri_grid)
        algo = ga.IcpRegistration(c)
        cfg = ga.IcpConfiguration(maxIterations=30, initialSigma=20.0, endSigma=1.0, correspondenceMethod="AlongNormalClosestPoint")
        state = algo.createInitialState(model, target, cfg, targetCells=tcells)
        cp, w = algo.surfaceCorrespondence(state)
        if ocp is None:
            ocp, ow, _ = go.along_normal_correspondence(np.asarray(state.general.fit), cells, target, tcells)
        assert np.array_equal(w, ow), (case, tri_grid, int((w != ow).sum()))
        assert np.abs(cp - ocp).max() < 1e-9 * max(1.0, np.abs(target).max()), (case, tri_grid)
        assert w.sum() > 0, case
        algo.close()
        c.close()


@pytest.mark.parametrize("method", ["TriangularClosestPoint", "AlongNormalClosestPoint", "PointcloudClosestPoint"])
def test_reversed_correspondence_direction(ctx, method):
    """reverseCorrespondenceDirection = true (ICP.scala:46-48): per-target assignments and one update against the oracle."""
    import gingr_amd as ga
    ref, cells, target, tcells = femur()
    target, tcells = target[:], tcells
    mo = model_over(ref, cells, 16)
    model = ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam, cells=cells)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=30, initialSigma=20.0, endSigma=1.0, correspondenceMethod=method,
                              reverseCorrespondenceDirection=True)
    state = algo.createInitialState(model, target, cfg, targetCells=tcells, initial_pose=((0.01, 0.02, -0.01), (0.5, 0.3, -0.4)))
    tid, w = algo.reversedCorrespondence(state)
    otid, opts, ow = go.correspondence_reversal(np.asarray(state.general.fit), cells, target, tcells, method)
    assert np.array_equal(w, ow), (method, int((w != ow).sum()))
    assert np.array_equal(tid[ow == 1.0], otid[ow == 1.0]), method
    assert ow.sum() > 0 and np.bincount(otid[ow == 1.0]).max() > 1      # some template vertices receive several observations
    st_in = oracle_state_of(state.general, 1)
    s1 = algo.update(state)
    st1, _ = go.icp_reversed_update(mo, cells, target, tcells, st_in, 20.0, 1.0, 30, method)
    assert s1.general.status == st1.status == 0 and rel(s1.general.fit, st1.fit) < 1e-5, (method, rel(s1.general.fit, st1.fit))
    pairs = algo.getCorrespondence(state)
    assert np.array_equal(pairs.pids, otid[ow == 1.0]) and np.array_equal(pairs.points, target[ow == 1.0])
    algo.close()


def _icosphere(level):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, dtype=np.int32)


def test_benchmark_size_correspondence_against_sampled_oracle(ctx):
    """41k vertices / 82k triangles with a hole (boundary) in the target: the whole correspondence (closest surface point,
    nearest target vertex, boundary / opposite-normal / self-intersection rejections) of the device against the oracle's rules
    evaluated for 1 200 sampled template vertices -- closest points through the C brute force, line tests through the numpy
    restatement over ALL 82k template triangles."""
    import gingr_amd as ga
    from oracle import c_oracle as co
    verts, cells = _icosphere(6)
    ref = verts * 80.0
    bump = 1.0 + 0.08 * np.sin(3 * verts[:, 0]) * np.cos(2 * verts[:, 1]) + 0.05 * np.sin(5 * verts[:, 2])
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    tgt = (ref * bump[:, None]) @ R.T + np.array([1.5, -1.0, 0.5])
    tcells = cells[~np.all(verts[cells][:, :, 2] > 0.93, axis=1)]              # a hole around the north pole: boundary vertices
    M = ref.shape[0]
    rng = np.random.default_rng(3)
    model = ga.PointDistributionModel(ref, np.zeros_like(ref), np.linalg.qr(rng.normal(size=(3 * M, 4)))[0], np.ones(4), cells=cells)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=10, initialSigma=10.0, endSigma=1.0, correspondenceMethod="TriangularClosestPoint")
    state = algo.createInitialState(model, tgt, cfg, targetCells=tcells)
    cp, w = algo.surfaceCorrespondence(state)
    # the fused update at this size against the oracle's update from the SAME correspondences (its own Python search over 41k x 82k
    # would take minutes; the correspondences themselves are checked on the sample below): Gram, solve, projections, pose, sigma2
    st_in = oracle_state_of(state.general, 1)
    new_state = algo.update(state)
    mo = go.PDM(ref=ref, mean=np.zeros_like(ref), U=np.asarray(model.basis), lam=np.ones(4))
    pids = np.flatnonzero(w == 1.0)
    st = go.update_from_observations(mo, st_in, pids, cp[pids], np.full(pids.shape[0], st_in.sigma2),
                                     go.icp_update_sigma2(st_in.sigma2, 10.0, 1.0, 10), None)
    assert new_state.general.status == st.status == 0
    assert rel(new_state.general.fit, st.fit) < 1e-6 and abs(new_state.general.sigma2 - st.sigma2) < 1e-12
    assert rel(new_state.general.modelParameters.shape, st.alpha) < 1e-5
    algo.close()
    # oracle on a sample (go.surface_correspondence, ClosestPointRegistrator.scala:75-100, restricted to `ids`)
    ids = np.sort(np.concatenate([rng.choice(M, 1000, replace=False), np.flatnonzero(verts[:, 2] > 0.9)[:200]]))
    ocp, od2, _ = co.mesh_closest_point(ref[ids], tgt, tcells)
    assert np.abs(cp[ids] - ocp).max() < 1e-9
    nn_idx = co.nn(ocp, tgt)[0]
    bnd = go.boundary_vertices(tgt.shape[0], tcells)
    cn_t, cn_g = go.cell_normals(ref, cells), go.cell_normals(tgt, tcells)
    n_tmpl, n_tgt = np.zeros_like(ref), np.zeros_like(tgt)
    cnt_t, cnt_g = np.zeros(M), np.zeros(tgt.shape[0])
    for k in range(3):                                                       # vertex_normals, vectorised (same sums, index order)
        np.add.at(n_tmpl, cells[:, k], cn_t), np.add.at(cnt_t, cells[:, k], 1.0)
        np.add.at(n_tgt, tcells[:, k], cn_g), np.add.at(cnt_g, tcells[:, k], 1.0)
    n_tmpl /= np.maximum(cnt_t, 1)[:, None]
    n_tgt /= np.maximum(cnt_g, 1)[:, None]
    want = np.ones(ids.shape[0])
    unsure = np.zeros(ids.shape[0], dtype=bool)
    for q, i in enumerate(ids):
        j = int(nn_idx[q])
        dotn = float(n_tmpl[i] @ n_tgt[j])
        if bnd[j]:
            want[q] = 0.0
        elif dotn < 0:
            want[q] = 0.0
        else:
            v = ref[i] - ocp[q]
            ips = go.line_mesh_intersections(ref[i], v, ref, cells)
            keep = np.any(ips != ref[i], axis=1)
            if keep.any():
                dd = ips[keep] - ref[i]
                closest = np.sqrt((dd * dd).sum(1).min())
                vn = np.sqrt(v @ v)
                if closest < vn:
                    want[q] = 0.0
                unsure[q] = abs(closest - vn) < 1e-9 * max(vn, 1e-300)
        unsure[q] |= abs(dotn) < 1e-12
    assert bnd.any() and (want == 0).sum() > 20 and (want == 1).sum() > 500
    differ = (w[ids] != want) & ~unsure
    assert not differ.any(), (ids[differ][:10], w[ids][differ][:10], want[differ][:10])


def test_triangle_grid_search_is_bit_identical_to_the_tile_scan():
    """GINGR_OPT_TRI_GRID: the closest surface point searched over a grid of the (fixed) target triangles, warm-started from the
    previous iteration, with the masked tile scan for what the grid cannot certify -- same closest points, same weights, same
    trajectory bit for bit as the tile scan alone (0).  2 forces the grid on this small mesh (1, the default, takes it from 16 384
    target triangles on); the sphere pair below is large enough for the default."""
    import gingr_amd as ga
    from gingr_amd import _native as nat
    ref, cells, target, tcells = femur()
    out = []
    for tri_grid in (0, 2):
        c = ga.Context(0)
        c.set_option(nat.OPT_TRI_GRID, tri_grid)
        assert c.get_option(nat.OPT_TRI_GRID) == tri_grid
        mo, algo, state = make_state(c, ref, cells, target, tcells, rank=20, initial_pose=((0.02, -0.03, 0.01), (1.0, -2.0, 0.5)))
        for _ in range(5):
            state = algo.update(state)
        cp, w = algo.surfaceCorrespondence(state)
        out.append((np.array(state.general.fit), cp.copy(), w.copy(), state.general.sigma2))
        algo.close()
        c.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3]


def test_triangle_grid_default_on_a_large_mesh_equals_the_tile_scan():
    """20 480 target triangles (icosphere level 5): the default takes the grid; wide balls at the start (flagged queries go to the masked
    tile scan), narrow ones later; a few huge triangles would go to the short list (none here).  Bit-identical to the tile scan."""
    import gingr_amd as ga
    from gingr_amd import _native as nat
    tv, tt = _icosphere(5)
    rv, rt = _icosphere(4)
    target = 30.0 * tv * (1.0 + 0.05 * np.sin(3.0 * tv[:, :1]) * np.cos(2.0 * tv[:, 1:2]))
    ref = 29.0 * rv
    assert tt.shape[0] >= 16384
    out = []
    for tri_grid in (0, 1):
        c = ga.Context(0)
        c.set_option(nat.OPT_TRI_GRID, tri_grid)
        mo, algo, state = make_state(c, ref, rt, target, tt, rank=16, initial_pose=((0.03, -0.02, 0.01), (0.8, -0.5, 0.3)), sigma=(4.0, 1.0))
        for _ in range(6):
            state = algo.update(state)
        cp, w = algo.surfaceCorrespondence(state)
        out.append((np.array(state.general.fit), cp.copy(), w.copy(), state.general.sigma2))
        algo.close()
        c.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and out[0][2].sum() > 0


def test_triangle_grid_with_wide_triangles_and_a_flat_mesh_equals_the_tile_scan():
    """The corners of the grid's binning: a few triangles far wider than a cell (the short list every query tests), a target that is
    flat along one axis (one layer of cells), queries far outside the grid (clamped cells, big balls: flagged for the tile scan).
    Forced grid against the tile scan, bit for bit."""
    import gingr_amd as ga
    from gingr_amd import _native as nat
    tv, tt = _icosphere(4)
    target = 30.0 * tv
    n0 = target.shape[0]
    # two huge triangles cutting through the sphere's neighbourhood + a fan of three more sharing a far apex
    extra = np.array([[-80.0, -80.0, 31.0], [80.0, -80.0, 31.5], [0.0, 90.0, 30.5], [0.0, 0.0, 140.0]])
    target = np.concatenate([target, extra])
    tt = np.concatenate([tt, np.array([[n0, n0 + 1, n0 + 2], [n0, n0 + 1, n0 + 3], [n0 + 1, n0 + 2, n0 + 3], [n0 + 2, n0, n0 + 3]],
                                      dtype=np.int32)])
    rv, rt = _icosphere(3)
    cases = [(28.0 * rv, rt, target, tt, ((0.02, -0.01, 0.03), (0.5, -0.4, 2.5)))]
    gv, gt = grid_mesh(40, 50.0, 0.0, 3)                      # a flat sheet as target, the template hovering over it and beyond it
    gv[:, 2] = 0.0
    sv, st = grid_mesh(24, 70.0, 2.0, 4)
    cases.append((sv + np.array([0.0, 0.0, 1.5]), st, gv, gt, ((0.0, 0.0, 0.02), (0.3, 0.2, 0.0))))
    for ref, cells, tgt, tcells, pose in cases:
        out = []
        for tri_grid in (0, 2):
            c = ga.Context(0)
            c.set_option(nat.OPT_TRI_GRID, tri_grid)
            mo, algo, state = make_state(c, ref, cells, tgt, tcells, rank=12, initial_pose=pose, sigma=(4.0, 1.0))
            for _ in range(4):
                state = algo.update(state)
            cp, w = algo.surfaceCorrespondence(state)
            out.append((np.array(state.general.fit), cp.copy(), w.copy()))
            algo.close()
            c.close()
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("rank", [40, 130])
def test_gram_downdate_equals_the_pass_over_the_basis(ctx, rank):
    """GINGR_OPT_GRAM_DOWNDATE: with 0 / 1 weights the weighted Gram matrix is the model's moment minus the rows of the zero-weight
    vertices (rejected pairs, landmark vertices).  The exchange segment (Gram matrix + right-hand side) of the same state is the one
    the MFMA pass over the whole basis gives, up to the rounding of the subtraction -- with a quarter of the template rejected (open
    target) and with landmarks -- and so is the state after an update.  (Trajectories are not compared further: the self-intersection
    test keeps `intersection point != vertex` as an exact comparison, like the reference, and flips on last-bit differences.)"""
    import ctypes
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd.sharded import ShardedFitter, as_torch
    verts, cells = _icosphere(3)
    ref = np.asarray(verts, dtype=np.float64) * 60.0
    cells = np.asarray(cells, dtype=np.int32)
    rng = np.random.default_rng(5)
    bump = 1.0 + 0.1 * np.sin(4 * verts[:, 0]) * np.cos(3 * verts[:, 1])
    target = ref * bump[:, None] + np.array([1.0, -0.5, 0.8]) + rng.normal(0, 0.3, ref.shape)
    tcells = cells[~np.all(verts[cells][:, :, 2] > 0.55, axis=1)]       # a cap removed: the vertices over the hole map to its rim
    lm_pid = np.array([3, 77, 200], dtype=np.int32)
    states = ((np.zeros(rank), 6.0), (np.linspace(-0.3, 0.3, rank), 5.5))
    # (built once, on the session's context; rank 130: the downdate in 112-column patches against the wide Gram pass)
    model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=rank).Gaussian(30.0, 8.0).to_host()
    got = {}
    for val in (1, 0):
        c = ga.Context(0)
        c.set_option(nat.OPT_GRAM_DOWNDATE, val)
        assert c.get_option(nat.OPT_GRAM_DOWNDATE) == val
        f = ShardedFitter(c, model, target)
        f.set_meshes(cells, tcells)
        lx, lc = np.ascontiguousarray(target[lm_pid]), np.ascontiguousarray(np.tile(np.eye(3) * 0.5, (3, 1, 1)))
        assert f._lib.gingr_fitter_set_landmarks(f.handle, 3, nat.iptr(lm_pid), nat.dptr(lx), nat.dptr(lc)) == 0
        ip = nat.IcpParams(6.0, 1.0, 20)
        for k, (alpha, s2) in enumerate(states):
            f.set_state(alpha, s2, iteration=k)
            for ph in (0, 1):
                assert f._lib.gingr_fitter_icp_surface_phase_async(f.handle, ctypes.byref(ip), ph) == 0
            p, offs, cnts = ctypes.c_void_p(), (ctypes.c_int64 * nat.NUM_SEGMENTS)(), (ctypes.c_int64 * nat.NUM_SEGMENTS)()
            assert f._lib.gingr_fitter_exchange(f.handle, ctypes.byref(p), offs, cnts) == 0
            c.synchronize()
            w, cp = np.zeros(len(ref)), np.zeros((len(ref), 3))
            assert f._lib.gingr_fitter_get_surface_correspondence(f.handle, nat.dptr(cp), nat.dptr(w)) == 0
            seg = as_torch(p.value, offs[1] + cnts[1], 0).cpu().numpy()[offs[1]:].copy()      # (the whole exchange buffer from its base pointer)
            assert f._lib.gingr_fitter_icp_surface_phase_async(f.handle, ctypes.byref(ip), 2) == 0
            a1, sc1, fit1 = f.get_state()
            got[(val, k)] = (seg, w, a1.copy(), fit1.copy(), sc1.status)
        f.close()
        c.close()
    for k in range(len(states)):
        (sa, wa, aa, fa, sta), (sb, wb, ab, fb, stb) = got[(1, k)], got[(0, k)]
        assert np.array_equal(wa, wb) and 0.1 < 1.0 - wb.mean() < 0.6          # the same pairs, a good part of them rejected
        assert np.max(np.abs(sa - sb)) <= 1e-12 * np.max(np.abs(sb))
        assert sta == stb == 0
        assert np.max(np.abs(aa - ab)) <= 1e-10 * max(1.0, np.max(np.abs(ab))) and np.max(np.abs(fa - fb)) <= 1e-10 * np.max(np.abs(fb))


@pytest.mark.parametrize("zcut,lo,hi,rank", [(0.30, 0.45, 0.85, 40), (0.97, 0.95, 1.0, 40), (0.30, 0.45, 0.85, 130)])
def test_gram_downdate_leaves_to_the_pass_over_the_basis_when_many_rows_are_rejected(ctx, zcut, lo, hi, rank):
    """The device-side guard of GINGR_OPT_GRAM_DOWNDATE (rule served: ClosestPointRegistrator.scala:84-91 -- a pair
    whose target point lies on the boundary is rejected, ICP.scala:50 gives it weight 0).  A 41k template against a target that is
    only a CAP of the sphere: most template vertices map to the rim and are rejected.  By size (the default) the option is on at 41k
    rows, but with more than one zero-weight vertex in eight the downdate launch leaves at once and the weighted pass over the basis
    runs -- the SAME kernel on the same inputs as with the option off, so the exchange segment and the next state carry the same
    bits, and the iteration costs what the direct pass costs plus two empty launches."""
    import ctypes
    import json
    import os
    import time
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd.sharded import ShardedFitter, as_torch
    verts, cells = _icosphere(6)
    ref = np.asarray(verts, dtype=np.float64) * 60.0
    cells = np.asarray(cells, dtype=np.int32)
    assert len(ref) == 40962
    bump = 1.0 + 0.05 * np.sin(4 * verts[:, 0]) * np.cos(3 * verts[:, 1])
    target = ref * bump[:, None] + np.array([0.5, -0.3, 0.4])
    tcells = cells[np.all(verts[cells][:, :, 2] > zcut, axis=1)]             # only the cap above z = zcut is there
    model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=rank).Gaussian(30.0, 8.0).to_host()
    got, per_it = {}, {}
    for val in (-1, 0):
        c = ga.Context(0)
        c.set_option(nat.OPT_GRAM_DOWNDATE, val)
        f = ShardedFitter(c, model, target)
        f.set_meshes(cells, tcells)
        ip = nat.IcpParams(6.0, 1.0, 200)
        f.set_state(np.linspace(-0.2, 0.2, rank), 6.0)
        for ph in (0, 1):
            assert f._lib.gingr_fitter_icp_surface_phase_async(f.handle, ctypes.byref(ip), ph) == 0
        p, offs, cnts = ctypes.c_void_p(), (ctypes.c_int64 * nat.NUM_SEGMENTS)(), (ctypes.c_int64 * nat.NUM_SEGMENTS)()
        assert f._lib.gingr_fitter_exchange(f.handle, ctypes.byref(p), offs, cnts) == 0
        c.synchronize()
        w, cp = np.zeros(len(ref)), np.zeros((len(ref), 3))
        assert f._lib.gingr_fitter_get_surface_correspondence(f.handle, nat.dptr(cp), nat.dptr(w)) == 0
        seg = as_torch(p.value, offs[1] + cnts[1], 0).cpu().numpy()[offs[1]:].copy()
        assert f._lib.gingr_fitter_icp_surface_phase_async(f.handle, ctypes.byref(ip), 2) == 0
        a1, sc1, fit1 = f.get_state()
        got[val] = (seg, w, a1.copy(), fit1.copy(), sc1.status)
        best = float("inf")
        for _ in range(5):                                                   # iteration time: 20 updates in one native call, best of five
            f.set_state(np.linspace(-0.2, 0.2, rank), 6.0)
            c.synchronize()
            t0 = time.perf_counter()
            assert f._lib.gingr_fitter_update_icp_surface_async(f.handle, ctypes.byref(ip), 20) == 0
            c.synchronize()
            best = min(best, (time.perf_counter() - t0) / 20)
        per_it[val] = best
        f.close()
        c.close()
    (sa, wa, aa, fa, sta), (sb, wb, ab, fb, stb) = got[-1], got[0]
    rejected = 1.0 - wb.mean()
    assert np.array_equal(wa, wb) and lo < rejected < hi, rejected
    assert sta == stb == 0
    assert np.max(np.abs(sa - sb)) <= 1e-9 * np.max(np.abs(sb))             # (in fact the same bits: the same kernel ran)
    assert np.max(np.abs(aa - ab)) <= 1e-9 * max(1.0, np.max(np.abs(ab))) and np.max(np.abs(fa - fb)) <= 1e-9 * np.max(np.abs(fb))
    rec = {"rejected_fraction": rejected, "ms_per_iteration_guarded_default": per_it[-1] * 1e3, "ms_per_iteration_option_off": per_it[0] * 1e3,
           "extra_us": (per_it[-1] - per_it[0]) * 1e6}
    os.makedirs("gpurun_out", exist_ok=True)
    rec["rank"] = rank
    with open(f"gpurun_out/r06_gram_downdate_guard_zcut{zcut}_rank{rank}.json", "w") as fh:
        json.dump(rec, fh)
    # loose bound here (a wall-clock figure in a test); the measured difference is recorded above and in profiles/
    assert per_it[-1] <= 1.25 * per_it[0] + 10e-6, rec


@pytest.fixture(scope="module")
def sheet_queries():
    """16 385 queries against the 288-triangle sheet and their brute-force closest points, computed once: the special queries come
    first, so every prefix the test below takes holds them."""
    from oracle import c_oracle as co
    from tests.tri_grid_cases import sheet
    V, C = sheet()
    rng = np.random.default_rng(21)
    P = np.concatenate([V[:40],                                                   # exactly on vertices
                        0.5 * (V[C[:40, 0]] + V[C[:40, 1]]),                      # exactly on edges
                        (V[C[:40, 0]] + V[C[:40, 1]] + V[C[:40, 2]]) / 3.0,       # inside triangles
                        rng.uniform([-1.0, -1.0, -1.0], [2.0, 2.0, 1.0], (16385 - 120, 3))])   # within one sheet width of the sheet
    want_cp, want_d2, _ = co.mesh_closest_point(P, V, C)
    return V, C, P, want_cp, want_d2


@pytest.mark.parametrize("nq", [4096, 4097, 16384, 16385])
def test_tile_scan_instances_on_both_sides_of_their_query_count_thresholds(ctx, sheet_queries, nq):
    """The tile scan holds 16, 8 or 4 copies of a query per workgroup, chosen by the number of queries (surface.h: surface_h, up to
    4 096 -> 16, up to 16 384 -> 8, else 4): every instance, on a mesh whose last tile (32 of 256 triangles) and last quarter are
    partial, against the brute-force oracle (tolerances of test_closest_points_with_triangle_and_barycentric_weights, extent 1)."""
    V, C, P, want_cp, want_d2 = sheet_queries
    assert C.shape == (288, 3) and P.shape == (16385, 3)
    cp, d2, tid, bary = ctx.mesh_closest_points(P[:nq], V, C)
    assert np.allclose(cp, want_cp[:nq], atol=1e-10) and np.allclose(d2, want_d2[:nq], atol=1e-9)
    assert tid.min() >= 0 and tid.max() < C.shape[0]
    rebuilt = (bary[:, :, None] * V[C[tid]]).sum(1)                               # the weights reproduce the closest point
    assert np.allclose(rebuilt, cp, atol=1e-10)
