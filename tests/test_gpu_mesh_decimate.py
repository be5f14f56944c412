"""gingr_mesh_decimate on the device against the definition it has to reproduce, gingr_amd.simple.cluster_decimate (host numpy,
unchanged): np.array_equal on the kept vertices and on the cells, so no tolerance.  The inputs are those of tests/decimate_restatement.py
(test_mesh_decimate_host.py pins the kernels' arithmetic order against the same definition on them); what each is there for:

  femur fixture, the whole range of n_target       identity at and above the vertex count
  femur as a point cloud                           out_triangles == NULL
  random clouds of 1 .. 1 025 points               wave / workgroup / scan-tile edges
  integer lattice, also far from the origin        exact ties of d2 -> lowest index; count plateaus; subtraction at a large offset
  300 points on 40 positions                       no cube size is ever accepted -> the cells of lo
  identical / collinear / coplanar points          extent 0, degenerate axes
  repeated and collapsing triangles                the first of a corner set stays, order preserved
  224 x 224 surface (50 176 / 99 458)              many workgroups in the sort, the scans and both tables; runs of ~500 per cluster
  ... twice, and after an unrelated call           no dependence on the arrival order of atomics or on stale tables
  bad arguments                                    error code and text; the context stays usable"""
import os

import numpy as np
import pytest

from tests import decimate_restatement as dr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def same(ctx, vertices, cells, n_target):
    """Context.mesh_decimate and the decimator built on it, against the definition."""
    from gingr_amd.simple import cluster_decimate, device_decimate
    want_v, want_c = cluster_decimate(vertices, cells, n_target)
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    kept, got_c, h = ctx.mesh_decimate(v, cells, n_target)
    assert kept.dtype == np.int32 and np.all(np.diff(kept) > 0)                       # ascending original indices
    assert np.array_equal(v[kept], want_v), (n_target, kept.shape, want_v.shape)
    if cells is None:
        assert got_c is None and want_c is None
    else:
        assert got_c.dtype == np.int32 and got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (n_target, got_c.shape, want_c.shape)
    assert (h == 0.0) == (n_target >= v.shape[0])
    dv, dc = device_decimate(ctx)(vertices, cells, n_target)
    assert np.array_equal(dv, want_v) and (dc is None if cells is None else np.array_equal(dc, want_c))
    return kept, got_c, h


@pytest.fixture(scope="module")
def femur():
    return dr.femur()


@pytest.mark.parametrize("n_target", dr.FEMUR_TARGETS)
def test_femur(ctx, femur, n_target):
    v, c = femur
    kept, got_c, h = same(ctx, v, c, n_target)
    if n_target >= v.shape[0]:
        assert np.array_equal(kept, np.arange(v.shape[0])) and np.array_equal(got_c, c)
    else:
        # the cube size is the one the host recurrence chooses from the same counts, to the bit
        lo = v.min(axis=0)
        count = lambda mid: np.unique(np.floor((v - lo) / mid).astype(np.int64), axis=0).shape[0]
        want_h, steps, _, _ = dr.bisect(float(np.max(v.max(axis=0) - lo)), count, n_target)
        assert h == want_h and steps == 15


def test_femur_as_a_point_cloud(ctx, femur):
    for n_target in (100, 1000):
        same(ctx, femur[0], None, n_target)


@pytest.mark.parametrize("n", dr.CLOUD_SIZES)
def test_random_clouds(ctx, n):
    for n_target in dr.cloud_targets(n):
        same(ctx, dr.cloud(n), None, n_target)


@pytest.mark.parametrize("shifted", (False, True))
def test_lattice_ties_go_to_the_lowest_index(ctx, shifted):
    v = dr.lattice(shifted)
    sizes = [same(ctx, v, None, n_target)[0].shape[0] for n_target in dr.LATTICE_TARGETS]
    assert sizes == [8, 27, 125]


def test_no_cube_size_is_accepted(ctx):
    v = dr.repeated_positions()
    kept, _, h = same(ctx, v, None, 100)
    assert kept.shape[0] == 40 and h == float(np.max(v.max(0) - v.min(0))) * 1e-6


@pytest.mark.parametrize("kind,n_target", dr.DEGENERATE)
def test_degenerate_extents(ctx, kind, n_target):
    kept, _, h = same(ctx, dr.degenerate(kind), None, n_target)
    if kind == "identical":
        assert kept.tolist() == [0] and h == 1e-6


def test_repeated_and_collapsing_triangles(ctx):
    v, tri = dr.repeated_triangles()
    kept, got_c, _ = same(ctx, v, tri, 6)
    nearest = ((v[:, None, :] - v[kept][None, :, :]) ** 2).sum(-1).argmin(1)
    assert np.array_equal(nearest, np.repeat(np.arange(6), 4))
    assert np.array_equal(got_c, nearest[tri[[0, 3, 4, 5, 9]]])
    _, all_c, _ = same(ctx, v, tri, v.shape[0])                                        # the identity drops nothing
    assert np.array_equal(all_c, tri)


# ---------------------------------------------------------------------------------------------------------------- the 50k surface
@pytest.fixture(scope="module")
def surface():
    """The mesh and the definition's answer at both sizes, computed once (a second of host time each)."""
    from gingr_amd.simple import cluster_decimate
    v, tri = dr.grid_surface(224)
    assert v.shape == (50176, 3) and tri.shape == (99458, 3)
    return v, tri, {n_target: cluster_decimate(v, tri, n_target) for n_target in (100, 5000)}


def check_surface(ctx, surface, n_target):
    v, tri, want = surface
    kept, c, h = ctx.mesh_decimate(v, tri, n_target)
    assert np.array_equal(v[kept], want[n_target][0]) and np.array_equal(c, want[n_target][1]) and h > 0.0
    return kept, c, h


@pytest.mark.parametrize("n_target", (100, 5000))
def test_surface_of_fifty_thousand_vertices(ctx, surface, n_target):
    kept, _, _ = check_surface(ctx, surface, n_target)
    assert n_target <= kept.shape[0] < 1.3 * n_target + 30


def test_repeated_calls_and_an_unrelated_call_in_between(ctx, surface):
    v, tri, _ = surface
    first = check_surface(ctx, surface, 5000)
    second = check_surface(ctx, surface, 5000)
    ctx.nn(v[:300], v[::7])                                                            # other work on the same context and stream
    check_surface(ctx, surface, 100)
    third = check_surface(ctx, surface, 5000)
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and first[2] == other[2]


def test_one_read_back_per_step_gives_the_same_result(ctx, surface, femur):
    """GINGR_OPT_DECIMATE_BATCH: the bisection's steps enqueued sixteen at a time (default) or one per read-back of the control block."""
    from gingr_amd import _native as nat
    assert ctx.get_option(nat.OPT_DECIMATE_BATCH) == 16
    try:
        for batch in (1, 7, 60):
            ctx.set_option(nat.OPT_DECIMATE_BATCH, batch)
            check_surface(ctx, surface, 100)
            same(ctx, femur[0], femur[1], 400)
    finally:
        ctx.set_option(nat.OPT_DECIMATE_BATCH, 16)


def test_bad_arguments_leave_the_context_usable(ctx, femur):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    v, c = femur
    bad_v = v.copy()
    bad_v[17, 1] = np.nan
    inf_v = v.copy()
    inf_v[3, 2] = np.inf
    bad_c = c.copy()
    bad_c[5, 2] = v.shape[0]
    neg_c = c.copy()
    neg_c[0, 0] = -1
    for args, text in (((v, c, 0), "n_target"), ((bad_v, c, 100), "not finite"), ((inf_v, None, 100), "not finite"),
                       ((v, bad_c, 100), "out of range"), ((v, neg_c, 100), "out of range"), ((v, bad_c, 10 ** 6), "out of range"),
                       ((np.zeros((0, 3)), None, 1), "n_vertices")):
        with pytest.raises(ga.GingrNativeError) as e:
            ctx.mesh_decimate(*args)
        assert e.value.code == nat.ERR_BAD_ARGUMENT and text in str(e.value), str(e.value)
    same(ctx, v, c, 100)


# ---------------------------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def femur_pair(ctx):
    import gingr_amd as ga
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    m = np.load(os.path.join(HERE, "golden", "femur_mesh.npz"))
    ref, tgt = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
    model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.05).Gaussian(sigma=70.0, scaling=50.0).to_host()
    model.cells = m["femur_cells"]
    return model, ga.TriangleMesh3D(tgt, m["femur_target_cells"])


def test_decimated_state_is_the_same_with_either_decimator(ctx, femur_pair):
    import gingr_amd as ga
    from gingr_amd.simple import cluster_decimate
    model, target = femur_pair
    states = []
    for decimate in (None, cluster_decimate):
        reg = ga.GingrInterface(ctx, model, target, decimate=decimate, verbose=False).CPD(ga.CpdConfiguration(maxIterations=5))
        assert (reg.decimate is cluster_decimate) == (decimate is not None)
        states.append(reg._decimateState(None, ga.GlobalTranformationType.RigidTransforms, 400, 400))
    a, b = states
    assert 400 <= a.model.numberOfPoints < 1622
    assert np.array_equal(a.model.reference, b.model.reference) and np.array_equal(a.model.cells, b.model.cells)
    assert a.model.cells.dtype == b.model.cells.dtype
    assert np.array_equal(a.target, b.target) and np.array_equal(a.targetCells, b.targetCells)
    assert np.array_equal(a.fit, b.fit) and a.sigma2 == b.sigma2


def test_evaluator_decimates_for_number_of_points_for_comparison(ctx, femur_pair):
    import gingr_amd as ga
    from gingr_amd.sampling import IndependentPointDistanceEvaluator, SymmetricEvaluation
    from gingr_amd.simple import cluster_decimate
    model, target = femur_pair
    algo = ga.IcpRegistration(ctx)
    state = algo.createInitialState(model, target.points, ga.IcpConfiguration(maxIterations=3, initialSigma=1.0, endSigma=1.0),
                                    targetCells=target.cells)
    g = state.general
    fv, _ = cluster_decimate(g.fit, g.model.cells, 60)
    tv, _ = cluster_decimate(g.target, g.targetCells, 60)
    assert 60 <= fv.shape[0] < 200 and 60 <= tv.shape[0] < 200
    want = IndependentPointDistanceEvaluator(algo, state, 5.0, SymmetricEvaluation, None, int(fv.shape[0]), tv)
    got = IndependentPointDistanceEvaluator(algo, state, 5.0, SymmetricEvaluation, 60)
    assert got.modelPointCount == want.modelPointCount and np.array_equal(got.targetPoints, want.targetPoints)
    assert got.logValue(state) == want.logValue(state) and np.isfinite(got.logValue(state)) and got.logValue(state) != 0.0
    moved = algo.update(state)
    assert got.logValue(moved) == want.logValue(moved) != got.logValue(state)
    for kw in (dict(modelPointCount=10), dict(targetPoints=tv)):
        with pytest.raises(ValueError):
            IndependentPointDistanceEvaluator(algo, state, 5.0, SymmetricEvaluation, 60, **kw)
    algo.close()
