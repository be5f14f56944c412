"""gingr_cloud_fpfh, gingr_feature_match, gingr_rigid_poses_from_triples (gingr_amd/csrc/feature_align.hip), gingr_rigid_search_poses
(rigid_search.hip) and classic.FeatureRigidAlignment against the definitions restated in tests/feature_alignment_restatement.py.
Every device call is made twice and asserted bit-equal.

Descriptor.  counts and valid are integers: they equal the restatement's exactly at every point none of whose pairs is EDGE-NEAR (a
feature within 16 DELTA of a bin edge, DELTA the float64 / longdouble spread of the restatement's pair features); a point with
edge-near pairs may differ by those pairs only, and at most 1 % of the points may be excused.  fpfh is judged against the longdouble
route run on the device's own counts: |difference| <= 100 * 256 * 2^-53 per bin (at most 65 non-negative terms, each with a square
root and a division, then a rescaling over 11 words).
Match.  Indices and d2 bit for bit: the expression is fixed, so there is no tolerance.
Triples.  Per triple MARGIN = 1000 (tests/test_gpu_rigid_search.py: two correct routes) times the float64 / longdouble spread of the
restatement on that triple, floored at one unit of rounding of the quantity's scale.
Search from poses.  Given the start poses of gingr_rigid_search -- (R0, mean Y - R0 mean X) in the order include/gingr_hip.h fixes:
feature_alignment_restatement.start_poses -- every output has gingr_rigid_search's bits.  rigid_search_restatement.start_poses forms
R0 mean X through numpy's matrix product, whose order is the BLAS library's; its poses that agree with the header's order to the bit
(59 of 64 on the femur pair) are checked as well, the others start an ulp apart and are only counted.
End to end.  FeatureRigidAlignment.register on the eight partial cases (template femur[::4], the target's lower third cut away, with
and without the 72 clutter points): the bound is 3 degrees from the pose trimmed ICP reaches from the true alignment.
On an MI355X (2026-10-21) the largest angle was 0.170 degrees (plain; 0.028 with clutter), the same for every seed; in all sixteen
cases the device's matches, kept triples, winning triple and inlier count were the restatement's.  Other figures of that run: no
edge-near pair on any descriptor input, fpfh 2.4e-14 from the longdouble judge (bound 2.8e-12), triples at 0.012 of their tolerance,
an exact copy's rotation recovered to 1.3e-13."""
import numpy as np
import pytest

from tests import feature_alignment_restatement as fa
from tests import rigid_search_restatement as rs

pytestmark = pytest.mark.gpu

MARGIN = 1000.0
EPS = float(np.finfo(np.float64).eps)
FPFH_TOL = 100 * 256 * 2.0 ** -53
FIELDS = ("rotations", "translations", "scores", "kept", "failed")


# ------------------------------------------------------------------------------------------------ descriptor
def device_fpfh(ctx, x, n, k, radius):
    a, b = ctx.cloud_fpfh(x, n, k, radius), ctx.cloud_fpfh(x, n, k, radius)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)                                                          # two calls: the same bits
    assert a[0].shape == (x.shape[0], 33) and a[1].dtype == np.int32 and a[2].dtype == np.int32
    return a


def check_descriptor(ctx, name, x, n, k, radius):
    x = np.ascontiguousarray(x, dtype=np.float64)
    fpfh, counts, valid = device_fpfh(ctx, x, n, k, radius)
    want = fa.fpfh(x, n, k, radius)
    idx, d2 = ctx.cloud_knn(x, k)
    assert np.array_equal(idx, want["idx"]) and np.array_equal(d2, want["d2"])               # the lists both sides walk
    near = (fa.edge_near(want["alpha"], want["phi"], want["theta"]) & want["counted"]).sum(1)
    clean = near == 0
    print(f"{name}: {int((~clean).sum())} of {x.shape[0]} points have an edge-near pair; counted pairs {int(want['valid'].sum())}")
    assert (~clean).sum() <= 0.01 * x.shape[0]
    assert np.array_equal(counts[clean], want["counts"][clean]) and np.array_equal(valid, want["valid"])
    for i in np.nonzero(~clean)[0]:                                                          # such a pair may sit in the bin next door
        diff = np.abs(counts[i].astype(np.int64) - want["counts"][i]).reshape(3, 11).sum(1)
        assert (diff <= 2 * near[i]).all() and (counts[i].reshape(3, 11).sum(1) == valid[i]).all()
    judge = fa.fpfh_from_counts(counts, valid, want["idx"], want["d2"], want["neighbour"], np.longdouble)
    worst = float(np.abs(fpfh.astype(np.longdouble) - judge).max())
    print(f"{name}: fpfh against longdouble on the device's counts {worst:.3g} (bound {FPFH_TOL:.3g})")
    assert np.isfinite(fpfh).all() and worst <= FPFH_TOL
    return fpfh, counts, valid, want


def random_cloud(N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 10.0, (N, 3)) + [50.0, -20.0, 5.0], rng.normal(size=(N, 3))          # (normals of any length: normalised on upload)


def test_descriptor_three_points(ctx):
    x, n = random_cloud(3, 1)
    _, _, valid, _ = check_descriptor(ctx, "N = k = 3", x, n, 3, 100.0)
    assert valid.tolist() == [2, 2, 2]


def test_descriptor_one_point_left_out_of_every_list(ctx):
    x, n = random_cloud(65, 2)
    _, _, valid, _ = check_descriptor(ctx, "N = 65, k = 64", x, n, 64, 1000.0)
    assert (valid == 63).all()
    check_descriptor(ctx, "N = 65, k = 64, radius 12", x, n, 64, 12.0)                       # the radius cuts the lists


def test_descriptor_radius_below_the_spacing(ctx):
    x, n = random_cloud(200, 3)
    spacing = float(np.sqrt(ctx.cloud_knn(x, 3)[1][:, 1].min()))
    fpfh, counts, valid, _ = check_descriptor(ctx, "radius below the spacing", x, n, 16, 0.5 * spacing)
    assert not fpfh.any() and not counts.any() and not valid.any()


def test_descriptor_duplicated_points(ctx):
    x, n = random_cloud(130, 4)
    x, n = np.concatenate([x, x[[5, 5, 77, 129]]]), np.concatenate([n, n[[5, 5, 77, 129]]])
    _, _, valid, want = check_descriptor(ctx, "four duplicated points", x, n, 32, 15.0)
    assert (want["d2"][5, :3] == 0).all() and not want["neighbour"][5, :3].any()             # the point and its two copies drop out
    assert valid[5] == valid[130] == valid[131]


def test_descriptor_a_third_of_the_normals_zero(ctx):
    x, n = random_cloud(300, 5)
    n[::3] = 0.0
    _, _, valid, want = check_descriptor(ctx, "a third of the normals zero", x, n, 24, 20.0)
    assert (valid[::3] == 0).all() and valid[1::3].sum() > 0
    assert (valid < want["neighbour"].sum(1))[1::3].any()                                     # pairs with a normal-less neighbour are skipped


def test_descriptor_flat_grid(ctx):
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    x = np.concatenate([g, np.zeros((64, 1))], axis=1)
    fpfh, counts, valid, _ = check_descriptor(ctx, "flat 8 x 8 grid", x, np.tile([0.0, 0.0, 1.0], (64, 1)), 64, 3.0)
    centre = np.zeros(33, dtype=bool)
    centre[[5, 16, 27]] = True
    assert (valid > 0).all() and (counts[:, ~centre] == 0).all() and (counts[:, centre] == valid[:, None]).all()
    assert (fpfh[:, ~centre] == 0).all() and np.abs(fpfh[:, centre] - 100.0).max() <= FPFH_TOL


def test_descriptor_neighbour_along_the_normal_is_skipped(ctx):
    x = np.array([[0.0, 0, 0], [0, 0, 2.0], [3.0, 0, 0], [0, 4.0, 0]])
    _, counts, valid, want = check_descriptor(ctx, "a neighbour along the normal", x, np.tile([0.0, 0.0, 1.0], (4, 1)), 3, 10.0)
    assert want["neighbour"][0].sum() == 2 and valid[0] == 1 and counts[0].sum() == 3


@pytest.fixture(scope="module")
def femur_target(ctx):
    _, tgt = rs.femur_pair()
    return tgt, ctx.cloud_normals(tgt, 12, viewpoint=tgt.mean(0))[0]


def test_descriptor_femur_target(ctx, femur_target):
    tgt, n = femur_target
    _, _, valid, _ = check_descriptor(ctx, "femur target, k = 64, radius 25", tgt, n, 64, 25.0)
    assert tgt.shape == (1622, 3) and valid.min() > 0


def test_descriptor_refusals(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    x, n = random_cloud(10, 6)

    def code(*a):
        with pytest.raises(ga.GingrNativeError) as e:
            ctx.cloud_fpfh(*a)
        return e.value.code

    assert code(x, n, 2, 5.0) == code(x, n, 65, 5.0) == code(x, n, 11, 5.0) == nat.ERR_BAD_ARGUMENT
    assert code(x, n, 5, 0.0) == code(x, n, 5, -1.0) == code(x, n, 5, float("nan")) == nat.ERR_BAD_ARGUMENT
    for bad in (float("nan"), float("inf")):
        xb, nb = x.copy(), n.copy()
        xb[3, 1] = nb[7, 2] = bad
        assert code(xb, n, 5, 5.0) == nat.ERR_NONFINITE and code(x, nb, 5, 5.0) == nat.ERR_NONFINITE


# ------------------------------------------------------------------------------------------------ match
def device_match(ctx, a, b):
    p, q = ctx.feature_match(a, b), ctx.feature_match(a, b)
    assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    return p


@pytest.mark.parametrize("M,N,D", [(1, 1, 1), (3, 257, 33), (300, 1025, 64), (65, 64, 33)])
def test_match_bit_for_bit(ctx, M, N, D):
    rng = np.random.default_rng(M + N + D)
    a, b = rng.uniform(0, 100.0, (M, D)), rng.uniform(0, 100.0, (N, D))
    idx, d2 = device_match(ctx, a, b)
    want_idx, want_d2 = fa.feature_match(a, b)
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)


def test_match_ties_go_to_the_lowest_index_and_equal_rows_give_zero(ctx):
    rng = np.random.default_rng(9)
    b = rng.uniform(0, 100.0, (1025, 33))
    b[[40, 700, 1024]] = b[7]                                                                # the copies lie in later tiles and chunks
    b[3] = b[900]
    a = np.concatenate([b[[7, 900, 1000]], rng.uniform(0, 100.0, (70, 33))])
    idx, d2 = device_match(ctx, a, b)
    want_idx, want_d2 = fa.feature_match(a, b)
    assert idx[:3].tolist() == [7, 3, 1000] and (d2[:3] == 0.0).all()
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)


def test_match_on_descriptors(ctx, femur_target):
    tgt, n = femur_target
    fb = ctx.cloud_fpfh(tgt, n, 64, 25.0)[0]
    femur = rs.femur_pair()[0]
    tpl = np.ascontiguousarray(femur[::4])
    f_a = ctx.cloud_fpfh(tpl, ctx.cloud_normals(tpl, 12, viewpoint=tpl.mean(0))[0], 64, 25.0)[0]
    for a, b in ((f_a, fb), (fb, f_a)):
        idx, d2 = device_match(ctx, a, b)
        want_idx, want_d2 = fa.feature_match(a, b)
        assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)


# ------------------------------------------------------------------------------------------------ triples
def device_triples(ctx, X, Y, tm, tt):
    p, q = ctx.rigid_poses_from_triples(X, Y, tm, tt), ctx.rigid_poses_from_triples(X, Y, tm, tt)
    assert np.array_equal(p[0], q[0], equal_nan=True) and np.array_equal(p[1], q[1])
    return p


def test_triples_against_the_restatement(ctx):
    rng = np.random.default_rng(21)
    X = rng.normal(0, 30.0, (300, 3)) + [200.0, -50.0, 10.0]
    Y = rng.normal(0, 30.0, (500, 3)) + [-40.0, 300.0, 80.0]
    H = 257                                                                                  # five workgroups of 64 lanes, the last one partial
    tm = np.stack([rng.choice(300, 3, replace=False) for _ in range(H)])
    tt = np.stack([rng.choice(500, 3, replace=False) for _ in range(H)])
    poses, deg = device_triples(ctx, X, Y, tm, tt)
    a, da = fa.poses_from_triples(X, Y, tm, tt)
    b, _ = fa.poses_from_triples(X, Y, tm, tt, np.longdouble)
    assert np.array_equal(deg, da) and not deg.any()
    scale = float(max(np.abs(X).max(), np.abs(Y).max()))
    spread = np.abs(a.astype(np.longdouble) - b).astype(np.float64)
    tol_r = MARGIN * np.maximum(spread[:, :9].max(1), EPS)
    tol_t = MARGIN * np.maximum(spread[:, 9:].max(1), EPS * scale)
    ratio_r, ratio_t = np.abs(poses[:, :9] - a[:, :9]).max(1) / tol_r, np.abs(poses[:, 9:] - a[:, 9:]).max(1) / tol_t
    print(f"triples: observed / tolerance rotation {ratio_r.max():.3g}, translation {ratio_t.max():.3g}")
    assert np.isfinite(poses).all() and ratio_r.max() <= 1.0 and ratio_t.max() <= 1.0
    R = poses[:, :9].reshape(-1, 3, 3)
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12


def test_triples_degenerate_are_flagged_and_nan(ctx):
    X = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 0], [5, 0, 1]]) * 10.0 + [7.0, 8.0, 9.0]
    Y = np.array([[0.0, 0, 0], [4, 0, 0], [0, 3, 0], [4, 0, 0], [1, 2, 3]]) * 10.0 - [3.0, 2.0, 1.0]
    tm = [[0, 1, 2], [0, 3, 3], [0, 3, 4], [0, 3, 4], [0, 3, 4]]                               # collinear; a repeated index; fine x 3
    tt = [[0, 1, 2], [0, 1, 2], [0, 1, 3], [0, 1, 1], [0, 1, 2]]                               # fine; fine; zero area (two equal points); repeat; fine
    poses, deg = device_triples(ctx, X, Y, tm, tt)
    want, dw = fa.poses_from_triples(X, Y, tm, tt)
    assert deg.tolist() == dw.tolist() == [True, True, True, True, False]
    assert np.isnan(poses[:4]).all() and np.isfinite(poses[4]).all()
    import gingr_amd as ga
    with pytest.raises(ga.GingrNativeError):
        ctx.rigid_poses_from_triples(X, Y, [[0, 1, 5]], [[0, 1, 2]])                          # an index out of range is refused


def test_triples_of_an_exact_rigid_copy_return_the_motion(ctx):
    """triangles with longest edge^2 / (2 area) <= 100: the rotation of a rank-two cross-covariance is determined to its condition
    times rounding, so the bound is MARGIN * EPS * 100 (times the coordinates' scale for the translation)"""
    rng = np.random.default_rng(22)
    X = rng.normal(0, 30.0, (200, 3)) + [200.0, -50.0, 10.0]
    R_true, t_true = rs.random_rotation(rng), np.array([-300.0, 40.0, 90.0])
    Y = X @ R_true.T + t_true
    tri = np.stack([rng.choice(200, 3, replace=False) for _ in range(400)])
    p = X[tri]
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 2] - p[:, 1]], axis=1)
    aspect = (e * e).sum(2).max(1) / np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
    tri = tri[aspect <= 100.0]
    assert tri.shape[0] > 200
    poses, deg = device_triples(ctx, X, Y, tri, tri)
    scale = float(max(np.abs(X).max(), np.abs(Y).max()))
    err_r, err_t = np.abs(poses[:, :9] - R_true.reshape(9)).max(), np.abs(poses[:, 9:] - t_true).max()
    print(f"exact copy: rotation error {err_r:.3g} (bound {MARGIN * EPS * 100:.3g}), translation error {err_t:.3g}")
    assert not deg.any() and err_r <= MARGIN * EPS * 100 and err_t <= MARGIN * EPS * 100 * scale


# ------------------------------------------------------------------------------------------------ search from poses
def run_poses(ctx, X, Y, poses, K, rho=1.0, distance=0.0, select=0):
    a = ctx.rigid_search_poses(X, Y, poses, K, rho, distance, select)
    b = ctx.rigid_search_poses(X, Y, poses, K, rho, distance, select)
    assert a.best == b.best
    for f in FIELDS + ("inliers",):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    return a


def search_case(which):
    if which == "small":
        rng = np.random.default_rng(19)
        X = rng.normal(0, 30.0, (7, 3)) + [200.0, -50.0, 10.0]
        Y = rng.normal(0, 30.0, (5, 3)) + [-40.0, 300.0, 80.0]
        return X, Y, np.stack([rs.random_rotation(rng) for _ in range(3)]), 2, 1.0
    tpl, Y, _, _ = rs.recovery_case(0)
    return tpl, Y, rs.rotation_samples(64), 3, 0.6


@pytest.mark.parametrize("which", ["small", "femur"])
def test_search_from_the_start_poses_has_the_bits_of_rigid_search(ctx, which):
    X, Y, R0, K, rho = search_case(which)
    assert (X.shape[0], Y.shape[0], R0.shape[0], K, rho) in ((7, 5, 3, 2, 1.0), (406, 1622, 64, 3, 0.6))
    want = ctx.rigid_search(X, Y, R0, K, rho)
    start = fa.start_poses(X, Y, R0)
    got = run_poses(ctx, X, Y, start, K, rho, 3.0, 0)
    assert got.best == want.best and got.score == want.score and np.array_equal(got.R, want.R) and np.array_equal(got.t, want.t)
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    # the numpy restatement's own start poses: bit-equal wherever its R0 @ mean X has the bits of the header's order
    theirs = np.stack([np.concatenate([R.reshape(9), t]) for R, t in rs.start_poses(X, Y, R0)])
    same = (theirs == start).all(1)
    print(f"{which}: {int(same.sum())} of {same.size} start poses of rigid_search_restatement.start_poses have the header's bits")
    assert same.sum() >= 0.75 * same.size
    other = run_poses(ctx, X, Y, theirs, K, rho, 3.0, 0)
    for f in FIELDS:
        assert np.array_equal(getattr(other, f)[same], getattr(want, f)[same]), f


def test_inliers_equal_the_count_from_the_returned_poses(ctx):
    X, Y, R0, K, rho = search_case("femur")
    for distance in (0.0, 3.0, 10.0, 1e6):
        got = run_poses(ctx, X, Y, fa.start_poses(X, Y, R0)[:9], K, rho, distance, 1)
        for s in range(9):
            R, t = got.rotations[s], got.translations[s]                                     # the pose kernel's expression, term by term
            p = np.stack([((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + t[a] for a in range(3)], axis=1)
            d2 = ctx.nn(p, Y)[1]
            assert got.inliers[s] == int((d2 <= distance * distance).sum()), (distance, s)
        assert got.inliers.dtype == np.int64 and (distance < 1e6 or (got.inliers == X.shape[0]).all())
        order = sorted(range(9), key=lambda s: (-int(got.inliers[s]), float(got.scores[s]), s))
        assert got.best == order[0] == fa.select_best(got.scores, got.inliers, got.failed, 1)


def test_select_by_inliers_and_its_tie_rule(ctx):
    X, Y, R0, _, _ = search_case("femur")
    start = fa.start_poses(X, Y, R0)
    base = run_poses(ctx, X, Y, start, 0, 1.0, 6.0, 1)
    by_score = run_poses(ctx, X, Y, start, 0, 1.0, 6.0, 0)
    assert by_score.best == int(np.argmin(base.scores)) and np.array_equal(by_score.inliers, base.inliers)
    w = base.best
    assert base.inliers[w] == base.inliers.max()
    # the winner repeated behind everything and in front: equal inliers and equal scores, the lowest index wins
    twice = run_poses(ctx, X, Y, np.concatenate([start, start[w:w + 1]]), 0, 1.0, 6.0, 1)
    assert twice.best == w and twice.inliers[64] == twice.inliers[w] and twice.scores[64] == twice.scores[w]
    front = run_poses(ctx, X, Y, np.concatenate([start[w:w + 1], start]), 0, 1.0, 6.0, 1)
    assert front.best == 0
    # equal inliers, different scores: with a distance that takes every point the smaller score decides
    everything = run_poses(ctx, X, Y, start, 0, 1.0, 1e6, 1)
    assert (everything.inliers == X.shape[0]).all() and everything.best == int(np.argmin(everything.scores))
    want = fa.search_poses(X, Y, start[:8], 0, 1.0, 6.0, 1)
    got = run_poses(ctx, X, Y, start[:8], 0, 1.0, 6.0, 1)
    assert np.array_equal(got.inliers, want["inliers"]) and got.best == want["best"]


def test_a_nan_start_pose_fails_and_leaves_its_neighbours_alone(ctx):
    X, Y, R0, K, rho = search_case("femur")
    start = fa.start_poses(X, Y, R0)[:5]
    clean = run_poses(ctx, X, Y, start, K, rho, 3.0, 1)
    dirty = start.copy()
    dirty[2, 4] = np.nan
    dirty[4, 11] = np.inf
    got = run_poses(ctx, X, Y, dirty, K, rho, 3.0, 1)
    assert got.failed.tolist() == [False, False, True, False, True] and got.best in (0, 1, 3)
    assert np.isinf(got.scores[[2, 4]]).all() and (got.kept[[2, 4]] == 0).all() and (got.inliers[[2, 4]] == 0).all()
    for f in FIELDS + ("inliers",):
        assert np.array_equal(getattr(got, f)[[0, 1, 3]], getattr(clean, f)[[0, 1, 3]]), f
    import gingr_amd as ga
    from gingr_amd import _native as nat
    with pytest.raises(ga.GingrNativeError) as e:
        ctx.rigid_search_poses(X, Y, dirty[[2, 4]], K, rho, 3.0, 1)                           # every pose failed
    assert e.value.code == nat.ERR_NONFINITE
    for bad in ((-1.0, 0), (float("nan"), 0), (3.0, 2), (3.0, -1)):
        with pytest.raises(ga.GingrNativeError) as e:
            ctx.rigid_search_poses(X, Y, start, K, rho, *bad)
        assert e.value.code == nat.ERR_BAD_ARGUMENT


def test_no_iteration_scores_the_poses_as_given(ctx):
    X, Y, R0, _, _ = search_case("small")
    start = fa.start_poses(X, Y, R0)
    got = run_poses(ctx, X, Y, start, 0, 1.0, 50.0, 1)
    want = fa.search_poses(X, Y, start, 0, 1.0, 50.0, 1)
    assert np.array_equal(got.rotations.reshape(-1, 9), start[:, :9]) and np.array_equal(got.translations, start[:, 9:])
    assert np.allclose(got.scores, want["scores"], rtol=1e-12, atol=0) and np.array_equal(got.inliers, want["inliers"])
    assert got.best == want["best"] and isinstance(got.inliers, np.ndarray)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def bases():
    part = fa.partial_target(rs.femur_pair()[1])
    return {clutter: rs.icp_from(rs.recovery_case(0, clutter)[0], part, np.eye(3), np.zeros(3), 50, 0.6)[0] for clutter in (False, True)}


@pytest.mark.parametrize("clutter", [False, True])
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_partial_target_is_recovered(ctx, bases, seed, clutter):
    from gingr_amd import classic
    tpl, Y, R_true, _, _ = fa.partial_case(seed, clutter)
    align = classic.FeatureRigidAlignment(ctx, tpl, 25.0, inlierDistance=3.0)
    aligned = align.register(Y)
    R, t = align.transform
    angle = rs.angle_deg(R, R_true @ bases[clutter])
    hyp = rs.angle_deg(align.searchResult.R, R_true)
    print(f"seed {seed} clutter {clutter}: hypothesis {hyp:.2f} deg from the truth, refined {angle:.3f} deg from the base pose; {align.info}")
    assert angle <= 3.0
    assert np.abs(aligned - (tpl @ R.T + t)).max() <= 1e-9 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    assert set(align.info) == {"matches", "mutual", "drawn", "kept", "degenerate", "inliers"} and align.info["drawn"] == 2000
    # the restatement on the device's own descriptors: where its matches are the device's, its triple is too
    x = align.searchPoints()
    fx = ctx.cloud_fpfh(x, ctx.cloud_normals(x, 12, viewpoint=x.mean(0))[0], 64, 25.0)[0]
    fy = ctx.cloud_fpfh(Y, ctx.cloud_normals(Y, 12, viewpoint=Y.mean(0))[0], 64, 25.0)[0]
    want = fa.align(tpl, Y, 25.0, descriptors=(fx, fy))
    if np.array_equal(want["match"], align.matches):
        assert np.array_equal(want["triples"], align.triples) and want["info"]["mutual"] == align.info["mutual"]
        assert np.array_equal(want["triples"][want["best"]], align.triples[align.searchResult.best])
        assert want["info"]["inliers"] == align.info["inliers"]
    else:
        print(f"seed {seed} clutter {clutter}: the matches differ from the restatement's; its triple is not compared")


def test_alignment_with_given_normals_and_the_default_distance(ctx):
    from gingr_amd import classic
    tpl, Y, R_true, _, _ = fa.partial_case(3)
    ny = ctx.cloud_normals(Y, 12, viewpoint=Y.mean(0))[0]
    nt = ctx.cloud_normals(tpl, 12, viewpoint=tpl.mean(0))[0]
    given = classic.FeatureRigidAlignment(ctx, tpl, 25.0, inlierDistance=3.0, templateNormals=nt)
    plain = classic.FeatureRigidAlignment(ctx, tpl, 25.0, inlierDistance=3.0)
    assert np.array_equal(given.register(Y, ny), plain.register(Y))                           # the normals it would have made itself
    sub = classic.FeatureRigidAlignment(ctx, tpl, 25.0, maxPoints=250, hypotheses=1000)       # every second point; the default distance
    out = sub.register(Y)
    assert sub.searchPoints().shape == (203, 3) and out.shape == tpl.shape and np.isfinite(out).all()
    assert sub.info["matches"] == 203 and sub.info["drawn"] == 1000
