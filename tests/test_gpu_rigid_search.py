"""gingr_rigid_search (gingr_amd/csrc/rigid_search.hip) against the definition restated in tests/rigid_search_restatement.py.  Every
device run is made twice and asserted bit-equal (run()).

Tolerance.  Device and restatement are two correct routes (block partials and the polar iteration there, numpy sums and an SVD here):
the tolerance of a case is MARGIN = 1000 (the repository's rule for two routes) times the float64 / longdouble spread of
the restatement on the same input, the spread floored at one unit of rounding of the quantity's scale (1 for a rotation entry, the
largest |coordinate| for a translation or a score).  Each check prints observed / tolerance.  On an MI355X the largest observed
fractions were 0.0013 (rotation, translation) and 0.0009 (score): the device sits about as far from the restatement as the restatement
from its own extended-precision run.

Shapes are the smallest at which a piece can go wrong: M around the 256-thread workgroup of the segmented sums and the selection (255,
256, 257) and several workgroups per pose (1000); S = 65 crosses the slab of 64 poses (rigid_search_plan.h: kMaxSlabPoses), so pose 64
runs in a second slab, alone; N = 1 and 7 are answered inside the grid kernel, N = 5000 is past its brute-force limit (4096), so the
flagged queries of bad starts go to the masked tile scan.

Recovery (femur[::4] against all of femur_target under a random rigid motion, seeds 0..7, 64 spiral starts, K = 10): the bound is 3
degrees from R_true R_base after GlobalRigidAlignment's refinement; the restatement itself, re-measured, reaches 1.02 degrees (plain)
and 0.82 degrees (72 clutter points, overlap 0.85) at most (tests/test_rigid_search_host.py).  On an MI355X the device search picked
the restatement's start for every seed, scores agreed to 4e-14 relative, and after the RigidICP refinement (which stops at its own
convergence test after 2 to 31 iterations) the largest angles were 1.87 degrees (plain, seed 1) and 2.39 degrees (clutter, seed 2)."""
import numpy as np
import pytest

from tests import rigid_search_restatement as rs

pytestmark = pytest.mark.gpu

MARGIN = 1000.0
EPS = float(np.finfo(np.float64).eps)
FIELDS = ("rotations", "translations", "scores", "kept", "failed")


def run(ctx, X, Y, rotations, K, rho=1.0):
    """the call, twice: the same bits"""
    a = ctx.rigid_search(X, Y, rotations, K, rho)
    b = ctx.rigid_search(X, Y, rotations, K, rho)
    assert a.best == b.best
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    return a


def cloud_case(M, N, S, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 30.0, (M, 3)) + [200.0, -50.0, 10.0]
    Y = rng.normal(0, 30.0, (N, 3)) + [-40.0, 300.0, 80.0]
    R0 = np.stack([rs.random_rotation(rng) for _ in range(S)])
    return X, Y, R0


def yardstick(X, Y, R0, K, rho):
    """(the float64 restatement, tolerances of rotation, translation, score)"""
    a = rs.search(X, Y, R0, K, rho)
    b = rs.search(X, Y, R0, K, rho, np.longdouble)
    scale = float(max(np.abs(X).max(), np.abs(Y).max()))
    tol = (MARGIN * max(float(np.abs(a["rotations"] - b["rotations"]).max()), EPS),
           MARGIN * max(float(np.abs(a["translations"] - b["translations"]).max()), EPS * scale),
           MARGIN * max(float(np.abs(a["scores"] - b["scores"]).max()), EPS * scale))
    return a, tol


def ratio(name, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)), name
    worst = float(np.abs(got - want).max() / tol)
    print(f"{name}: observed / tolerance = {worst:.3g}")
    assert worst <= 1.0, (name, worst)


def proper(name, R):
    R = np.asarray(R).reshape(-1, 3, 3)
    assert np.all(np.isfinite(R)), name
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 1e-12, name
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12, name


# ------------------------------------------------------------------------------------------------ one iteration from given poses
WELL_POSED = [(255, 1, 7), (255, 2, 5000), (256, 2, 5000), (256, 65, 7), (257, 65, 5000), (1000, 1, 7), (1000, 65, 5000)]
ILL_POSED = [(1, 1, 1), (2, 2, 1), (3, 65, 1), (1, 2, 7), (2, 65, 7), (3, 2, 5000), (257, 2, 1), (1000, 65, 1)]


@pytest.mark.parametrize("M,S,N", WELL_POSED)
def test_one_iteration_against_the_restatement(ctx, M, S, N):
    X, Y, R0 = cloud_case(M, N, S, seed=M + S + N)
    got = run(ctx, X, Y, R0, 1)
    want, (tr, tt, ts) = yardstick(X, Y, R0, 1, 1.0)
    name = f"M {M} S {S} N {N}"
    assert got.best == want["best"] and np.array_equal(got.kept, want["kept"]) and not got.failed.any()
    ratio(f"rotation: {name}", got.rotations, want["rotations"], tr)
    ratio(f"translation: {name}", got.translations, want["translations"], tt)
    ratio(f"score: {name}", got.scores, want["scores"], ts)
    proper(name, got.rotations)
    assert np.array_equal(got.R, got.rotations[got.best]) and np.array_equal(got.t, got.translations[got.best]) and got.score == got.scores[got.best]


@pytest.mark.parametrize("M,S,N", ILL_POSED)
def test_one_iteration_with_a_rank_deficient_cross_covariance(ctx, M, S, N):
    """M <= 3 or N = 1: H has rank < 3 (zero for N = 1 or M = 1) and the rotation is not determined.  Required: a finite pose, a
    proper rotation, the centroids of the pairs mapped onto each other, and kept count and score as the restatement's."""
    X, Y, R0 = cloud_case(M, N, S, seed=M + S + N)
    got = run(ctx, X, Y, R0, 1)
    name = f"M {M} S {S} N {N}"
    proper(name, got.rotations)
    assert np.all(np.isfinite(got.translations)) and np.all(np.isfinite(got.scores)) and not got.failed.any()
    assert np.array_equal(got.kept, np.full(S, M))
    scale = float(max(np.abs(X).max(), np.abs(Y).max()))
    tree = __import__("scipy.spatial", fromlist=["cKDTree"]).cKDTree(Y)
    for s, (R, t) in enumerate(rs.start_poses(X, Y, R0)):
        j, _ = rs.nearest(X @ R.T + t, Y, tree)
        mu_y = Y[j].mean(0)
        moved = (X @ got.rotations[s].T + got.translations[s]).mean(0)                       # R mu_p + t = mu_y
        assert np.abs(moved - mu_y).max() <= MARGIN * EPS * scale, (name, s)
        _, d2 = rs.nearest(X @ got.rotations[s].T + got.translations[s], Y, tree)            # the score of the pose that came back
        assert abs(got.scores[s] - np.sqrt(d2.mean())) <= MARGIN * EPS * scale, (name, s)


# ------------------------------------------------------------------------------------------------ trimming
@pytest.mark.parametrize("M", [256, 257, 1000])
@pytest.mark.parametrize("which", ["one", "half", "all but one", "all"])
def test_ties_at_the_threshold_stay(ctx, M, which):
    """every moving point three times gives bit-equal distances: wherever in a triple the rank keep - 1 falls, all three are kept"""
    rho = {"one": 1.0 / M, "half": 0.5, "all but one": (M - 1.0) / M, "all": 1.0}[which]
    X, Y, R0 = cloud_case(M, 300, 3, seed=M)
    X = np.ascontiguousarray(X[np.arange(M) // 3 * 3])
    got = run(ctx, X, Y, R0, 1, rho)
    want, (tr, tt, ts) = yardstick(X, Y, R0, 1, rho)
    keep = rs.keep_count(M, rho)
    print(f"M {M} rho {rho:.6f}: keep {keep}, kept {got.kept.tolist()}")
    assert np.array_equal(got.kept, want["kept"]) and (got.kept >= keep).all()
    if which != "all":
        assert (got.kept > keep).any()                                                     # a tie at the threshold did occur
    ratio(f"score: M {M} {which}", got.scores, want["scores"], ts)
    if which != "one":                                                                       # (coincident points determine no rotation)
        ratio(f"rotation: M {M} {which}", got.rotations, want["rotations"], tr)
        ratio(f"translation: M {M} {which}", got.translations, want["translations"], tt)
    proper(f"M {M} {which}", got.rotations)


@pytest.mark.parametrize("M", [257, 1000])
def test_a_far_point_is_trimmed_away(ctx, M):
    """One moving point 300 units off, overlap (M - 1) / M, against the call without it at overlap 1.  The two calls start a little apart
    (the far point moves mean X by 300 / M), so both run to ICP's fixed point, where the pose is a function of the kept pairs alone."""
    rng = np.random.default_rng(M)
    Xn = rng.normal(0, 30.0, (M - 1, 3)) + [200.0, -50.0, 10.0]
    R_true = rs.random_rotation(rng)
    Y = Xn @ R_true.T + [-300.0, 40.0, 90.0]
    X = np.concatenate([Xn[:M // 2], Xn.mean(0)[None] + [300.0, 0.0, 0.0], Xn[M // 2:]])
    K, rho = 25, (M - 1.0) / M
    trimmed, plain = run(ctx, X, Y, R_true[None], K, rho), run(ctx, Xn, Y, R_true[None], K)
    want, (tr, tt, ts) = yardstick(X, Y, R_true[None], K, rho)
    assert trimmed.kept.tolist() == [M - 1] == want["kept"].tolist() and plain.kept.tolist() == [M - 1]
    ratio(f"rotation: far point, M {M}", trimmed.R, plain.R, tr)
    ratio(f"translation: far point, M {M}", trimmed.t, plain.t, tt)
    ratio(f"rotation against the restatement: far point, M {M}", trimmed.R, want["R"], tr)
    ratio(f"translation against the restatement: far point, M {M}", trimmed.t, want["t"], tt)
    assert np.abs(trimmed.R - R_true).max() < 1e-9 and trimmed.score < 1e-6                   # the rigid copy is found


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("rho", [1.0, 0.5])
def test_a_pose_does_not_depend_on_its_company(ctx, rho):
    """The same start rotation alone, as pose 0 of 65 and as pose 64 of 65: pose 0 is the first lane of a full slab of 64 poses (64 000
    queries: the 8-lane grid kernel, 250 workgroups of the pose kernel per pose row), pose 64 the only pose of the second slab, and alone
    it is a slab of one (1000 queries: the 16-lane grid kernel, the chunked tile scan).  The bits must not change."""
    X, Y, R0 = cloud_case(1000, 5000, 65, seed=11)
    R0[64] = R0[0]
    full, alone, other = run(ctx, X, Y, R0, 2, rho), run(ctx, X, Y, R0[:1], 2, rho), run(ctx, X, Y, R0[63:64], 2, rho)
    for f in FIELDS:
        assert np.array_equal(getattr(full, f)[0], getattr(alone, f)[0]), f
        assert np.array_equal(getattr(full, f)[64], getattr(alone, f)[0]), f
        assert np.array_equal(getattr(full, f)[63], getattr(other, f)[0]), f               # the last lane of the full slab
    assert full.best == int(np.argmin(full.scores)) and (full.best != 64)                    # ties go to the lowest pose


# ------------------------------------------------------------------------------------------------ refusals and failures
def test_refusals(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    X, Y, R0 = cloud_case(10, 12, 3)

    def code(*a, **k):
        with pytest.raises(ga.GingrNativeError) as e:
            ctx.rigid_search(*a, **k)
        return e.value.code

    assert code(X[:0], Y, R0) == nat.ERR_BAD_ARGUMENT and code(X, Y[:0], R0) == nat.ERR_BAD_ARGUMENT
    assert code(X, Y, R0[:0]) == nat.ERR_BAD_ARGUMENT and code(X, Y, R0, iterations=-1) == nat.ERR_BAD_ARGUMENT
    for rho in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert code(X, Y, R0, overlap=rho) == nat.ERR_BAD_ARGUMENT, rho
    for bad in (float("nan"), float("inf"), -float("inf")):
        Xb, Yb, Rb = X.copy(), Y.copy(), R0.copy()
        Xb[3, 1] = Yb[11, 2] = Rb[2, 1, 1] = bad
        assert code(Xb, Y, R0) == nat.ERR_NONFINITE and code(X, Yb, R0) == nat.ERR_NONFINITE and code(X, Y, Rb) == nat.ERR_NONFINITE
    with pytest.raises(ValueError):
        ctx.rotation_samples(0)
    ok = run(ctx, X, Y, R0, 0)                                                               # K = 0: the start poses, scored
    want = rs.search(X, Y, R0, 0)
    assert np.array_equal(ok.rotations, R0) and ok.best == want["best"] and np.allclose(ok.scores, want["scores"], rtol=1e-12, atol=0)
    assert run(ctx, X, Y, R0, 3, 1e-300).kept.tolist() == [1, 1, 1]                          # the smallest overlap keeps one pair


def test_equal_poses_tie_to_the_first(ctx):
    X, Y, _ = cloud_case(300, 400, 1)
    R0 = np.repeat(rs.rotation_samples(3)[1:2], 70, axis=0)                                   # 70 equal starts, two slabs
    res = run(ctx, X, Y, R0, 3, 0.7)
    assert res.best == 0 and np.all(res.scores == res.scores[0]) and np.all(res.rotations == res.rotations[0])
    assert np.array_equal(ctx.rotation_samples(64), ctx.rotation_samples(64))
    assert np.abs(ctx.rotation_samples(64) - rs.rotation_samples(64)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ recovery
@pytest.fixture(scope="module")
def bases():
    _, tgt = rs.femur_pair()
    return {clutter: rs.icp_from(rs.recovery_case(0, clutter)[0], tgt, np.eye(3), np.zeros(3), 50, rho)[0]
            for clutter, rho in ((False, 1.0), (True, 0.85))}


@pytest.mark.parametrize("clutter,rho", [(False, 1.0), (True, 0.85)])
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_recovery_from_an_arbitrary_pose(ctx, bases, seed, clutter, rho):
    from gingr_amd import classic
    tpl, Y, R_true, _ = rs.recovery_case(seed, clutter)
    got = run(ctx, tpl, Y, 64, 10, rho)
    want = rs.search(tpl, Y, rs.rotation_samples(64), 10, rho)
    order = np.sort(got.scores)
    print(f"seed {seed} clutter {clutter}: best {got.best} (restatement {want['best']}) score {got.score:.6f}, "
          f"scores relative {np.abs(got.scores / want['scores'] - 1).max():.3g}, runner-up {order[1] / order[0] - 1:.3%} above")
    assert got.best == want["best"] and not got.failed.any()
    assert np.abs(got.scores / want["scores"] - 1.0).max() <= 1e-6
    ga = classic.GlobalRigidAlignment(ctx, tpl, starts=64, iterations=10, overlap=rho)
    aligned = ga.register(Y)
    R, t = ga.transform
    angle = rs.angle_deg(R, R_true @ bases[clutter])
    print(f"seed {seed} clutter {clutter}: after refinement ({ga.refineIterationsDone} iterations) {angle:.3f} degrees from R_true R_base")
    assert angle <= 3.0
    assert ga.searchResult.best == got.best and np.abs(aligned - (tpl @ R.T + t)).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ the Python layer
def test_result_record_and_alignment(ctx):
    from gingr_amd import classic
    femur, tgt = rs.femur_pair()
    tpl, Y = np.ascontiguousarray(femur[::4]), tgt @ rs.rotation_samples(5)[3].T + [30.0, -80.0, 120.0]
    res = run(ctx, tpl, Y, 7, 2, 0.9)
    assert isinstance(res.best, int) and 0 <= res.best < 7 and isinstance(res.score, float)
    assert res.R.shape == (3, 3) and res.t.shape == (3,) and res.rotations.shape == (7, 3, 3) and res.translations.shape == (7, 3)
    assert res.scores.shape == res.kept.shape == res.failed.shape == (7,) and res.kept.dtype == np.int64 and res.failed.dtype == bool
    assert (res.kept >= rs.keep_count(406, 0.9)).all()
    ga = classic.GlobalRigidAlignment(ctx, tpl, starts=16, iterations=4, maxPoints=100, refineIterations=5)
    aligned = ga.register(Y)
    R, t = ga.transform
    assert aligned.shape == tpl.shape and np.abs(aligned - (tpl @ R.T + t)).max() <= 1e-9      # transform reproduces register's points
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    sub = run(ctx, tpl[::5], Y, 16, 4)                                                        # 406 > 100 points: every 5th
    assert ga.searchPoints().shape == (82, 3) and np.array_equal(ga.searchResult.rotations, sub.rotations)
    none = classic.GlobalRigidAlignment(ctx, tpl, starts=16, iterations=4, maxPoints=100, refineIterations=0)
    assert np.array_equal(none.register(Y), tpl @ sub.R.T + sub.t) and np.array_equal(none.transform[0], sub.R)
