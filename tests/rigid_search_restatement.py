"""The definition of the global rigid pre-alignment (gingr_rigid_search, include/gingr_hip.h) restated in numpy: the yardstick of
tests/test_rigid_search_host.py and tests/test_gpu_rigid_search.py.  Nothing here is shared with the device code.

Inputs: moving points X (M, 3), target points Y (N, 3), S start rotations, K >= 0 iterations, overlap rho in (0, 1].
Start pose of s: T_s(x) = R0_s (x - mean X) + mean Y, held as (R_s, t_s), p = R_s x + t_s.  One iteration, per pose:
  1. p_i = R_s x_i + t_s, always from the original X and the composed pose;
  2. j_i = the exact nearest target, the lowest index on ties, d2_i = dx*dx + dy*dy + dz*dz;
  3. keep = ceil(rho M) (of the float64 product, in [1, M]); tau = the order statistic of rank keep - 1 of d2; kept = {i: d2_i <= tau},
     ties included; rho = 1 keeps everything;
  4. from the kept pairs, centred on mean Y: mu_p, mu_y, H = sum (y - mu_y)(p - mu_p)^T / n; dR = the proper rotation closest to H
     (U diag(1, 1, det(U V^T)) V^T); dt = mu_y - dR mu_p;
  5. R_s <- dR R_s, t_s <- dR t_s + dt.
After K iterations one more search and selection: score_s = sqrt(mean of the kept d2).  A pose whose transform is not finite gets the
score +inf and failed = True.  The result is the pose of the smallest score, the lowest s on ties.

dtype = np.longdouble runs the same definition in extended precision (the 3 x 3 rotation by a Newton iteration for the polar factor,
numpy's SVD being float64 only); the difference between the two runs is the spread the device tolerances are set from.
brute = True replaces the k-d tree by the argmin over all pairs."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PHI = np.sqrt(np.longdouble(2.0))
PSI = np.longdouble("1.533751168755204288118041")


# ------------------------------------------------------------------------------------------------ rotations
def quaternion_to_rotation(q):
    """row-major rotation of the unit quaternion (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.asarray(q).dtype)


def spiral_quaternions(n, dtype=np.float64):
    """super-Fibonacci spiral (Alexa 2022), (n, 4) as (x, y, z, w)"""
    s = np.arange(n, dtype=dtype) + dtype(0.5)
    two_pi = 2 * np.pi if dtype is np.float64 else 2 * np.longdouble("3.14159265358979323846264338327950288")
    phi, psi = dtype(PHI), dtype(PSI)
    r, big = np.sqrt(s / n), np.sqrt(1 - s / n)
    a, b = two_pi * s / phi, two_pi * s / psi
    return np.stack([r * np.sin(a), r * np.cos(a), big * np.sin(b), big * np.cos(b)], axis=1)


def rotation_samples(n, dtype=np.float64):
    return np.stack([quaternion_to_rotation(q) for q in spiral_quaternions(n, dtype)])


def random_rotation(rng):
    """the rotation of the normalised quaternion rng.normal(size=4), (x, y, z, w)"""
    q = rng.normal(size=4)
    return quaternion_to_rotation(q / np.linalg.norm(q))


def angle_deg(A, B):
    c = (np.trace(np.asarray(A, dtype=np.float64).T @ np.asarray(B, dtype=np.float64)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ------------------------------------------------------------------------------------------------ the pieces of an iteration
def keep_count(M, rho):
    return int(min(M, max(1, np.ceil(np.float64(rho) * np.float64(M)))))


def _d2(p, y):
    d = p - y
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_brute(P, Y):
    """(j, d2): the argmin over all pairs, the lowest index on ties (np.argmin returns the first)"""
    j = np.empty(P.shape[0], dtype=np.int64)
    d2 = np.empty(P.shape[0], dtype=P.dtype)
    for a in range(0, P.shape[0], 512):
        D = _d2(P[a:a + 512, None, :], Y[None, :, :])
        j[a:a + 512] = D.argmin(1)
        d2[a:a + 512] = D[np.arange(D.shape[0]), j[a:a + 512]]
    return j, d2


def nearest(P, Y, tree=None):
    """the same by scipy's k-d tree: its two nearest candidates, the distances recomputed as above; rows whose two candidates tie go to
    the argmin over all pairs (the tie rule)"""
    if tree is None or Y.shape[0] < 2:
        return nearest_brute(P, Y)
    _, cand = tree.query(P, k=2)
    d = np.stack([_d2(P, Y[cand[:, 0]]), _d2(P, Y[cand[:, 1]])], axis=1)
    pick = np.where((d[:, 1] < d[:, 0]) | ((d[:, 1] == d[:, 0]) & (cand[:, 1] < cand[:, 0])), 1, 0)
    rows = np.arange(P.shape[0])
    j, d2 = cand[rows, pick].astype(np.int64), d[rows, pick]
    tie = np.nonzero(d[:, 0] == d[:, 1])[0]
    if tie.size:
        j[tie], d2[tie] = nearest_brute(P[tie], Y)
    return j, d2


def kept_mask(d2, keep):
    if keep >= d2.shape[0]:
        return np.ones(d2.shape[0], dtype=bool)
    tau = np.partition(d2, keep - 1)[keep - 1]
    return d2 <= tau


def closest_rotation(H):
    """the proper rotation closest to H: U diag(1, 1, det(U V^T)) V^T.  longdouble: the float64 answer polished by Newton's iteration
    for the polar factor where H has a determinant safely above zero (there the two are the same matrix)"""
    H64 = np.asarray(H, dtype=np.float64)
    U, _, Vt = np.linalg.svd(H64)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    R = U @ D @ Vt
    if H.dtype == np.float64:
        return R
    nf = np.sqrt((H64 * H64).sum())
    if not (np.linalg.det(H64) > 1e-10 * nf ** 3):
        return R.astype(H.dtype)
    X = H / H.dtype.type(nf)
    for _ in range(60):
        C = np.array([[X[1, 1] * X[2, 2] - X[1, 2] * X[2, 1], X[1, 2] * X[2, 0] - X[1, 0] * X[2, 2], X[1, 0] * X[2, 1] - X[1, 1] * X[2, 0]],
                      [X[0, 2] * X[2, 1] - X[0, 1] * X[2, 2], X[0, 0] * X[2, 2] - X[0, 2] * X[2, 0], X[0, 1] * X[2, 0] - X[0, 0] * X[2, 1]],
                      [X[0, 1] * X[1, 2] - X[0, 2] * X[1, 1], X[0, 2] * X[1, 0] - X[0, 0] * X[1, 2], X[0, 0] * X[1, 1] - X[0, 1] * X[1, 0]]],
                     dtype=H.dtype)                                                    # cofactors: X^-T = C / det
        det = (X[0] * C[0]).sum()
        g = np.sqrt(np.sqrt((C * C).sum() / (X * X).sum()) / det)
        Xn = (g * X + C / (det * g)) / 2
        done = np.abs(Xn - X).max() < 1e-19
        X = Xn
        if done:
            break
    return X


def step(p, y, c):
    """(dR, dt) of the pairs (p_i, y_i), sums centred on c"""
    pt, yt = p - c, y - c
    n = p.dtype.type(p.shape[0])
    mup, muy = pt.sum(0) / n, yt.sum(0) / n
    H = (yt.T @ pt) / n - np.outer(muy, mup)
    dR = closest_rotation(H)
    return dR, (muy + c) - dR @ (mup + c)


# ------------------------------------------------------------------------------------------------ the search
def start_poses(X, Y, rotations):
    mx, c = X.mean(0), Y.mean(0)
    return [(R.copy(), c - R @ mx) for R in rotations]


def iterate_pose(X, Y, R, t, K, rho, tree=None):
    """K iterations and the scoring pass of one pose: (R, t, score, kept, failed)"""
    c = Y.mean(0)
    keep = keep_count(X.shape[0], rho)
    failed = False
    for _ in range(K):
        p = X @ R.T + t
        j, d2 = nearest(p, Y, tree)
        m = kept_mask(d2, keep)
        dR, dt = step(p[m], Y[j[m]], c)
        Rn, tn = dR @ R, dR @ t + dt
        if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
            failed = True
            break
        R, t = Rn, tn
    if failed:
        return R, t, np.inf, 0, True
    p = X @ R.T + t
    j, d2 = nearest(p, Y, tree)
    m = kept_mask(d2, keep)
    return R, t, float(np.sqrt(d2[m].sum() / m.sum())), int(m.sum()), False


def search(X, Y, rotations, K, rho=1.0, dtype=np.float64, brute=False):
    """dict(best, R, t, score, rotations, translations, scores, kept, failed); every pose failed: best = -1"""
    X, Y = np.asarray(X, dtype=dtype).reshape(-1, 3), np.asarray(Y, dtype=dtype).reshape(-1, 3)
    rotations = np.asarray(rotations, dtype=dtype).reshape(-1, 3, 3)
    tree = None
    if not brute:                                      # (the tree proposes two candidates in float64; their distances are taken in dtype)
        from scipy.spatial import cKDTree
        tree = cKDTree(Y.astype(np.float64))
    out = [iterate_pose(X, Y, R, t, K, rho, tree) for R, t in start_poses(X, Y, rotations)]
    scores = np.array([o[2] for o in out], dtype=np.float64)
    failed = np.array([o[4] for o in out])
    best = -1 if failed.all() else int(np.argmin(np.where(failed, np.inf, scores)))
    res = dict(best=best, rotations=np.stack([o[0] for o in out]), translations=np.stack([o[1] for o in out]), scores=scores,
               kept=np.array([o[3] for o in out], dtype=np.int64), failed=failed)
    if best >= 0:
        res.update(R=res["rotations"][best], t=res["translations"][best], score=float(scores[best]))
    return res


def icp_from(X, Y, R, t, iterations=50, rho=1.0):
    """plain ICP of the definition from a given pose: what the restatement reaches from there"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    from scipy.spatial import cKDTree
    return iterate_pose(X, Y, np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), iterations, rho, cKDTree(Y))


# ------------------------------------------------------------------------------------------------ the recovery inputs
SEEDS = tuple(range(8))


def femur_pair():
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    return np.ascontiguousarray(d["femur"], dtype=np.float64), np.ascontiguousarray(d["femur_target"], dtype=np.float64)


def recovery_case(seed, clutter=False):
    """(template, target, R_true, t_true): femur[::4] (plus 72 clutter points), all of femur_target turned by the seed's rotation and
    shifted by normal(size=3) * 100"""
    femur, tgt = femur_pair()
    tpl = np.ascontiguousarray(femur[::4])
    if clutter:
        lo, hi = tpl.min(0) - 40.0, tpl.max(0) + 40.0
        tpl = np.concatenate([tpl, np.random.default_rng(7).uniform(lo, hi, (72, 3))])
    rng = np.random.default_rng(seed)
    R = random_rotation(rng)
    shift = rng.normal(size=3) * 100.0
    return tpl, tgt @ R.T + shift, R, shift
