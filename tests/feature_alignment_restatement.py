"""The definition of the feature-based global alignment (gingr_cloud_fpfh, gingr_feature_match, gingr_rigid_poses_from_triples,
gingr_rigid_search_poses of include/gingr_hip.h; classic.FeatureRigidAlignment) restated in numpy: the yardstick of
tests/test_feature_alignment_host.py and tests/test_gpu_feature_alignment.py.  Nothing here is shared with the device code.  The
definitions are this package's own (Fast Point Feature Histograms after Rusu 2009, with the neighbourhood, the bins and the weights
fixed as below), not a toolkit's.

Neighbours of i: the entries of i's k-nearest list (sorted by (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in float64), in list order,
with 0 < d2 <= radius^2.
Pair features of (i, j), u = n_i, d = x_j - x_i, dn = d / |d|: phi = u . dn; v = dn x u, the pair is SKIPPED when |v|^2 <= 2^-40 or a
normal of the two is zero, else v is normalised; w = u x v; alpha = v . n_j; theta = atan2(w . n_j, u . n_j).
Bins, eleven per feature: min(10, max(0, floor((f + 1) / 2 * 11))) for alpha and phi, the same of (f + pi) / (2 pi) for theta.
counts_i [33]: alpha bins, then phi, then theta; valid_i: the counted pairs.  SPFH_i = 100 counts_i / valid_i (0 when valid_i = 0).
FPFH_i = SPFH_i + (sum_j SPFH_j / d_j) / (sum_j 1 / d_j) over ALL neighbours in list order, d_j = sqrt(d2_j) (the second term is 0
without neighbours); then every third is rescaled to sum 100 (a third that sums to 0 is left alone).
Match: per row of a the row of b with the smallest sum_c (a_c - b_c)^2, terms added in ascending c, the lowest index on ties.
Pose of a triple of pairs: the step of tests/rigid_search_restatement.py (Kabsch with the reflection fix) of the three pairs, sums
centred on the mean of the triple's target points; degenerate (NaN pose) when an index repeats or the squared area of either triangle
is <= 2^-40 (longest edge)^4.
Search from poses: the iteration of rigid_search_restatement from given (R, t); inliers = the moving points with d2 <= distance^2 in
the scoring pass; select 0: the smallest score; select 1: the most inliers, then the smaller score, then the lowest index.

dtype = np.longdouble runs the pair features, the histogram weights and the triple step in extended precision.  DELTA below is the
largest difference the two routes show in any pair feature of the femur fixture (k = 64, radius 25, normals of 12 neighbours turned
towards the centroid), measured by tests/test_feature_alignment_host.py: 8.4e-15 (theta; alpha 4.4e-16, phi 2.6e-16).  A pair is EDGE-NEAR
when a feature lies within 16 DELTA of a bin edge, in the feature's own units (for theta also of +-pi, where the angle wraps)."""
import os

import numpy as np

from tests import rigid_search_restatement as rs

HERE = os.path.dirname(os.path.abspath(__file__))
BINS = 11
SKIP = 2.0 ** -40
DELTA = 2.0 ** -46                  # 1.42e-14: the measured 8.4e-15 rounded up to a power of two
PI_LD = np.longdouble("3.14159265358979323846264338327950288")


# ------------------------------------------------------------------------------------------------ lists and normals
def knn(x, k):
    """(idx (N, k) int64, d2 (N, k)) sorted by (d2, index).  Up to 4096 points from all pairs (exact ties included); beyond, from the
    k-d tree's k + 8 candidates with the distances recomputed (a tie across the candidate boundary is not seen: benchmarks only)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N = x.shape[0]
    if N <= 4096:
        d = x[:, None, :] - x[None, :, :]
        D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx = np.argsort(D, axis=1, kind="stable")[:, :k]
        return idx.astype(np.int64), np.take_along_axis(D, idx, axis=1)
    from scipy.spatial import cKDTree
    kk = min(N, k + 8)
    _, cand = cKDTree(x).query(x, k=kk)
    d = x[cand] - x[:, None, :]
    D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.lexsort((cand, D), axis=1)[:, :k]
    return np.take_along_axis(cand, order, axis=1).astype(np.int64), np.take_along_axis(D, order, axis=1)


def normals(x, k, viewpoint=None):
    """unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance (float64, numpy's eigh), zero where
    lam1 - lam0 <= 2^-26 lam2, turned towards the viewpoint"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    idx, _ = knn(x, k)
    q = x[idx] - x[:, None, :]
    q = q - q.mean(1, keepdims=True)
    lam, V = np.linalg.eigh(np.einsum("nki,nkj->nij", q, q) / k)
    n = V[:, :, 0].copy()
    n[lam[:, 1] - lam[:, 0] <= 2.0 ** -26 * lam[:, 2]] = 0.0
    if viewpoint is not None:
        n[((np.asarray(viewpoint)[None] - x) * n).sum(1) < 0] *= -1.0
    return n


def unit_normals(n):
    """the rule of gingr_fitter_set_target_normals: unit to 2^-48 taken as it is, else scaled by the largest component and normalised;
    zero stays zero"""
    n = np.ascontiguousarray(n, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(n)
    for j, (x, y, z) in enumerate(n):
        big = max(abs(x), abs(y), abs(z))
        if big > 0.0:
            n2 = (x * x + y * y) + z * z
            if abs(n2 - 1.0) <= 2.0 ** -48:
                out[j] = x, y, z
            else:
                sx, sy, sz = x / big, y / big, z / big
                ln = np.sqrt((sx * sx + sy * sy) + sz * sz)
                out[j] = sx / ln, sy / ln, sz / ln
    return out


# ------------------------------------------------------------------------------------------------ descriptor
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(x, n, idx, d2, radius, dtype=np.float64):
    """(neighbour (N, k) bool, counted (N, k) bool, alpha, phi, theta (N, k) in dtype): the features of the pairs that are not counted
    are meaningless"""
    x64, n64 = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(n, dtype=np.float64)
    xd, nd = x64.astype(dtype), n64.astype(dtype)
    nb = (d2 > 0.0) & (d2 <= np.float64(radius) * np.float64(radius))
    has = (n64 != 0.0).any(1)
    u = np.broadcast_to(nd[:, None, :], idx.shape + (3,))
    nj = nd[idx]
    d = xd[idx] - xd[:, None, :]
    ln = np.sqrt(_dot(d, d))
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = d / ln[..., None]
        phi = _dot(u, dn)
        v = _cross(dn, u)
        v2 = _dot(v, v)
        ok = nb & has[:, None] & has[idx] & (v2 > dtype(SKIP))
        v = v / np.sqrt(v2)[..., None]
        w = _cross(u, v)
        alpha = _dot(v, nj)
        theta = np.arctan2(_dot(w, nj), _dot(u, nj))
    return nb, ok, alpha, phi, theta


def _unit_interval(f, which, dtype):
    if which == 2:
        pi = np.pi if dtype is np.float64 else PI_LD
        return (f + pi) / (2 * pi)
    return (f + 1) / 2


def bins_of(alpha, phi, theta, dtype=np.float64):
    """(..., 3) int: the bin of each feature"""
    out = []
    with np.errstate(invalid="ignore"):
        for which, f in enumerate((alpha, phi, theta)):
            b = np.floor(_unit_interval(f, which, dtype) * BINS)
            out.append(np.clip(np.where(np.isfinite(b), b, 0), 0, BINS - 1).astype(np.int64))
    return np.stack(out, axis=-1)


def edge_near(alpha, phi, theta, width=16 * DELTA):
    """a feature within `width` of an interior bin edge in its own units, or theta within `width` of +-pi"""
    near = np.zeros(np.shape(alpha), dtype=bool)
    with np.errstate(invalid="ignore"):
        for which, f in enumerate((alpha, phi, theta)):
            f = np.asarray(f, dtype=np.float64)
            lo, span = (-np.pi, 2 * np.pi) if which == 2 else (-1.0, 2.0)
            for b in range(1, BINS):
                near |= np.abs(f - (lo + span * b / BINS)) <= width
            if which == 2:
                near |= np.pi - np.abs(f) <= width
    return near


def histograms(ok, bins):
    """(counts (N, 33) int32, valid (N,) int32)"""
    N = ok.shape[0]
    counts = np.zeros((N, 3 * BINS), dtype=np.int32)
    rows = np.nonzero(ok)
    for which in range(3):
        np.add.at(counts, (rows[0], which * BINS + bins[..., which][rows]), 1)
    return counts, ok.sum(1).astype(np.int32)


def fpfh_from_counts(counts, valid, idx, d2, nb, dtype=np.float64):
    """(N, 33) in dtype: the weighted sums in list order, then the three thirds rescaled"""
    c, val = np.asarray(counts).astype(dtype), np.asarray(valid).astype(dtype)
    spfh = np.where(val[:, None] > 0, dtype(100) * c / np.where(val > 0, val, dtype(1))[:, None], dtype(0))
    N, k = idx.shape
    num, den = np.zeros((N, 3 * BINS), dtype=dtype), np.zeros(N, dtype=dtype)
    dj = np.sqrt(np.asarray(d2).astype(dtype))
    for s in range(k):
        m = nb[:, s]
        inv = np.where(m, dtype(1) / np.where(m, dj[:, s], dtype(1)), dtype(0))
        num = num + np.where(m[:, None], spfh[idx[:, s]] / np.where(m, dj[:, s], dtype(1))[:, None], dtype(0))
        den = den + inv
    f = spfh + np.where(den[:, None] > 0, num / np.where(den > 0, den, dtype(1))[:, None], dtype(0))
    for t in range(3):
        third = f[:, t * BINS:(t + 1) * BINS]
        s = np.zeros(N, dtype=dtype)
        for b in range(BINS):
            s = s + third[:, b]
        f[:, t * BINS:(t + 1) * BINS] = np.where(s[:, None] != 0, third * (dtype(100) / np.where(s != 0, s, dtype(1)))[:, None], third)
    return f


def fpfh(x, n, k, radius, dtype=np.float64, lists=None):
    """dict(fpfh, counts, valid, idx, d2, neighbour, counted, alpha, phi, theta); the normals by unit_normals"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    n = unit_normals(n)
    idx, d2 = knn(x, k) if lists is None else lists
    nb, ok, alpha, phi, theta = pair_features(x, n, idx, d2, radius, dtype)
    counts, valid = histograms(ok, bins_of(alpha, phi, theta, dtype))
    return dict(fpfh=fpfh_from_counts(counts, valid, idx, d2, nb, dtype), counts=counts, valid=valid, idx=idx, d2=d2, neighbour=nb,
                counted=ok, alpha=alpha, phi=phi, theta=theta)


# ------------------------------------------------------------------------------------------------ match
def feature_match(a, b):
    """(idx (M,) int64, d2 (M,)): float64, terms in ascending column order, np.argmin takes the first of equal sums"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    M, D = a.shape
    idx, d2 = np.empty(M, dtype=np.int64), np.empty(M)
    for r0 in range(0, M, 128):
        blk = a[r0:r0 + 128]
        acc = np.zeros((blk.shape[0], b.shape[0]))
        for c in range(D):
            t = blk[:, c, None] - b[None, :, c]
            acc = acc + t * t
        j = acc.argmin(1)
        idx[r0:r0 + 128], d2[r0:r0 + 128] = j, acc[np.arange(blk.shape[0]), j]
    return idx, d2


# ------------------------------------------------------------------------------------------------ poses of triples
def _area2_and_edge4(p):
    e0, e1, e2 = p[1] - p[0], p[2] - p[0], p[2] - p[1]
    c = _cross(e0, e1)
    longest = max(_dot(e0, e0), _dot(e1, e1), _dot(e2, e2))
    return _dot(c, c) / 4, longest * longest


def triple_degenerate(X, Y, tm, tt):
    if len(set(int(i) for i in tm)) < 3 or len(set(int(i) for i in tt)) < 3:
        return True
    for P, tri in ((X, tm), (Y, tt)):
        with np.errstate(over="ignore", invalid="ignore"):
            a2, e4 = _area2_and_edge4(P[np.asarray(tri)])
            if not a2 > SKIP * e4:
                return True
    return False


def poses_from_triples(X, Y, tri_moving, tri_target, dtype=np.float64):
    """(poses (H, 12) in dtype: R row-major then t, NaN where degenerate; degenerate (H,) bool)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    tri_moving, tri_target = np.asarray(tri_moving).reshape(-1, 3), np.asarray(tri_target).reshape(-1, 3)
    H = tri_moving.shape[0]
    poses, deg = np.full((H, 12), np.nan, dtype=dtype), np.zeros(H, dtype=bool)
    for h in range(H):
        if triple_degenerate(X, Y, tri_moving[h], tri_target[h]):
            deg[h] = True
            continue
        p, y = X[tri_moving[h]].astype(dtype), Y[tri_target[h]].astype(dtype)
        c = ((y[0] + y[1]) + y[2]) / dtype(3)
        dR, dt = rs.step(p, y, c)
        poses[h, :9], poses[h, 9:] = np.asarray(dR, dtype=dtype).reshape(9), dt
    return poses, deg


# ------------------------------------------------------------------------------------------------ search from poses
def start_poses(X, Y, rotations):
    """(S, 12): the start poses of gingr_rigid_search, (R0, mean Y - R0 mean X), with the translation in the order the header fixes --
    c - ((R0 mx0 + R1 mx1) + R2 mx2) in scalar float64, the means summed in index order.  rigid_search_restatement.start_poses writes
    R @ mx, which numpy hands to a BLAS routine whose order (and fused multiply-adds) is its own: on the femur pair 5 of 64 translations
    differ from this one in the last bit"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    mx, c = np.zeros(3), np.zeros(3)
    for row in X:
        mx = mx + row
    for row in Y:
        c = c + row
    mx, c = mx / np.float64(X.shape[0]), c / np.float64(Y.shape[0])
    out = np.empty((len(rotations), 12))
    for s, R in enumerate(np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)):
        out[s, :9] = R.reshape(9)
        for a in range(3):
            out[s, 9 + a] = c[a] - ((R[a, 0] * mx[0] + R[a, 1] * mx[1]) + R[a, 2] * mx[2])
    return out


def select_best(scores, inliers, failed, select):
    ok = np.nonzero(~np.asarray(failed))[0]
    if ok.size == 0:
        return -1
    if select == 0:
        return int(ok[np.argmin(np.asarray(scores)[ok])])
    key = sorted(ok, key=lambda s: (-int(inliers[s]), float(scores[s]), int(s)))
    return int(key[0])


def search_poses(X, Y, poses, K, rho=1.0, inlier_distance=0.0, select=0, dtype=np.float64):
    """dict(best, R, t, score, rotations, translations, scores, kept, failed, inliers): rigid_search_restatement's iteration from
    the given poses (S, 12); a non-finite start pose is failed from the beginning"""
    X, Y = np.asarray(X, dtype=dtype).reshape(-1, 3), np.asarray(Y, dtype=dtype).reshape(-1, 3)
    poses = np.asarray(poses, dtype=dtype).reshape(-1, 12)
    from scipy.spatial import cKDTree
    tree = cKDTree(Y.astype(np.float64))
    S = poses.shape[0]
    out = dict(rotations=poses[:, :9].reshape(S, 3, 3).copy(), translations=poses[:, 9:].copy(), scores=np.full(S, np.inf),
               kept=np.zeros(S, dtype=np.int64), failed=np.zeros(S, dtype=bool), inliers=np.zeros(S, dtype=np.int64))
    lim = dtype(inlier_distance) * dtype(inlier_distance)
    for s in range(S):
        if not np.isfinite(poses[s].astype(np.float64)).all():
            out["failed"][s] = True
            continue
        R, t, score, kept, failed = rs.iterate_pose(X, Y, out["rotations"][s], out["translations"][s], K, rho, tree)
        out["rotations"][s], out["translations"][s], out["scores"][s], out["kept"][s], out["failed"][s] = R, t, score, kept, failed
        if not failed:
            out["inliers"][s] = int((rs.nearest(X @ R.T + t, Y, tree)[1] <= lim).sum())
    best = select_best(out["scores"], out["inliers"], out["failed"], select)
    out["best"] = best
    if best >= 0:
        out.update(R=out["rotations"][best], t=out["translations"][best], score=float(out["scores"][best]))
    return out


# ------------------------------------------------------------------------------------------------ the pipeline
def subsample(template, max_points):
    M = template.shape[0]
    stride = -(-M // max_points) if M > max_points else 1
    return np.ascontiguousarray(template[::stride])


def draw_triples(pool, hypotheses, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(pool, 3, replace=False) for _ in range(hypotheses)]).astype(np.int64)


def edge_similar(X, Y, tri, match, similarity):
    """keep a triple when the smallest ratio, shorter over longer, of its three corresponding edge lengths is >= similarity"""
    a, b = X[tri], Y[match[tri]]
    keep = np.ones(tri.shape[0], dtype=bool)
    for p, q in ((0, 1), (0, 2), (1, 2)):
        la, lb = np.linalg.norm(a[:, p] - a[:, q], axis=1), np.linalg.norm(b[:, p] - b[:, q], axis=1)
        hi = np.maximum(la, lb)
        keep &= np.where(hi > 0, np.minimum(la, lb) / np.where(hi > 0, hi, 1.0), 0.0) >= similarity
    return keep


def mutual_pool(m_ab, m_ba, minimum=10):
    mutual = np.nonzero(m_ba[m_ab] == np.arange(m_ab.shape[0]))[0]
    return (mutual if mutual.size >= minimum else np.arange(m_ab.shape[0])), int(mutual.size)


def align(template, target, radius, normals_k=12, descriptor_k=64, hypotheses=2000, edge_similarity=0.8, inlier_distance=3.0,
          overlap=0.6, refine_iterations=30, max_points=2000, seed=0, descriptors=None):
    """dict(R, t, hypothesis (R, t), match, triples, kept, pool, inliers, info): the whole route of classic.FeatureRigidAlignment.
    descriptors = (fa, fb) replaces the two descriptor arrays (a GPU test hands over the device's own)"""
    X, Y = subsample(np.ascontiguousarray(template, dtype=np.float64), max_points), np.ascontiguousarray(target, dtype=np.float64)
    if descriptors is None:
        fa = fpfh(X, normals(X, normals_k, X.mean(0)), min(descriptor_k, X.shape[0]), radius)["fpfh"]
        fb = fpfh(Y, normals(Y, normals_k, Y.mean(0)), min(descriptor_k, Y.shape[0]), radius)["fpfh"]
    else:
        fa, fb = descriptors
    m_ab, m_ba = feature_match(fa, fb)[0], feature_match(fb, fa)[0]
    pool, n_mutual = mutual_pool(m_ab, m_ba)
    tri = draw_triples(pool, hypotheses, seed)
    keep = edge_similar(X, Y, tri, m_ab, edge_similarity)
    tri = tri[keep]
    if tri.shape[0] == 0:
        raise ValueError("no triple passed the edge test")
    poses, deg = poses_from_triples(X, Y, tri, m_ab[tri])
    scored = search_poses(X, Y, poses, 0, 1.0, inlier_distance, 1)
    b = scored["best"]
    refined = search_poses(X, Y, poses[b:b + 1], refine_iterations, overlap, inlier_distance, 1)
    return dict(R=refined["R"], t=refined["t"], hypothesis=(scored["R"], scored["t"]), match=m_ab, triples=tri, best=b,
                inliers=int(scored["inliers"][b]),
                info=dict(matches=int(m_ab.shape[0]), mutual=n_mutual, drawn=int(hypotheses), kept=int(tri.shape[0]),
                          degenerate=int(deg.sum()), inliers=int(scored["inliers"][b])))


# ------------------------------------------------------------------------------------------------ the partial inputs
def partial_target(tgt):
    """the target without its lower third along its longest axis (examples/demo_robust_icp.py)"""
    axis = int(np.argmax(tgt.max(0) - tgt.min(0)))
    cut = tgt[:, axis].min() + (tgt[:, axis].max() - tgt[:, axis].min()) / 3.0
    return np.ascontiguousarray(tgt[tgt[:, axis] >= cut])


def partial_case(seed, clutter=False):
    """(template, target, R_true, t_true, part): recovery_case with the target's lower third cut away before the motion; part is the
    cut target where the template lies"""
    tpl, _, R, shift = rs.recovery_case(seed, clutter)
    part = partial_target(rs.femur_pair()[1])
    return tpl, part @ R.T + shift, R, shift, part
