"""numpy restatement of the point-to-plane pairs of the fitter (gingr_fitter_set_pairs_plane_async / gingr_fitter_update_plane_async,
gingr_amd/csrc/fitter_pairs.hip: plane_pairs_kernel, plane_schedule_kernel), in the precision the caller names:

  correspondence  go.mesh_closest_point's scan with the winning triangle kept (ties: the lowest triangle index), the weights of
                  go.surface_correspondence
  normal          n_t = (b - a) x (c - a) / |.| of the winning triangle; zero for a degenerate triangle
  planes          Lambda_i = (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T,  xbar_i = closest point;  rejected: both zero
                  v_n = sigma2, v_t = ratio sigma2 -- the closed-form inverse of v_t I + (v_n - v_t) n n^T
  schedule        sigma2 <- max(sigma2 - (initial - end) / max_iterations, end)
  update          the oracle's landmark route, one full covariance per observed vertex (go.update_from_observations)

and the triangle quality kappa_t = |e1| |e2| / |e1 x e2| that the element-wise bound of the GPU test is stated in."""
import numpy as np

from oracle import gingr_oracle as go
from tests import pairs_cov_gram_restatement as pr

U53 = pr.U53
NONE_ISO = (np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros(0))


def closest_triangles(P, verts, tris, near=64 * U53):
    """(closest points, squared distances, winning triangle, candidates): go.mesh_closest_point with the argmin kept.  candidates[i]:
    every triangle whose distance is within a relative `near` of the minimum (a closest point on a shared edge or vertex: which of the
    triangles around it wins is decided by the last bit of two differently rounded distances)"""
    A, B, C = verts[tris[:, 0]], verts[tris[:, 1]], verts[tris[:, 2]]
    pts, d2 = np.empty((P.shape[0], 3)), np.empty(P.shape[0])
    win, cands = np.empty(P.shape[0], dtype=np.int64), []
    for i in range(P.shape[0]):
        q = go.closest_point_on_triangles(P[i], A, B, C)
        dd = q - P[i]
        dist = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
        dist = np.where(np.isnan(dist), np.inf, dist)
        t = int(np.argmin(dist))
        pts[i], d2[i], win[i] = q[t], dist[t], t
        cands.append(np.flatnonzero(dist <= dist[t] * (1.0 + near) + 1e-300))
    return pts, d2, win, cands


def unit_normals(verts, tris, dtype=np.longdouble):
    """(T, 3) unit cell normals in `dtype`; zero for a triangle without area"""
    v = np.asarray(verts, dtype=dtype)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    length = np.sqrt((n * n).sum(1))
    out = np.zeros_like(n)
    ok = length > 0
    out[ok] = n[ok] / length[ok][:, None]
    return out


def kappa(verts, tris):
    """|e1| |e2| / |e1 x e2| per triangle (inf for a triangle without area): how much the rounding of the corners is magnified in the
    unit normal"""
    e1, e2 = verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]]
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    with np.errstate(divide="ignore"):
        return np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / area2


def closed_form(normals, v_n, ratio, dtype=np.float64):
    """(K, 3, 3): (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T with the operations of the kernel, in `dtype`"""
    n = np.asarray(normals, dtype=dtype)
    vn = dtype(v_n)
    vt = dtype(ratio) * vn
    a = dtype(1) / vt
    b = dtype(1) / vn - a
    bn = b * n
    L = a * np.eye(3, dtype=dtype)[None] + bn[:, :, None] * n[:, None, :]
    for r, s in ((1, 0), (2, 0), (2, 1)):  # six planes: the upper triangle ((b n_r) n_s, r <= s) is what is stored
        L[:, r, s] = L[:, s, r]
    return L


def covariances(normals, v_n, ratio, dtype=np.float64):
    """(K, 3, 3): v_t I + (v_n - v_t) n n^T of unit (or zero) normals"""
    n = np.asarray(normals, dtype=dtype)
    vn = dtype(v_n)
    vt = dtype(ratio) * vn
    return vt * np.eye(3, dtype=dtype)[None] + (vn - vt) * (n[:, :, None] * n[:, None, :])


def correspondence(fit, cells, target, tcells):
    """(closest points, 0/1 weights, winning triangle, candidates) of the forward TriangularClosestPoint correspondence"""
    cp, w, _ = go.surface_correspondence(fit, cells, target, tcells)
    cp2, _, win, cands = closest_triangles(fit, target, tcells)
    assert np.array_equal(cp, cp2)
    return cp, w, win, cands


def planes(cp, w, normals, sigma2, ratio, reject, dtype=np.float64):
    """(xbar (M, 3), Lambda (M, 3, 3)) from the closest points, the 0/1 weights and the winning triangles' normals"""
    L = closed_form(normals, sigma2, ratio, dtype)
    x = np.asarray(cp, dtype=dtype).copy()
    if reject:
        L[w == 0.0] = 0
        x[w == 0.0] = 0
    return x, L


def schedule(sigma2, initial, end, max_iterations):
    return max(sigma2 - (initial - end) / float(max_iterations), end)


def oracle_update(mo, cells, target, tcells, st, ratio, reject, sched, landmarks=None):
    """one point-to-plane update by the oracle's landmark route: every observed vertex with its closest point and the covariance
    v_t I + (v_n - v_t) n n^T; a vertex a landmark overrides loses its plane.  -> (next state, (cp, w, win))"""
    cp, w, win, _ = correspondence(st.fit, cells, target, tcells)
    nrm = unit_normals(target, tcells, np.float64)[win]
    covs = covariances(nrm, st.sigma2, ratio)
    pids = np.flatnonzero(w == 1.0) if reject else np.arange(cp.shape[0])
    if landmarks is not None:
        pids = pids[~np.isin(pids, landmarks.pids)]
        lm = go.Landmarks(np.concatenate([pids, landmarks.pids]), np.concatenate([cp[pids], landmarks.points]),
                          np.concatenate([covs[pids], landmarks.covs]))
    else:
        lm = go.Landmarks(pids, cp[pids], covs[pids])
    return go.update_from_observations(mo, st, *NONE_ISO, schedule(st.sigma2, *sched), landmarks=lm), (cp, w, win)
