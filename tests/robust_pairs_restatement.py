"""numpy restatement of the robust (M-estimator) weighting of the point-to-plane pairs (gingr_fitter_set_plane_robust,
gingr_amd/csrc/fitter_pairs.hip: plane_residual_kernel, plane_pairs_robust_kernel; the median: robust_select.hip), in the precision
the caller names.  The definition is the package's own:

  residual   s_i = e_n^2 + max(|d_i|^2 - e_n^2, 0) / rho,  d_i = fit vertex - observed point, e_n = n_i . d_i, n_i the unit (or zero)
             normal of the vertex's plane, rho = tangent_over_normal  -- sigma2 d^T Lambda d of the plane the vertex gets
  scale      c fixed, or c = tuning * 1.4826 * sqrt(s_(k)), s_(k) the k-th smallest s_i over the n observed vertices, k = (n - 1) // 2;
             then c = max(c, min_scale); n = 0 or c = 0: u = 1 everywhere
  inflation  cauchy u = 1 + s / c^2;  huber u = max(1, sqrt(s) / c);  tukey: s >= c^2 removes the vertex (u = 0 here), else
             u = 1 / (1 - s / c^2)^2.  The vertex is observed with the plane of variance sigma2 * u along its normal
  update     the oracle's landmark route, one full covariance per vertex that is still observed (go.update_from_observations)
"""
import numpy as np

from oracle import gingr_oracle as go
from tests import cloud_normals_restatement as cr
from tests import plane_pairs_restatement as pp

LOSSES = {"cauchy": 1, "huber": 2, "tukey": 3}
TUNINGS = {"cauchy": 2.385, "huber": 1.345, "tukey": 4.685}
MAD = 1.4826


def residual(d, normals, ratio, dtype=np.float64):
    """(K,) s of the differences d (K, 3) and the unit-or-zero normals (K, 3), in `dtype`"""
    d, n = np.asarray(d, dtype=dtype), np.asarray(normals, dtype=dtype)
    d2 = (d * d).sum(1)
    en = (n * d).sum(1)
    tang = np.maximum(d2 - en * en, dtype(0))
    return en * en + tang / dtype(ratio)


def lower_median(s):
    """the k-th smallest of s, k = (n - 1) // 2: an element of the data"""
    s = np.asarray(s)
    return np.partition(s, (s.shape[0] - 1) // 2)[(s.shape[0] - 1) // 2]


def scale(s_observed, mode, value, min_scale=0.0):
    """(selected, c) in float64, by the operations of the device: (value * 1.4826) * sqrt(selected)"""
    s_observed = np.asarray(s_observed, dtype=np.float64)
    if s_observed.shape[0] == 0:
        return 0.0, 0.0
    selected = float(lower_median(s_observed))
    c = float(value) if mode == 0 else float((np.float64(value) * np.float64(MAD)) * np.sqrt(np.float64(selected)))
    return selected, max(c, float(min_scale))


def inflation(kind, s, c, dtype=np.float64):
    """(K,) u >= 1; 0 where Tukey removes the vertex"""
    s = np.asarray(s, dtype=dtype)
    if not c > 0:
        return np.ones_like(s)
    c = dtype(c)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "huber":
            return np.maximum(np.sqrt(s) / c, dtype(1))
        r = s / (c * c)
        if kind == "cauchy":
            return dtype(1) + r
        w = dtype(1) - r
        return np.where(s >= c * c, dtype(0), dtype(1) / (w * w))


def weigh(fit, points, normals, seen, ratio, kind, mode, value, min_scale=0.0, dtype=np.float64):
    """(s (M,), u (M,), selected, c, n): s and u are 0 where `seen` is False; the scale from the float64 residuals"""
    s64 = np.where(seen, residual(np.asarray(fit) - np.asarray(points), normals, ratio), 0.0)
    selected, c = scale(s64[seen], mode, value, min_scale)
    s = np.where(seen, residual(np.asarray(fit) - np.asarray(points), normals, ratio, dtype), dtype(0))
    u = np.where(seen, inflation(kind, s, c, dtype), dtype(0))
    return s, u, selected, c, int(np.count_nonzero(seen))


def covariances(normals, sigma2, u, ratio):
    """(K, 3, 3): v_t I + (v_n - v_t) n n^T at v_n = sigma2 u_k per vertex"""
    n = np.asarray(normals, dtype=np.float64)
    vn = float(sigma2) * np.asarray(u, dtype=np.float64)
    vt = float(ratio) * vn
    return vt[:, None, None] * np.eye(3)[None] + (vn - vt)[:, None, None] * (n[:, :, None] * n[:, None, :])


def oracle_update_surface(mo, cells, target, tcells, st, ratio, reject, sched, loss):
    """one robust point-to-plane update against a mesh by the oracle's landmark route; loss = (kind, mode, value, min_scale) or None.
    -> (next state, (cp, seen, u))"""
    cp, w, win, _ = pp.correspondence(st.fit, cells, target, tcells)
    nrm = pp.unit_normals(target, tcells, np.float64)[win]
    seen = (w == 1.0) if reject else np.ones(cp.shape[0], bool)
    u = np.where(seen, 1.0, 0.0) if loss is None else weigh(st.fit, cp, nrm, seen, ratio, *loss)[1]
    pids = np.flatnonzero(u > 0)
    lm = go.Landmarks(pids, cp[pids], covariances(nrm[pids], st.sigma2, u[pids], ratio))
    return go.update_from_observations(mo, st, *pp.NONE_ISO, pp.schedule(st.sigma2, *sched), landmarks=lm), (cp, seen, u)


def oracle_update_cloud(mo, target, tnormals, st, ratio, sched, loss, max_distance=0.0):
    """the same against a point cloud with a normal per target point -> (next state, (nn, seen, u))"""
    nn, d2 = cr.nearest(st.fit, target)
    cp, nrm = target[nn], np.asarray(tnormals, dtype=np.float64)[nn]
    seen = np.ones(nn.shape[0], bool) if not max_distance > 0 else ~(d2 > max_distance * max_distance)
    u = np.where(seen, 1.0, 0.0) if loss is None else weigh(st.fit, cp, nrm, seen, ratio, *loss)[1]
    pids = np.flatnonzero(u > 0)
    lm = go.Landmarks(pids, cp[pids], covariances(nrm[pids], st.sigma2, u[pids], ratio))
    return go.update_from_observations(mo, st, *pp.NONE_ISO, pp.schedule(st.sigma2, *sched), landmarks=lm), (nn, seen, u)
