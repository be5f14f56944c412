"""numpy restatement of the k-nearest-neighbour normals of a cloud (gingr_cloud_knn / gingr_cloud_normals, gingr_amd/csrc/cloud_knn.hip)
and of point-to-plane ICP against a point cloud (gingr_fitter_set_pairs_plane_cloud_async / gingr_fitter_update_plane_cloud_async,
gingr_amd/csrc/fitter_pairs.hip: plane_cloud_pairs_kernel), in the precision the caller names:

  lists       per point j the k points with the smallest (d2, index), d2 = dx*dx + dy*dy + dz*dz in float64, by a stable sort
  moments     q_i = x_i - x_j, m = sum q_i / k, C = sum (q_i - m)(q_i - m)^T / k, both sums in list order
  normal      the unit eigenvector of the smallest eigenvalue of C; zero when lam1 - lam0 <= 2^-26 lam2; the component of largest
              magnitude positive (lowest axis on ties); with a viewpoint v turned so that n . (v - x_j) >= 0
  variation   lam0 / (lam0 + lam1 + lam2), 0 when the trace is 0
  planes      xbar_i = target[nn_i], Lambda_i = (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T of the target point's normal; a vertex with
              d2 > max_distance^2 is not observed
  update      the oracle's landmark route, one full covariance per observed vertex (go.update_from_observations)

np.longdouble is the judge of the GPU tests: numpy has no eigen-solver in that type, so the eigenpairs come from cyclic Jacobi rotations
written here (converged to the type's own rounding)."""
import numpy as np

from oracle import gingr_oracle as go
from tests import plane_pairs_restatement as pp

U53 = pp.U53
DEGENERATE = 2.0 ** -26


def d2_matrix_row(x, j):
    d = x - x[j]
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def knn(x, k):
    """(idx (N, k) int32, d2 (N, k)): brute force, a stable sort by d2 -- equal distances stay in index order"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N = x.shape[0]
    idx, d2 = np.empty((N, k), dtype=np.int32), np.empty((N, k))
    for j in range(N):
        row = d2_matrix_row(x, j)
        order = np.argsort(row, kind="stable")[:k]
        idx[j], d2[j] = order, row[order]
    return idx, d2


def nearest(fit, target):
    """(nn (M,), d2 (M,)): the brute-force argmin, lowest index on ties"""
    nn, d2 = np.empty(fit.shape[0], dtype=np.int64), np.empty(fit.shape[0])
    for i in range(fit.shape[0]):
        d = target - fit[i]
        row = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        nn[i] = int(np.argmin(row))
        d2[i] = row[nn[i]]
    return nn, d2


def moments(x, idx, dtype=np.float64):
    """C (N, 3, 3): the second central moments of the neighbourhoods, summed in list order in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    N, k = idx.shape
    q = x[idx] - x[:, None, :]
    m = np.zeros((N, 3), dtype=dtype)
    for i in range(k):
        m = m + q[:, i]
    m = m / dtype(k)
    C = np.zeros((N, 3, 3), dtype=dtype)
    for i in range(k):
        d = q[:, i] - m
        C = C + d[:, :, None] * d[:, None, :]
    return C / dtype(k)


def jacobi_eigh(C, sweeps=30):
    """(lam (N, 3) ascending, V (N, 3, 3) columns): cyclic Jacobi on a batch of symmetric 3 x 3 matrices in their own dtype"""
    A = np.array(C, copy=True)
    dtype = A.dtype.type
    N = A.shape[0]
    V = np.zeros((N, 3, 3), dtype=A.dtype)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = dtype(1)
    for _ in range(sweeps):
        moved = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[:, p, q]
            go_ = apq != 0
            if not go_.any():
                continue
            moved = True
            safe = np.where(go_, apq, dtype(1))
            with np.errstate(over="ignore"):                                   # (a huge theta: t = 0, no rotation)
                theta = (A[:, q, q] - A[:, p, p]) / (dtype(2) * safe)
                t = np.where(theta >= 0, dtype(1), dtype(-1)) / (np.abs(theta) + np.sqrt(theta * theta + dtype(1)))
            t = np.where(go_, t, dtype(0))
            c = dtype(1) / np.sqrt(t * t + dtype(1))
            s = t * c
            J = np.zeros((N, 3, 3), dtype=A.dtype)
            J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = dtype(1)
            J[:, p, p], J[:, q, q], J[:, p, q], J[:, q, p] = c, c, s, -s
            A = np.swapaxes(J, 1, 2) @ A @ J
            A[:, p, q] = A[:, q, p] = np.where(np.abs(A[:, p, q]) <= np.finfo(A.dtype).eps * dtype(0.25) *
                                               np.sqrt(np.abs(A[:, p, p] * A[:, q, q])), dtype(0), A[:, p, q])
            V = V @ J
        if not moved:
            break
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    order = np.argsort(lam, axis=1, kind="stable")
    lam = np.take_along_axis(lam, order, axis=1)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    return lam, V


def canonical_sign(n):
    """the component of largest magnitude positive, lowest axis on ties"""
    lead = np.argmax(np.abs(n), axis=1)                                    # (argmax: the first of equal entries)
    s = np.where(np.take_along_axis(n, lead[:, None], axis=1)[:, 0] < 0, -1, 1)
    return n * s[:, None].astype(n.dtype)


def normals(x, k, viewpoint=None, dtype=np.float64, idx=None):
    """(normals (N, 3), variation (N,), lam (N, 3), idx) in `dtype`"""
    if idx is None:
        idx = knn(x, k)[0]
    lam, V = jacobi_eigh(moments(x, idx, dtype))
    n = V[:, :, 0]
    n = canonical_sign(n / np.sqrt((n * n).sum(1))[:, None])
    trace = lam.sum(1)
    var = np.where(trace != 0, lam[:, 0] / np.where(trace != 0, trace, dtype(1)), dtype(0))
    n = np.where((lam[:, 1] - lam[:, 0] <= dtype(DEGENERATE) * lam[:, 2])[:, None], dtype(0), n)
    if viewpoint is not None:
        away = ((np.asarray(viewpoint, dtype=dtype)[None] - np.asarray(x, dtype=dtype)) * n).sum(1) < 0
        n = np.where(away[:, None], -n, n)
    return n, var, lam, idx


def cloud_planes(target, tnormals, nn, d2, sigma2, ratio, max_distance=0.0, dtype=np.float64):
    """(xbar (M, 3), Lambda (M, 3, 3), observed (M,) bool)"""
    L = pp.closed_form(tnormals[nn], sigma2, ratio, dtype)
    x = np.asarray(target, dtype=dtype)[nn].copy()
    seen = np.ones(nn.shape[0], bool) if not max_distance > 0 else ~(d2 > max_distance * max_distance)
    L[~seen] = 0
    x[~seen] = 0
    return x, L, seen


def oracle_update_cloud(mo, target, tnormals, st, ratio, sched, max_distance=0.0, landmarks=None):
    """one point-to-plane update against the cloud by the oracle's landmark route -- tests/plane_pairs_restatement.py: oracle_update with
    cp = target[nn] and the target points' normals.  -> (next state, (nn, d2, observed))"""
    nn, d2 = nearest(st.fit, target)
    cp = target[nn]
    covs = pp.covariances(np.asarray(tnormals, dtype=np.float64)[nn], st.sigma2, ratio)
    seen = np.ones(nn.shape[0], bool) if not max_distance > 0 else ~(d2 > max_distance * max_distance)
    pids = np.flatnonzero(seen)
    if landmarks is not None:
        pids = pids[~np.isin(pids, landmarks.pids)]
        lm = go.Landmarks(np.concatenate([pids, landmarks.pids]), np.concatenate([cp[pids], landmarks.points]),
                          np.concatenate([covs[pids], landmarks.covs]))
    else:
        lm = go.Landmarks(pids, cp[pids], covs[pids])
    return go.update_from_observations(mo, st, *pp.NONE_ISO, pp.schedule(st.sigma2, *sched), landmarks=lm), (nn, d2, seen)
