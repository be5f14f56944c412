"""numpy restatement of the dense covariance pairs of the fitter (gingr_fitter_set_pairs_cov_dense, gingr_amd/csrc/fitter_pairs.hip and
gp_gram_cov.hip), in the precision the caller names (float64 as the device, np.longdouble as the reference of the element-wise tests):

  consolidation   Lambda_i = sum_k Sigma_k^-1,  xbar_i = Lambda_i^-1 sum_k Sigma_k^-1 x_k   (ascending pair position; one pair: its point)
  per update      W_i = R^T Lambda_i R,  v_i = R^T (xbar_i - c - t) - (ref_i - c + mean_i)
                  G = sum_i Q_i^T W_i Q_i,  rhs = sum_i Q_i^T W_i v_i          Q_i: the 3 x r block of vertex i in U sqrt(lam)
  posterior       a = (G + I)^-1 rhs,  mean mesh = R (ref - c + mean + Q a) + c + t

and the plain summation bound of the element-wise tests, and the slab plan of gram_cov_plan.h."""
import numpy as np

U53 = 2.0 ** -53
MIN_SLAB_VERTS, SLAB_QUANTUM, WANT_WORKGROUPS, MAX_SLABS, PATCH = 64, 16, 768, 768, 64


def inverse3(C):
    """(..., 3, 3) inverses by cofactors, in the dtype of C (np.linalg has no extended precision)"""
    C = np.asarray(C)
    a, b, c, d, e, f, g, h, i = (C[..., r, s] for r in range(3) for s in range(3))
    co = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], -1),
                   np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                   np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return co / det[..., None, None]


def consolidate(M, pids, pts, covs, dtype=np.float64):
    """(xbar (M, 3), Lambda (M, 3, 3), pairs per vertex (M,)): the definition, per vertex in ascending pair position"""
    pids = np.asarray(pids, dtype=np.int64)
    pts, covs = np.asarray(pts, dtype=dtype).reshape(-1, 3), np.asarray(covs, dtype=dtype).reshape(-1, 3, 3)
    covs = 0.5 * (covs + np.swapaxes(covs, 1, 2))
    prec = inverse3(covs) if pids.shape[0] else np.zeros((0, 3, 3), dtype=dtype)
    L, b, n = np.zeros((M, 3, 3), dtype=dtype), np.zeros((M, 3), dtype=dtype), np.zeros(M, dtype=np.int64)
    last = np.zeros((M, 3), dtype=dtype)
    for k in range(pids.shape[0]):
        i = pids[k]
        L[i] += prec[k]
        b[i] += prec[k] @ pts[k]
        last[i] = pts[k]
        n[i] += 1
    obs = np.zeros((M, 3), dtype=dtype)
    many = n > 1
    obs[many] = np.einsum("mab,mb->ma", inverse3(L[many]), b[many]) if many.any() else obs[many]
    obs[n == 1] = last[n == 1]
    return obs, L, n


def prec6(L):
    return np.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], axis=1)


def model_basis(mo, dtype=np.float64):
    """Q (M, 3, r) = U sqrt(lam)"""
    return (np.asarray(mo.U, dtype=dtype) * np.sqrt(np.asarray(mo.lam, dtype=dtype))[None, :]).reshape(mo.M, 3, mo.rank)


def posed_terms(mo, R, center, t, obs, L, dtype=np.float64, masked=None):
    """(W (M, 3, 3), v (M, 3)); masked: vertices a landmark overrides (their rows are zero).  v of a vertex without pairs is zero."""
    R, c, t = np.asarray(R, dtype=dtype), np.asarray(center, dtype=dtype), np.asarray(t, dtype=dtype)
    L = np.asarray(L, dtype=dtype).copy()
    if masked is not None:
        L[np.asarray(masked, dtype=np.int64)] = 0
    W = np.einsum("ia,mij,jb->mab", R, L, R)
    v = (np.asarray(obs, dtype=dtype) - c - t) @ R - (np.asarray(mo.ref, dtype=dtype) - c + np.asarray(mo.mean, dtype=dtype))
    v[~L.any(axis=(1, 2))] = 0
    return W, v


def system(Q, W, v):
    """(G (r, r), rhs (r,)) in the dtype of the inputs"""
    M, _, r = Q.shape
    WQ = np.einsum("mde,mea->mda", W, Q).reshape(3 * M, r)
    return Q.reshape(3 * M, r).T @ WQ, WQ.T @ np.asarray(v).reshape(3 * M)


def bounds(Q, W, v, M):
    """Per-entry bounds of the element-wise tests: (3 M + 32) u sum_i 3 |W_i|_2 |Q_i[:, a]|_2 |Q_i[:, b]|_2, and for rhs with |v_i|_2 in
    place of one column norm"""
    Q64, W64, v64 = np.asarray(Q, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(v, dtype=np.float64)
    wn = np.linalg.norm(W64, 2, axis=(1, 2))
    cn = np.linalg.norm(Q64, axis=1)                    # (M, r)
    f = (3 * M + 32) * U53 * 3.0
    return f * np.einsum("m,ma,mb->ab", wn, cn, cn), f * np.einsum("m,ma,m->a", wn, cn, np.linalg.norm(v64, axis=1))


def posterior(mo, R, center, t, G, rhs):
    """(coefficients a, posterior mean mesh in the world frame)"""
    a = np.linalg.solve(np.asarray(G, dtype=np.float64) + np.eye(mo.rank), np.asarray(rhs, dtype=np.float64))
    c = np.asarray(center, dtype=np.float64)
    shape = mo.ref - c + mo.mean + (model_basis(mo) @ a)
    return a, shape @ np.asarray(R).T + c + np.asarray(t)


def normal_tangent(normals, var_normal, var_tangent):
    """the definition of registration.normalTangentCovariances, pair by pair"""
    n = np.asarray(normals, dtype=np.float64)
    K = n.shape[0]
    vn, vt = np.broadcast_to(np.asarray(var_normal, dtype=np.float64), (K,)), np.broadcast_to(np.asarray(var_tangent, dtype=np.float64), (K,))
    out = np.empty((K, 3, 3))
    for k in range(K):
        length = np.linalg.norm(n[k])
        u = n[k] / length if length > 0 else np.zeros(3)
        out[k] = vt[k] * np.eye(3) + (vn[k] - vt[k]) * np.outer(u, u)
    return out


# (rank, M) of the element-wise GPU test: every rank at two M, every M at two ranks.  M = 1, 3, 5: fewer vertices than one K-step;
# 63, 64, 65: around the smallest slab (65 is the first size with two slabs); 259 and 4 099: several slabs, the last one short
GPU_RANKS = [1, 16, 17, 100, 112, 113, 128, 512]
GPU_SHAPES = ([(r, 65) for r in GPU_RANKS] +
              [(1, 4099), (16, 64), (17, 4099), (100, 4099), (112, 63), (113, 259), (128, 259), (512, 259)] +
              [(16, 1), (100, 1), (17, 3), (113, 3), (1, 5), (128, 5), (16, 63), (113, 64)])


def padded(rank):
    return -(-rank // 16) * 16


def plan(M, rp):
    """(patches per side, upper patches, slabs, vertices per slab) of gram_cov_plan::make_plan"""
    nbp = -(-rp // PATCH)
    npatch = nbp * (nbp + 1) // 2
    want = max(1, min(WANT_WORKGROUPS // npatch, -(-M // MIN_SLAB_VERTS), MAX_SLABS))
    vps = -(-(-(-M // want)) // SLAB_QUANTUM) * SLAB_QUANTUM
    return nbp, npatch, -(-M // vps), vps
