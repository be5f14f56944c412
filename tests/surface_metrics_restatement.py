"""numpy restatement of the surface-distance model metrics (gingr_amd/csrc/surface_metrics.hip) and the bounds the device results are
held to.  Not a test module: tests/test_surface_metrics_host.py and tests/test_gpu_surface_metrics.py import it.

Definition.  The surface distance of a model-side mesh A (a projection or a sample) to a data shape B with the same triangles `cells`:
for every vertex p of A, d(p) = |p - closestPointOnSurface_B(p)| (oracle/gingr_oracle.py: mesh_closest_point, Ericson 5.1.5 over every
triangle); avg = the mean over the vertices, max = the largest.  Model side -> data surface.  The projections and samples are those of
tests/model_metrics_restatement.py (longdouble, rounded to float64 before the closest-point query).
"""
import numpy as np

from oracle import gingr_oracle as go
from tests import model_metrics_restatement as mm

U = mm.U


def distances(A, B, cells, closest=go.mesh_closest_point):
    """(M,) d(p) for the rows p of A against the mesh (B, cells).  closest: (points, verts, cells) -> (points, squared distances, ...)"""
    d2 = closest(np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64), np.asarray(cells))[1]
    return np.sqrt(d2)


def avg_max(A, B, cells, closest=go.mesh_closest_point):
    d = distances(A, B, cells, closest)
    return float(d.sum() / d.shape[0]), float(d.max())


def set_distances(sets, meshes, cells, pairing="all", closest=go.mesh_closest_point):
    """avg, max: (n_sets, n_meshes) for "all"; (n_sets,) for "cyclic" (set c against mesh c % n_meshes)"""
    sets, meshes = np.asarray(sets, dtype=np.float64), np.asarray(meshes, dtype=np.float64)
    if pairing == "all":
        out = np.array([[avg_max(s, m, cells, closest) for m in meshes] for s in sets])
        return out[:, :, 0], out[:, :, 1]
    out = np.array([avg_max(s, meshes[c % meshes.shape[0]], cells, closest) for c, s in enumerate(sets)])
    return out[:, 0], out[:, 1]


def generalization(model, shapes, cells, ranks, closest=go.mesh_closest_point):
    """coef [n_ranks, n, r] (longdouble, project_direct), avg, max [n_ranks, n]: projection (i, k) against the surface of shape i"""
    shapes = np.asarray(shapes, dtype=np.float64).reshape(-1, model.M, 3)
    coef = mm.project_direct(model, shapes, ranks)[0]
    avg, mx = np.zeros(coef.shape[:2]), np.zeros(coef.shape[:2])
    for q in range(len(ranks)):
        proj = np.asarray(mm.instances(model, coef[q]), dtype=np.float64)
        for i in range(shapes.shape[0]):
            avg[q, i], mx[q, i] = avg_max(proj[i], shapes[i], cells, closest)
    return coef, avg, mx


def specificity(model, train, alphas, cells, ranks, closest=go.mesh_closest_point):
    """means [n_ranks, S, n_train], min_avg [n_ranks, S], argmin [n_ranks, S] (the lowest index on an exact tie: np.argmin)"""
    train = np.asarray(train, dtype=np.float64).reshape(-1, model.M, 3)
    S = np.asarray(alphas).reshape(-1, model.rank).shape[0]
    means = np.zeros((len(ranks), S, train.shape[0]))
    for q, k in enumerate(ranks):
        smp = np.asarray(mm.instances(model, mm.truncated(alphas, k)), dtype=np.float64)
        means[q] = set_distances(smp, train, cells, "all", closest)[0]
    return means, means.min(axis=-1), means.argmin(axis=-1)


# ------------------------------------------------------------------------------------------------------------------- the bounds
def summation_term(M, avg):
    """two sums of the same M terms in different orders differ by at most gamma_M = M u / (1 - M u) of the sum"""
    return M * U / (1.0 - M * U) * np.abs(avg)


def query_bound(model, alphas):
    """(n,): how far a computed instance lies from another computed (or the exact) instance of the same coefficients, per vertex at
    most: sqrt(3) times the largest per-coordinate bound of mm.instance_bound.  The closest-point distance is 1-Lipschitz in the query,
    so d, its maximum and its mean over the vertices move by no more."""
    return np.sqrt(3.0) * mm.instance_bound(model, alphas).reshape(np.asarray(alphas).reshape(-1, model.rank).shape[0], -1).max(axis=1)


def grid_mesh(gx, gy, jitter=0.0, seed=0, spacing=1.0):
    """(points (gx gy, 3), cells (2 (gx - 1)(gy - 1), 3)): a triangulated gx x gy grid in the plane z = 0, in-plane and out-of-plane
    jitter of `jitter` spacings (normal)"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(gx, dtype=np.float64), np.arange(gy, dtype=np.float64), indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), np.zeros(gx * gy)], axis=1) * spacing
    if jitter:
        pts = pts + rng.normal(0.0, jitter * spacing, pts.shape)
    idx = np.arange(gx * gy).reshape(gx, gy)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    cells = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)]).astype(np.int32)
    return pts, cells


def grid_model(gx, gy, r, seed, spacing=10.0):
    """a model on a jittered grid reference (so that its shapes are meshes): random basis columns of norm about 1, variances within
    [0.25, 64] (mm.variances), and the grid's cells"""
    ref, cells = grid_mesh(gx, gy, 0.15, seed, spacing)
    rng = np.random.default_rng(seed + 1)
    M = ref.shape[0]
    mean = rng.normal(0.0, 1.0, (M, 3))
    basis = rng.normal(0.0, 1.0, (3 * M, r)) / np.sqrt(3.0 * M)
    return mm.Model(ref, mean, basis, mm.variances(r)), cells


def specificity_block_case():
    """(model, cells, training shapes, alphas, ranks) of the 513-sample specificity check of tests/test_gpu_surface_metrics.py: small
    enough (M = 12, four shapes) for the numpy oracle to restate every pair on the CPU"""
    mo, cells = grid_model(4, 3, 5, 21)
    rng = np.random.default_rng(22)
    train = np.asarray(mm.instances(mo, rng.standard_normal((4, 5))), dtype=np.float64) + rng.normal(0.0, 0.3, (4, mo.M, 3))
    return mo, cells, train, rng.standard_normal((513, 5)), [2, 5]
