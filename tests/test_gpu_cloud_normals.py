"""GPU tests of the k nearest neighbours of a cloud within itself and of the normals from them (gingr_cloud_knn / gingr_cloud_normals,
gingr_amd/csrc/cloud_knn.hip; Context.cloud_knn / Context.cloud_normals).

Lists: idx element for element and d2 bit for bit against the brute-force restatement (tests/cloud_normals_restatement.py), on inputs
that take the grid path alone (info.flagged == 0) and on inputs that need the scan of the whole cloud (info.flagged > 0).
Normals: sin of the angle to the np.longdouble restatement's normal at most B_j = 64 (k + 2) u d_k^2 / (lam1 - lam0), u = 2^-53, d_k^2 the
k-th neighbour's squared distance and lam the longdouble eigenvalues -- Davis-Kahan's 2 |E| / gap with the rounding of the k centred
second moments (each entry a sum of k products of differences no longer than d_k) in |E|.  Every point with relative gap (lam1 - lam0) /
lam2 >= 0.05 is judged, and the inputs are such that none is left out.  variation within B_j (lam1 - lam0) / trace + 16 u.
Largest error / bound ratio seen on an MI355X: DESIGN.md section 4."""
import functools

import numpy as np
import pytest

from tests import cloud_normals_restatement as cr
from tests.test_gpu_surface_icp import femur, grid_mesh

pytestmark = pytest.mark.gpu

ERR_BAD_ARGUMENT, ERR_NONFINITE = 1, 3
KS = (3, 8, 16, 33, 64)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def cloud(name):
    if name.startswith("uniform"):
        return np.random.default_rng(int(name[7:])).uniform(-1.0, 1.0, (int(name[7:]), 3))
    if name == "femur":
        return np.ascontiguousarray(femur()[2])
    if name == "lattice":                                                  # exact ties, decided by index
        g = np.arange(12.0)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng({"duplicates": 1, "sheet": 2, "outliers": 3, "crowded": 4}[name])
    if name == "duplicates":                                               # 40 exact copies of one point among 600
        x = rng.uniform(-1.0, 1.0, (600, 3))
        x[rng.permutation(600)[:40]] = x[17]
        return x
    if name == "sheet":                                                    # z = 0: the grid is one cell thick
        return np.concatenate([rng.uniform(-3.0, 3.0, (1500, 2)), np.zeros((1500, 1))], 1)
    if name == "outliers":                                                 # a blob and five points 10^4 widths away
        far = 1e4 * np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, -1.0, 0], [1.0, 1.0, 1.0]])
        return np.concatenate([rng.uniform(-0.5, 0.5, (2000, 3)), far])[rng.permutation(2005)]
    if name == "crowded":                                                  # 1 500 coincident points in one cell, 500 spread ones
        x = np.concatenate([np.broadcast_to([0.25, -0.5, 0.125], (1500, 3)), rng.uniform(-1.0, 1.0, (500, 3))])
        return np.ascontiguousarray(x[rng.permutation(2000)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def lists(name):
    """the restatement's lists at the largest k the cloud allows; a smaller k is their first k columns (a stable sort)"""
    x = cloud(name)
    return cr.knn(x, min(64, x.shape[0]))


UNIFORM = ["uniform3", "uniform16", "uniform17", "uniform255", "uniform256", "uniform257", "uniform5000"]
FLAGGED = ["outliers", "crowded"]
OTHERS = ["femur", "lattice", "duplicates", "sheet"]
LIST_CASES = [(n, k) for n in UNIFORM for k in KS if k <= int(n[7:])] + [(n, k) for n in OTHERS + FLAGGED for k in (3, 16, 64)]


# ---------------------------------------------------------------------------------------------------------------- 1. lists
@pytest.mark.parametrize("name, k", LIST_CASES)
def test_lists_exactly(ctx, name, k):
    x = cloud(name)
    want_idx, want_d2 = (a[:, :k] for a in lists(name))
    info, again = {}, {}
    idx, d2 = ctx.cloud_knn(x, k, info)
    idx2, d22 = ctx.cloud_knn(x, k, again)
    print(f"{name} k {k}: cell {info['cell_size']:.4g}, grid {info['grid']}, flagged {info['flagged']} of {x.shape[0]}")
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(d2.view(np.uint64), want_d2.view(np.uint64))                      # bit for bit
    assert np.array_equal(idx, idx2) and np.array_equal(d2.view(np.uint64), d22.view(np.uint64)) and info == again
    if name in UNIFORM:
        assert info["flagged"] == 0                                                        # the grid path alone
    if name in FLAGGED:
        assert 0 < info["flagged"] <= x.shape[0]                                           # the scan of the whole cloud ran


# ---------------------------------------------------------------------------------------------------------------- 2. normals
@functools.lru_cache(maxsize=None)
def normal_input(name):
    if name == "femur":
        return cloud("femur")
    return np.ascontiguousarray(grid_mesh(*{"grid24": (24, 40.0, 6.0, 1), "grid17": (17, 40.0, 6.0, 3)}[name])[0])


@functools.lru_cache(maxsize=None)
def judged(name, k):
    x = normal_input(name)
    idx, d2 = cr.knn(x, k)
    n, var, lam, _ = cr.normals(x, k, dtype=np.longdouble, idx=idx)
    return x, idx, d2, n, var, lam


@pytest.mark.parametrize("k", [12, 16])
@pytest.mark.parametrize("name", ["femur", "grid24", "grid17"])
def test_normals_against_longdouble(ctx, name, k):
    x, idx, d2, n_ld, var_ld, lam = judged(name, k)
    n, var = ctx.cloud_normals(x, k)
    gap = (lam[:, 1] - lam[:, 0]).astype(np.float64)
    relgap = (gap / lam[:, 2].astype(np.float64))
    assert (relgap >= 0.05).all(), f"{(relgap < 0.05).sum()} points below the gap threshold: they would be left out"
    bound = 64.0 * (k + 2) * cr.U53 * d2[:, -1] / gap
    nl = n.astype(np.longdouble)
    sin = np.sqrt((np.cross(nl, n_ld) ** 2).sum(1)).astype(np.float64)
    ratio = sin / bound
    trace = lam.sum(1).astype(np.float64)
    vbound = bound * gap / trace + 16 * cr.U53
    vratio = np.abs(var.astype(np.longdouble) - var_ld).astype(np.float64) / vbound
    print(f"{name} k {k}: smallest relative gap {relgap.min():.3g}, worst sin / bound {ratio.max():.3e}, worst variation error / bound "
          f"{vratio.max():.3e}, largest |length - 1| {np.abs(np.linalg.norm(n, axis=1) - 1).max():.2e}")
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 8 * cr.U53                      # unit: the division and numpy's own norm
    assert ratio.max() <= 1.0 and vratio.max() <= 1.0
    # the canonical sign, element for element: the rule leaves the device's normals as they are, and they face the judge's
    assert np.array_equal(cr.canonical_sign(n), n) and ((nl * n_ld).sum(1) > 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. degenerate, sign
def test_degenerate_neighbourhoods(ctx):
    x = np.concatenate([np.broadcast_to([1.0, 2.0, 3.0], (30, 3)), np.random.default_rng(0).uniform(5.0, 9.0, (200, 3))])
    n, var = ctx.cloud_normals(x, 8)
    assert not n[:30].any() and np.isfinite(var).all() and not var[:30].any()             # all-coincident neighbourhoods
    line = np.stack([np.zeros(40), np.arange(40.0), np.zeros(40)], 1)                       # lattice points on an axis
    n, var = ctx.cloud_normals(line, 5)
    assert not n.any() and np.isfinite(var).all() and not var.any()


def test_exact_plane_lattice(ctx):
    g = np.arange(14.0)
    x = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), np.full((196, 1), 2.0)], 1)
    for k in (9, 16):
        n, var = ctx.cloud_normals(x, k)
        assert np.abs(np.abs(n) - np.array([0.0, 0.0, 1.0])).max() <= 1e-12 and (n[:, 2] > 0).all()
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12 and np.abs(var).max() <= 16 * cr.U53


def test_viewpoint_turns_every_normal_inward(ctx):
    u = np.random.default_rng(3).normal(0, 1, (1500, 3))
    x = 5.0 * u / np.linalg.norm(u, axis=1)[:, None] + np.array([10.0, -4.0, 2.0])
    c = np.array([10.0, -4.0, 2.0])
    free, _ = ctx.cloud_normals(x, 12)
    n, _ = ctx.cloud_normals(x, 12, viewpoint=c)
    assert (((c - x) * n).sum(1) > 0).all() and np.array_equal(np.abs(n), np.abs(free))
    assert ((np.abs(((x - c) / 5.0 * n).sum(1))) > 0.99).all()                              # and they are the sphere's normals
    assert not np.array_equal(n, free)


def test_argument_errors(ctx):
    from gingr_amd import _native as nat
    from gingr_amd._native import dptr, iptr
    x = np.random.default_rng(1).uniform(0, 1, (20, 3))
    lib, h = ctx._lib, ctx.handle
    idx, d2, nrm = np.full((20, 64), -7, dtype=np.int32), np.empty((20, 64)), np.full((20, 3), 7.0)
    for k in (2, 65, 21, 0, -1):
        assert lib.gingr_cloud_knn(h, 20, dptr(x), k, iptr(idx), dptr(d2), None) == ERR_BAD_ARGUMENT, k
        assert lib.gingr_cloud_normals(h, 20, dptr(x), k, None, dptr(nrm), None, None) == ERR_BAD_ARGUMENT, k
    assert lib.gingr_cloud_knn(h, 20, None, 3, iptr(idx), None, None) == ERR_BAD_ARGUMENT
    assert lib.gingr_cloud_knn(h, 0, dptr(x), 3, iptr(idx), None, None) == ERR_BAD_ARGUMENT
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[11, 1] = bad
        assert lib.gingr_cloud_knn(h, 20, dptr(y), 3, iptr(idx), dptr(d2), None) == ERR_NONFINITE
        assert lib.gingr_cloud_normals(h, 20, dptr(y), 3, None, dptr(nrm), None, None) == ERR_NONFINITE
    assert (idx == -7).all() and (nrm == 7.0).all()                                        # nothing was computed
    v = np.array([0.0, np.nan, 0.0])
    assert lib.gingr_cloud_normals(h, 20, dptr(x), 3, dptr(v), dptr(nrm), None, None) == ERR_NONFINITE
    with pytest.raises(nat.GingrNativeError):
        ctx.cloud_knn(x, 2)
    idx3, _ = ctx.cloud_knn(x, 20)                                                         # k = N is allowed: every point, sorted
    assert np.array_equal(np.sort(idx3, axis=1), np.broadcast_to(np.arange(20), (20, 20)))
