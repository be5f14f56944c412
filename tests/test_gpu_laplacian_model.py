"""gingr_model_from_laplacian / GPMMTriangleMesh3D.InverseLaplacianSpectral: the inverse-Laplacian model from the sparse graph
Laplacian's own smallest eigenpairs, against the dense numpy.linalg.eigh of L (the definition) and against the reference-parity
route (the oracle's model of LookupKernel(pinv(L)) built to 1e-10 and truncated).

Bounds: those of check_model_against_oracle as test_gpu_gpmm_kernels.py calls it -- variances 1e-8 relative in norm, |U^T U - I| < 1e-9,
covariance on 300 random rows 1e-8 of its largest entry.  Where they come from: the stop rule bounds a residual by 1e-10 Lambda ~
2e-9, the eigenvector error is at most residual / (absolute gap at the cut, >= 0.022 on these meshes) <= 1e-7, which moves a
covariance entry by ~ 1e-7 (1 / mu_k) / n against a largest entry of ~ (1 / mu_1) / n; eigenvalues are quadratic in the residual.
The cuts of the table are where the relative gap is at least 1 % (fixture facts: numpy eigvalsh of go.graph_laplacian)."""
import ctypes
import gc
import math
import os

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import lap_spectral_restatement as rs
from tests.test_gpu_gpmm_kernels import check_model_against_oracle, cov_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCALING = 30.0

_cache = {}


def mesh(name):
    if name not in _cache:
        if name == "femur":
            v, c = rs.femur_full()
        elif name == "small":
            v, c = rs.femur_small(220)
        elif name == "doubled":
            v, c = rs.doubled_with_isolated(*mesh("small")[:2])
        else:
            v, c = rs.tetrahedron()
        L = go.graph_laplacian(v.shape[0], c)
        mu, V = np.linalg.eigh(L)
        _cache[name] = (v, c, L, mu, V)
    return _cache[name]


def want_model(name, k, scaling=SCALING):
    v, c, L, mu, V = mesh(name)
    keep = np.nonzero(mu > rs.CUTOFF)[0][:k]
    assert keep.shape[0] == k
    return rs.expand(mu[keep], V[:, keep], scaling)


def build(ctx, name, k, **kw):
    import gingr_amd as ga
    v, c = mesh(name)[:2]
    return ga.GPMMTriangleMesh3D(ctx, v, cells=c).InverseLaplacianSpectral(SCALING, 3 * k, **kw)


def check_structure(host, k):
    """entries off a column's coordinate exactly 0.0; the x, y and z copies of a vector bit-identical"""
    U = np.asarray(host.basis)
    n = U.shape[0] // 3
    assert U.shape == (3 * n, 3 * k)
    B = U.reshape(n, 3, k, 3)
    for d in range(3):
        for e in range(3):
            if d != e:
                assert not B[:, d, :, e].any(), (d, e)
    assert np.array_equal(B[:, 0, :, 0], B[:, 1, :, 1]) and np.array_equal(B[:, 0, :, 0], B[:, 2, :, 2])
    lam = np.asarray(host.variance).reshape(k, 3)
    assert np.array_equal(lam[:, 0], lam[:, 1]) and np.array_equal(lam[:, 0], lam[:, 2])
    assert np.all(np.diff(lam[:, 0]) <= 0)
    # sign: the component of largest magnitude of every vector is positive
    V = B[:, 0, :, 0]
    assert np.all(V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0)


# ---- 1. against the dense eigen-decomposition: the five (mesh, k) rows of the fixture table, with the table's relative gap at the cut
@pytest.mark.parametrize("name,k,gap", [("femur", 4, 0.43), ("femur", 34, 0.053), ("femur", 170, 0.011), ("small", 8, 0.148), ("small", 33, 0.073)])
def test_against_the_dense_eigendecomposition(ctx, name, k, gap):
    mu = mesh(name)[3]
    true_gap = (mu[k + 1] - mu[k]) / mu[k]                   # (one null vector in front)
    assert abs(true_gap - gap) < 0.05 * gap                   # the fixture facts hold
    dm = build(ctx, name, k)
    info = dm.laplacianInfo
    print(name, k, info)
    assert dm.rank == 3 * k and info.converged and info.n_components == 1 and info.n_dropped == 1
    assert info.max_residual <= 1e-10 and info.block_columns % 16 == 0 and k < info.block_columns <= 192
    assert abs(info.cut_gap - gap) < 0.1 * gap
    host = dm.to_host()
    assert not np.asarray(host.mean).any() and np.array_equal(host.reference, mesh(name)[0])
    check_model_against_oracle(host, want_model(name, k), tol_lam=1e-8, tol_cov=1e-8)
    check_structure(host, k)


# ---- 2. against the reference-parity route: the oracle's lookup-kernel model built to 1e-10, its first 24 components
def test_against_the_reference_route_truncated(ctx):
    v, c, L = mesh("small")[:3]
    full = go.build_gpmm_diagonal(v, go.lookup_kernel_fun(go.pinv_svd(L), SCALING), 1e-10, None)
    assert full.rank >= 24
    want = rs.Model(24, full.lam[:24], full.U[:, :24])
    # (the oracle's triples come in its own order inside a triple: the model is compared through variances and covariance)
    check_model_against_oracle(build(ctx, "small", 8).to_host(), want, tol_lam=1e-8, tol_cov=1e-8)


# ---- 3. components and degeneracy: two copies of the 221-vertex mesh and a vertex no cell names
def test_components_and_double_eigenvalues(ctx):
    v, c, L, mu, V = mesh("doubled")
    n = v.shape[0]
    lone = (n - 1) // 2
    assert np.sum(mu <= rs.CUTOFF) == 3 and abs(mu[3] - mu[4]) < 1e-12 and abs((mu[11] - mu[10]) / mu[10] - 0.195) < 0.01
    dm = build(ctx, "doubled", 8)
    info = dm.laplacianInfo
    assert info.converged and info.n_components == 3 and info.n_dropped == 3 and abs(info.cut_gap - 0.195) < 0.0195
    host = dm.to_host()
    want = want_model("doubled", 8)
    check_model_against_oracle(host, want, tol_lam=1e-8, tol_cov=1e-8)
    check_structure(host, 8)
    U = np.asarray(host.basis)
    assert not U[3 * lone:3 * lone + 3].any()                                        # the isolated vertex: exactly zero rows
    A = U * np.sqrt(host.variance)[None, :]
    rng = np.random.default_rng(1)
    ra, rb = rng.permutation(3 * lone)[:150], 3 * (lone + 1) + rng.permutation(3 * lone)[:150]
    top = np.abs(cov_of(want.U, want.lam, np.concatenate([ra, rb]))).max()
    assert np.abs(A[ra] @ A[rb].T).max() <= 1e-8 * top                                # nothing between the two copies
    # a cut inside a double eigenvalue: some orthonormal vectors of the eigenspace, the right variances, and the gap says so
    dm7 = build(ctx, "doubled", 7)
    assert dm7.laplacianInfo.converged and dm7.laplacianInfo.cut_gap < 1e-6
    h7 = dm7.to_host()
    lam7 = np.repeat(SCALING / mu[3:10], 3)
    assert np.linalg.norm(h7.variance - lam7) < 1e-8 * np.linalg.norm(lam7)
    U7 = np.asarray(h7.basis)
    assert np.abs(U7.T @ U7 - np.eye(21)).max() < 1e-9
    check_structure(h7, 7)


# ---- 4. smallest inputs: a tetrahedron, non-zero eigenvalues 4, 4, 4
def test_tetrahedron(ctx):
    import gingr_amd as ga
    v, c, L = mesh("tetra")[:3]
    dm = build(ctx, "tetra", 3)
    host = dm.to_host()
    assert dm.rank == 9 and dm.laplacianInfo.converged and dm.laplacianInfo.cut_gap == math.inf
    assert np.abs(np.asarray(host.variance) - SCALING / 4.0).max() < 1e-8 * SCALING / 4.0
    A = np.asarray(host.basis) * np.sqrt(host.variance)[None, :]
    C = A @ A.T
    P = SCALING * np.linalg.pinv(L)
    for d in range(3):
        for e in range(3):
            assert np.abs(C[d::3, e::3] - (P if d == e else 0.0)).max() < 1e-8 * np.abs(P).max()
    check_structure(host, 3)
    one = build(ctx, "tetra", 1)
    assert one.rank == 3 and np.abs(np.asarray(one.to_host().variance) - SCALING / 4.0).max() < 1e-8 * SCALING / 4.0
    with pytest.raises(ga.GingrNativeError) as e:
        build(ctx, "tetra", 4)
    assert e.value.code == 1 and "eigenvalues above the cut-off" in str(e.value)


def test_eigenvalues_below_the_cutoff_are_dropped(ctx):
    """a band of 2 x 1 200 vertices: mu_1 = 8.6e-6 lies below the cut-off and goes with the null vector; the model starts at mu_2.
    The gaps here are ~ 3e-5, so the residual bound says little about single vectors (residual / gap ~ 3e-5): checked are the
    variances (quadratic in the residual: 1e-8), orthonormality, and the contract itself, |L v - mu v| <= 1e-10 Lambda."""
    import gingr_amd as ga
    v, c = rs.strip(1200)
    L = rs.laplacian(v.shape[0], c)
    mu = np.linalg.eigvalsh(L)
    assert mu[1] <= rs.CUTOFF < mu[2]
    dm = ga.GPMMTriangleMesh3D(ctx, v, cells=c).InverseLaplacianSpectral(SCALING, 9)
    info = dm.laplacianInfo
    print("strip", info)
    gap = (mu[5] - mu[4]) / mu[4]
    assert info.converged and info.n_components == 1 and info.n_dropped == 2 and abs(info.cut_gap - gap) < 0.1 * gap
    host = dm.to_host()
    lam = np.repeat(SCALING / mu[2:5], 3)
    assert np.linalg.norm(host.variance - lam) < 1e-8 * np.linalg.norm(lam)
    check_structure(host, 3)
    V = np.asarray(host.basis)[0::3, 0::3]
    assert np.abs(V.T @ V - np.eye(3)).max() < 1e-9
    assert (np.linalg.norm(L @ V - V * (SCALING / np.asarray(host.variance)[0::3])[None, :], axis=0) / 8.0).max() <= 1.01e-10


# ---- 5. refusals with a text
def test_refusals(ctx):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    v, c = mesh("small")[:2]
    with pytest.raises(ValueError):
        ga.GPMMTriangleMesh3D(ctx, v).InverseLaplacianSpectral(SCALING, 24)          # no cells
    g = ga.GPMMTriangleMesh3D(ctx, v, cells=c)
    for rank in (25, 0, -3):
        with pytest.raises(ValueError):
            g.InverseLaplacianSpectral(SCALING, rank)
    lib = ctx._lib

    def call(k, cells, scaling=SCALING, max_degree=0, points=v):
        h, info = ctypes.c_void_p(), nat.LaplacianInfo()
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        rc = lib.gingr_model_from_laplacian(ctx.handle, points.shape[0], nat.dptr(nat.f64(points)), cells.shape[0], nat.iptr(cells), scaling, k, 0.0,
                                            max_degree, ctypes.byref(info), ctypes.byref(h))
        return rc, h.value, info, lib.gingr_last_error(ctx.handle).decode()

    bad_high, bad_neg = c.copy(), c.copy()
    bad_high[5, 1] = v.shape[0]
    bad_neg[7, 2] = -1
    for k, cells, word in ((0, c, "n_pairs"), (171, c, "n_pairs"), (8, bad_high, "cell 5"), (8, bad_neg, "cell 7"), (8, c[:0], "no cells")):
        rc, h, info, text = call(k, cells)
        assert rc == nat.ERR_BAD_ARGUMENT and not h and "model_from_laplacian" in text and word in text, (k, text)
    rc, h, info, text = call(8, c, scaling=0.0)
    assert rc == nat.ERR_BAD_ARGUMENT and not h and "scaling" in text
    with pytest.raises(ga.GingrNativeError):
        g.InverseLaplacianSpectral(SCALING, 513)                                     # k = 171
    # a budget of one block product on the femur: an error, no model, and info says why
    vf, cf = mesh("femur")[:2]
    rc, h, info, text = call(34, cf, max_degree=1, points=vf)
    assert rc == nat.ERR_NOT_CONVERGED and not h and info.converged == 0 and info.n_components == 1 and "budget" in text
    with pytest.raises(ga.GingrNativeError) as e:
        ga.GPMMTriangleMesh3D(ctx, vf, cells=cf).InverseLaplacianSpectral(SCALING, 102, maxDegree=1)
    assert e.value.code == nat.ERR_NOT_CONVERGED and not e.value.laplacianInfo.converged
    # a budget that ends in the middle of the iteration: still no model
    rc, h, info, text = call(34, cf, max_degree=40, points=vf)
    assert rc == nat.ERR_NOT_CONVERGED and not h and info.converged == 0 and 0 < info.total_degree <= 40 and info.max_residual > 1e-10


# ---- 6. determinism
def test_two_builds_give_the_same_bits(ctx):
    a, b = build(ctx, "femur", 34), build(ctx, "femur", 34)
    ha, hb = a.to_host(), b.to_host()
    assert np.array_equal(ha.variance, hb.variance) and np.array_equal(ha.basis, hb.basis)
    assert a.laplacianInfo == b.laplacianInfo


# ---- 7. the model is an ordinary model
def test_truncate_equals_the_smaller_build(ctx):
    big, small = build(ctx, "femur", 34), build(ctx, "femur", 10)
    t = big.truncate(30).to_host()
    s = small.to_host()
    check_model_against_oracle(t, rs.Model(30, np.asarray(s.variance), np.asarray(s.basis)), tol_lam=1e-8, tol_cov=1e-8)
    check_model_against_oracle(t, want_model("femur", 10), tol_lam=1e-8, tol_cov=1e-8)


def test_simple_interface_and_a_cpd_registration(ctx):
    import gingr_amd as ga
    from gingr_amd import simple as sp
    v, c = mesh("femur")[:2]
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    m = np.load(os.path.join(HERE, "golden", "femur_mesh.npz"))
    target = ga.TriangleMesh3D(d["femur_target"].astype(np.float64), m["femur_target_cells"].astype(np.int32))
    model = sp.SimpleTriangleModels3D.create(ctx, ga.TriangleMesh3D(v, c), sp.InvLapSpectralKernel(SCALING, 102))
    assert isinstance(model, ga.LaplacianDevicePointDistributionModel) and model.rank == 102 and model.cells is not None
    assert model.laplacianInfo.converged
    direct = build(ctx, "femur", 34).to_host()
    assert np.array_equal(model.to_host().variance, direct.variance) and np.array_equal(model.to_host().basis, direct.basis)
    # twenty CPD updates on the femur pair (run to the end, sigma2 collapses below 0.1 after ~27 updates and the reference's own
    # ModelFlexibilityError ends the run -- with this model as with any flexible one; that is not what this test is about)
    cpd = ga.CpdRegistration(ctx)
    st = cpd.createInitialState(model, target.points, ga.CpdConfiguration(maxIterations=40, w=0.1))
    for _ in range(20):
        st = cpd.update(st)
        assert st.general.status == ga.FittingStatuses.None_
    cpd.close()
    cmp_ = ga.RegistrationComparison(ctx, verbose=False)
    d0 = cmp_.avgDistance(ga.TriangleMesh3D(v, c), target)
    d1 = cmp_.avgDistance(ga.TriangleMesh3D(st.general.fit, c), target)
    print("average surface distance", d0, "->", d1)
    assert d1 < d0


def _free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def test_builds_release_their_device_memory(ctx):
    """the pattern of test_gpu_bcpd_no_leaks.py; at k = 170 every buffer of a build (block 2.5 MB, model basis 20 MB) kept 20 times
    would show against the 16 MiB the allocator's pools may move by"""
    def cycle():
        dm = build(ctx, "femur", 170)
        assert dm.rank == 510
        dm.device().close()

    cycle()
    gc.collect()
    before = _free_bytes()
    for _ in range(20):
        cycle()
    gc.collect()
    after = _free_bytes()
    assert before - after < 16 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
