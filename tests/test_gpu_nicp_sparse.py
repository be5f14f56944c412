"""The sparse least-squares step of the optimal-step non-rigid ICP baselines on the device (gingr_nicp_create / _step:
gingr_amd/csrc/nicp_sparse.hip, matrix-free block-Jacobi preconditioned CG over the template's edge graph) against the oracle's dense
stacked least squares, against the dense device path where the reductions span workgroups, and against a host assembly with
scipy.sparse at a size the dense path cannot reach; determinism and the failure statuses of the C ABI."""
import ctypes

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests.test_gpu_nicp import oracle_landmarks, pair, sphere_mesh

pytestmark = pytest.mark.gpu

GAMMA = 0.7


@pytest.mark.parametrize("kind", ["T", "A"])
def test_sparse_iterations_match_the_oracle(ctx, kind):
    """220 vertices: every reduction fits one workgroup.  Measured on the device, |sparse - oracle|max at alpha = 10 / 4 / 1
    (CG iterations): T 2.7e-13 / 5.9e-13 / 1.7e-12 (70 / 65 / 39), A 7.0e-10 / 2.9e-10 / 2.5e-9 (91 / 89 / 74); true relative residual
    between 5.6e-13 and 9.9e-13."""
    from gingr_amd import classic
    (tv, tt), (gv, gt), lm_t, lm_g = pair()
    task = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, gamma=GAMMA, kind=kind, solver="sparse")
    ids, ul = oracle_landmarks(tv, gv, lm_t, lm_g)
    assert np.array_equal(task.lmIdsOnTemplate, ids) and np.array_equal(task.UL, ul)
    edges = go.nicp_edges(tt)
    assert np.array_equal(task.edges, edges)
    fit = tv
    for it, (alpha, beta) in enumerate([(10.0, 10.0), (4.0, 2.0), (1.0, 0.5)]):
        got, dist, lm = task.Iteration(fit, alpha, beta)
        info = task.solveInfo
        if kind == "T":
            want, wdist = go.nicp_iteration_t(fit, tt, gv, gt, edges, ids, ul, alpha, beta)
            wlm = want[ids]
        else:
            want, wdist, wlm = go.nicp_iteration_a(fit, tt, gv, gt, edges, ids, ul, alpha, beta, GAMMA)
        err = np.abs(got - want).max()
        rel = (info["residual"] / info["rhs_norm"]).max()
        print(f"n=220 kind={kind} alpha={alpha}: |sparse - oracle|max {err:.3e}, CG iterations {info['iterations']}, true residual {rel:.3e}")
        assert err < 1e-7, (kind, it, err)                 # normal equations against lstsq on the stacked system
        assert np.abs(lm - wlm).max() < 1e-7
        assert abs(dist - wdist) < 1e-12 * wdist
        assert info["converged"] and rel <= 1e-12
        fit = want
    task.close()


@pytest.mark.parametrize("kind", ["T", "A"])
@pytest.mark.parametrize("n", [1000, 3000])
def test_sparse_matches_dense_across_workgroups(ctx, n, kind):
    """n = 1 000 = 3 x 256 + 232 (a ragged last workgroup) and 3 000: the reductions span workgroups.  One Iteration from the same fit
    by both solvers.  Measured on the device, |sparse - dense|max at alpha = 10 / 1 (CG iterations):
    n = 1 000: T 4.7e-13 / 2.3e-12 (138 / 43), A 4.7e-10 / 6.6e-9 (179 / 163);
    n = 3 000: T 7.8e-13 / 1.5e-12 (209 / 43), A 3.2e-10 / 3.7e-9 (288 / 254)."""
    from gingr_amd import classic
    (tv, tt), (gv, gt), lm_t, lm_g = pair(seed=10, n=n)
    dense = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, gamma=GAMMA, kind=kind)
    sparse = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, gamma=GAMMA, kind=kind, solver="sparse")
    for alpha in (10.0, 1.0):
        want, wdist, wlm = dense.Iteration(tv, alpha, alpha)
        got, dist, lm = sparse.Iteration(tv, alpha, alpha)
        info = sparse.solveInfo
        err = np.abs(got - want).max()
        print(f"n={n} kind={kind} alpha={alpha}: |sparse - dense|max {err:.3e}, CG iterations {info['iterations']}, "
              f"true residual {(info['residual'] / info['rhs_norm']).max():.3e}")
        assert dist == wdist and info["converged"]
        assert err < 1e-7, (n, kind, alpha, err)
        assert np.abs(lm - wlm).max() < 1e-7
    dense.close()
    sparse.close()


def step(ctx, handle, n, moving, w, cp, ul, alpha, beta, gamma=1.0, rel_tol=0.0, max_iterations=0, n_lm=0):
    from gingr_amd import _native as nat
    out, lm, info = np.empty((n, 3)), np.empty((max(n_lm, 1), 3)), nat.NicpInfo()
    rc = ctx._lib.gingr_nicp_step(handle, nat.dptr(nat.f64(moving)), nat.dptr(nat.f64(w)), nat.dptr(nat.f64(cp)),
                                  nat.dptr(nat.f64(ul)) if n_lm else None, alpha, beta, gamma, rel_tol, max_iterations, nat.dptr(out),
                                  nat.dptr(lm) if n_lm else None, ctypes.byref(info))
    return rc, out, lm[:n_lm], info


def create(ctx, kind, n, edges, lm_ids=()):
    from gingr_amd import _native as nat
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    ids = np.ascontiguousarray(lm_ids, dtype=np.int32)
    h = ctypes.c_void_p()
    rc = ctx._lib.gingr_nicp_create(ctx.handle, kind, n, edges.shape[0], nat.iptr(edges) if edges.size else None, ids.shape[0],
                                    nat.iptr(ids) if ids.size else None, ctypes.byref(h))
    return rc, h


def test_two_steps_give_the_same_bits(ctx):
    from gingr_amd import classic
    (tv, tt), (gv, gt), lm_t, lm_g = pair(seed=10, n=1000)
    task = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, gamma=GAMMA, kind="A", solver="sparse")
    cp, w, _ = task.getClosestPoints(tv)
    L = task.lmIdsOnTemplate.shape[0]
    runs = [step(ctx, task._nicp, 1000, tv, w, cp, task.UL, 10.0, 10.0, GAMMA, n_lm=L) for _ in range(2)]
    (rc0, out0, lm0, info0), (rc1, out1, lm1, info1) = runs
    assert rc0 == 0 and rc1 == 0 and L == 3
    assert np.array_equal(out0, out1) and np.array_equal(lm0, lm1)
    assert info0.iterations == info1.iterations > 0 and info0.residual[:] == info1.residual[:] and info0.rhs_norm[:] == info1.rhs_norm[:]
    moved = np.einsum("ie,iec->ic", np.c_[tv, np.ones(1000)], task.solution().reshape(1000, 4, 3))      # D X of the unknowns
    assert np.abs(moved - out0).max() < 1e-9
    task.close()


def test_failures_are_reported_and_cleared(ctx):
    from gingr_amd import _native as nat
    from gingr_amd.classic import nicp_edges
    lib = ctx._lib
    tv, tt = sphere_mesh(80, 2)
    edges = nicp_edges(tt)
    target = tv * 1.03 + 0.2
    # a hull plus an isolated vertex without weight: its row of the normal equations is zero
    tv2 = np.concatenate([tv, [[100.0, 0.0, 0.0]]])
    for kind in (0, 1):
        rc, h = create(ctx, kind, 81, edges)
        assert rc == 0
        w = np.ones(81)
        w[-1] = 0.0
        rc, _, _, _ = step(ctx, h, 81, tv2, w, tv2 * 1.03, None, 10.0, 1.0)
        assert rc == nat.ERR_NOT_SPD and b"positive definite" in lib.gingr_last_error(ctx.handle)
        if kind == 0:        # the same handle, now anchored
            rc, out, _, info = step(ctx, h, 81, tv2, np.ones(81), tv2 * 1.03, None, 10.0, 1.0)
        else:                # (an isolated vertex's 4 x 4 block has rank one whatever its weight: a fresh handle over the hull alone)
            lib.gingr_nicp_destroy(h)
            rc, h = create(ctx, kind, 80, edges)
            assert rc == 0
            rc, out, _, info = step(ctx, h, 80, tv, np.ones(80), target, None, 10.0, 1.0)
        assert rc == 0 and info.converged == 1 and np.isfinite(out).all()
        lib.gingr_nicp_destroy(h)
    # two disjoint hulls, one of them without any weight and no landmark
    v2, e2 = np.concatenate([tv, tv + 100.0]), np.concatenate([edges, edges + 80])
    rc, h = create(ctx, 1, 160, e2)
    assert rc == 0
    rc, _, _, _ = step(ctx, h, 160, v2, np.concatenate([np.ones(80), np.zeros(80)]), v2 * 1.03, None, 10.0, 1.0)
    assert rc == nat.ERR_NOT_SPD and b"positive definite" in lib.gingr_last_error(ctx.handle)
    rc, out, _, info = step(ctx, h, 160, v2, np.ones(160), v2 * 1.03, None, 10.0, 1.0)
    assert rc == 0 and info.converged == 1
    lib.gingr_nicp_destroy(h)
    # the iteration cap
    rc, h = create(ctx, 0, 80, edges)
    assert rc == 0
    rc, out, _, info = step(ctx, h, 80, tv, np.ones(80), target, None, 10.0, 1.0, max_iterations=3)
    assert rc == nat.ERR_NOT_CONVERGED == 7 and info.iterations == 3 and info.converged == 0
    assert np.isfinite(info.residual[:]).all() and max(info.residual[:]) > 0.0 and np.isfinite(out).all()
    assert b"iterations" in lib.gingr_last_error(ctx.handle)
    with pytest.raises(nat.GingrNativeError, match="GINGR_ERR_NOT_CONVERGED"):
        from gingr_amd.api import _check
        _check(ctx.handle, rc, "gingr_nicp_step")
    rc, out, _, info = step(ctx, h, 80, tv, np.ones(80), target, None, 10.0, 1.0)
    assert rc == 0 and info.converged == 1 and info.iterations > 3
    lib.gingr_nicp_destroy(h)
    # what create refuses; a fresh handle works afterwards
    rc, h = create(ctx, 0, 80, np.concatenate([edges, edges[5:6]]))
    assert rc == nat.ERR_BAD_ARGUMENT and not h.value and b"repeats" in lib.gingr_last_error(ctx.handle)
    rc, h = create(ctx, 0, 80, [[5, 3]])
    assert rc == nat.ERR_BAD_ARGUMENT and not h.value and b"edge" in lib.gingr_last_error(ctx.handle)
    rc, h = create(ctx, 0, 80, [[5, 80]])
    assert rc == nat.ERR_BAD_ARGUMENT and not h.value
    rc, h = create(ctx, 0, 80, edges)
    assert rc == 0
    rc, out, _, info = step(ctx, h, 80, tv, np.ones(80), target, None, 10.0, 1.0)
    assert rc == 0 and info.converged == 1
    assert lib.gingr_nicp_get_solution(h, nat.dptr(np.empty((80, 3)))) == 0
    lib.gingr_nicp_destroy(h)


def test_a_size_the_dense_path_cannot_reach(ctx, monkeypatch):
    """N-ICP-A at 20 000 vertices: 80 000 unknowns, a dense matrix of 51 GB.  Checked against the normal equations assembled with
    scipy.sparse on the host from the returned correspondence; the dense entry point is never called.  Measured on the device:
    661 CG iterations, true relative residual 9.95e-13 (the host assembly finds the same 9.95e-13), |moved - splu|max 2.0e-10."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    from gingr_amd import classic
    n, alpha, beta = 20000, 10.0, 10.0
    (tv, tt), (gv, gt), lm_t, lm_g = pair(seed=20, n=n)
    task = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, gamma=GAMMA, kind="A", solver="sparse")

    def no_dense(*a, **k):
        raise AssertionError("the dense entry point was called")
    monkeypatch.setattr(ctx._lib, "gingr_nicp_solve", no_dense)
    got, dist, lm = task.Iteration(tv, alpha, beta)
    info, X = task.solveInfo, task.solution()
    cp, w, _ = task.getClosestPoints(tv)
    # the normal equations of NonRigidOptimalStepICP_A.Iteration, assembled independently
    ids, ul = task.lmIdsOnTemplate.astype(np.int64), task.UL
    w = w.copy()
    w[ids] = 0.0
    E = task.edges.shape[0]
    M = sp.csr_matrix((np.r_[np.ones(E), -np.ones(E)], (np.r_[np.arange(E), np.arange(E)], np.r_[task.edges[:, 0], task.edges[:, 1]])),
                      shape=(E, n))
    q = np.c_[tv, np.ones(n)]
    D = sp.csr_matrix((q.ravel(), (np.repeat(np.arange(n), 4), np.arange(4 * n))), shape=(n, 4 * n))
    DL = D[ids]
    W2 = sp.diags(w * w)
    A = (alpha * alpha * sp.kron(M.T @ M, sp.diags([1.0, 1.0, 1.0, GAMMA * GAMMA])) + D.T @ W2 @ D + beta * beta * (DL.T @ DL)).tocsc()
    B = D.T @ (W2 @ cp) + beta * beta * (DL.T @ ul)
    rel = np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)
    want = D @ splu(A).solve(B)
    err = np.abs(got - want).max()
    print(f"n={n} kind=A alpha={alpha}: CG iterations {info['iterations']}, true residual device {(info['residual'] / info['rhs_norm']).max():.3e} "
          f"host {rel.max():.3e}, |moved - splu|max {err:.3e}")
    assert info["converged"] and np.abs(D @ X - got).max() < 1e-9
    assert rel.max() <= 1e-11              # one decade over the stop for the rounding of an independent assembly
    assert err < 1e-7 and np.abs(lm - want[ids]).max() < 1e-7
    task.close()


def test_registration_loop_equals_its_iterations(ctx):
    from gingr_amd import classic
    (tv, tt), (gv, gt), lm_t, lm_g = pair(seed=4, n=150)
    task = classic.NonRigidOptimalStepICP_T(ctx, (tv, tt), (gv, gt), lm_t, lm_g, solver="sparse")
    got = task.Registration(2, tolerance=0.001, alpha=[10.0, 2.0], beta=[10.0, 1.0])
    assert task.iterations == 4
    fit = tv
    for a, b in [(10.0, 10.0), (10.0, 10.0), (2.0, 1.0), (2.0, 1.0)]:
        fit = task.Iteration(fit, a, b)[0]
    assert np.array_equal(got, fit)
    # a template that already lies on the target: b = 0 in every column, nothing to iterate on, and the stage stops at once
    same = classic.NonRigidOptimalStepICP_T(ctx, (gv, gt), (gv, gt), solver="sparse", relTol=1e-13, maxSolverIterations=500)
    out = same.Registration(5, tolerance=0.001, alpha=[10.0], beta=[10.0])
    assert same.iterations == 1 and np.abs(out - gv).max() < 1e-9 and same.solveInfo["converged"]
    same.close()
    with pytest.raises(ValueError):
        classic.NonRigidOptimalStepICP_T(ctx, (tv, tt), (gv, gt), solver="auto")
    task.close()
