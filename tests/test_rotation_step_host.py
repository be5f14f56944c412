"""Host side of the rotation-step tests (the device side is test_gpu_rotation_step.py):

1. every case of tests/rot3_cases.py takes the branch it is built for -- its guard holds against the oracle (go.umeyama, go.rot_to_euler,
   go.classic_cpd_maximization_rigid, pr.kabsch) --, the lattice slabs have the nearest neighbours they are designed to have, and the
   oracle's own spread (its change under perturbations of 2^-52 of its inputs) is measured per case and printed;
2. a dense sweep of gingr_amd/csrc/svd3.h compiled for the host (tests/c/rot3_driver.cpp): about 20 000 seeded matrices against numpy.
   Host arithmetic is not the device's; the sweep catches algorithmic slips at a density the device tests cannot afford."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import pca_restatement as pr
from tests import rot3_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize("name", sorted(rc.pairs()))
def test_pair_guards_hold_against_the_restatement(name):
    p = rc.pairs()[name]
    assert p.x.shape[0] <= 400
    S = p.S
    assert p.guard.holds(S=S), (name, np.linalg.svd(S, compute_uv=False), np.linalg.det(S))
    R, cx, ct = pr.kabsch(p.x, p.target)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    if p.guard.kind in ("det+", "det-"):    # (rank-deficient S: the sign of a rounding-level determinant decides, R may be improper --
        assert abs(np.linalg.det(R) - 1) < 1e-12   # the aligned points are the same either way, and only they are compared there)
    if p.guard.kind == "det-":          # the mirror branch of the restatement is the one that ran: U V^T alone would be improper
        U, _, Vt = np.linalg.svd(S)
        assert np.linalg.det(U @ Vt) < 0
    s = np.linalg.svd(S, compute_uv=False)
    if name.startswith("C-1e-2"):
        assert 0.2e-4 < s[2] / s[0] < 5e-4
    if name.startswith("C-1e-4"):
        assert 0.2e-8 < s[2] / s[0] < 5e-8
    if name.startswith("H-"):
        c = p.target.mean(0)
        assert np.linalg.norm(c) > 0.9e4 * np.ptp(p.target, axis=0).max()
    _, spread = rc.oracle_spread(lambda x, t: {"aligned": pr.align(x, t)}, (p.x, p.target))
    print(f"{name}: s3/s1 {s[2] / s[0]:.2e}, oracle spread of the aligned shape {spread['aligned'] / np.abs(p.x).max():.2e} of the largest coordinate")


def test_family_A_covers_the_quadrants_and_the_half_turns():
    rots = rc.rotations_A()
    quad = set()
    for name, R in rots.items():
        assert abs(np.linalg.det(R) - 1) < 1e-12
        phi, theta, psi = go.rot_to_euler(R)
        assert rc.Guard("euler", 0.3, 1.0).holds(R=R), name
        if name.startswith("phi-"):
            quad.add((phi > 0, abs(phi) > math.pi / 2, psi > 0, abs(psi) > math.pi / 2))
    assert len(quad) == 16
    for name in ("pi-x", "pi-y", "pi-z", "pi-random-axis"):
        assert abs(np.trace(rots[name]) + 1) < 1e-14 and np.abs(rots[name] - rots[name].T).max() < 1e-15   # angle pi exactly


@pytest.mark.parametrize("name", sorted(rc.slabs()))
def test_slab_guards_and_nearest_neighbours(name):
    s = rc.slabs()[name]
    assert s.tpl.shape[0] <= 400
    idx, _, _ = go.icp_closest_point(s.tpl, s.tgt)
    assert np.array_equal(idx, s.partner)                   # the design: every point's nearest neighbour is its partner
    S = rc.cross_covariance(s.tpl, s.tgt[idx])              # what go.umeyama decomposes in go.rigid_icp_iteration
    assert s.guard.holds(S=S), (name, np.linalg.svd(S, compute_uv=False), np.linalg.det(S))
    if s.scale == 1.0:                                      # (the classic CPD runs B, C, D, at variance 1 in the slab's own units)
        A = rc.classic_cpd_A(s)
        assert s.guard.holds(S=A), (name, np.linalg.svd(A, compute_uv=False), np.linalg.det(A))
        if s.guard.kind == "det-":
            u, _, vt = np.linalg.svd(A)
            assert np.linalg.det(u @ vt.T) < 0              # the classic CPD's own convention takes its mirror branch too
    if s.guard.kind == "det-":
        for sim in (False, True):
            R, t, c = go.umeyama(s.tpl, s.tgt[idx], sim)
            assert abs(np.linalg.det(R) - 1) < 1e-12
        d = np.linalg.svd(S, compute_uv=False)
        assert abs(c - (d[0] + d[1] - d[2]) / (((s.tpl - s.tpl.mean(0)) ** 2).sum() / s.tpl.shape[0])) < 1e-12   # d1 + d2 - d3
        assert d[1] > 10 * d[2]                             # d2 > d3 well separated
    if s.guard.kind != "rank2":
        def icp(tpl, tgt):
            pts, dist, (sc, R, t) = go.rigid_icp_iteration(tpl, tgt, True)
            return {"points": pts, "R": R, "scale": sc, "t": t}
        _, spread = rc.oracle_spread(icp, (s.tpl, s.tgt))
        print(f"{name}: rigid ICP oracle spread " + ", ".join(f"{k} {v:.2e}" for k, v in spread.items()))
    if s.scale != 1.0:
        return
    _, spread = rc.oracle_spread(rc.classic_cpd_outputs, (s.tgt, s.tpl))
    print(f"{name}: classic CPD oracle spread " + ", ".join(f"{k} {v:.2e}" for k, v in spread.items()))


@pytest.mark.parametrize("flavour", ["cpd", "icp"])
def test_update_guards(flavour):
    """the Umeyama step of the oracle's update sees the state's total rotation (families A, F) resp. a mirrored slab (family B)"""
    model = rc.stiff_model()
    cases = {k: (R, rc.Guard("euler", 0.3, 1.0)) for k, R in rc.rotations_A().items()}
    cases.update({k: (R, g) for k, (R, g, _) in rc.rotations_F().items()})
    for name, (R0, guard) in cases.items():
        target = rc.posed_target(model, R0, rc.T0)
        st = rc.state_at(model, 1.0, R0, rc.T0, go.RIGID_TRANSFORMS, direct=name in rc.rotations_F())
        S = rc.update_sigma_xy(model, target, st, flavour)
        assert rc.Guard("det+").holds(S=S), name
        R = rc.svd_rotation(S)
        assert guard.holds(R=R), (name, R[2, 0])
        assert np.abs(R - st.rotation()).max() < 1e-3, name          # the step returns the state's total rotation
    mm, target = rc.mirror_model()
    st = go.initial_state(mm, 1.0)
    S = rc.update_sigma_xy(mm, target, st, flavour)
    d = np.linalg.svd(S, compute_uv=False)
    assert rc.Guard("det-").holds(S=S) and d[1] > 10 * d[2], (d, np.linalg.det(S))


def test_gimbal_guards_stay_clear_of_the_window_edge():
    for name, (R, g, _) in rc.rotations_F().items():
        assert abs(abs(abs(R[2, 0]) - 1) - rc.LOCK_WINDOW) > 4e-5, name      # 1e-3 in delta about the edge 0.01414 is 1.4e-5 here ...
        delta = math.pi / 2 - abs(math.asin(-R[2, 0])) if abs(R[2, 0]) < 1 else 0.0
        assert abs(delta - math.sqrt(2 * rc.LOCK_WINDOW)) >= 1e-3, name      # ... and this is the margin in delta itself


# ------------------------------------------------------------------------------------------------------ dense sweep of svd3.h
def _orth(rng, n):
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return Q


def sweep_matrices():
    rng = np.random.default_rng(2024)
    out = [rng.normal(size=(4000, 3, 3))]
    # graded to condition 1e12, both determinant signs (the sign is that of det U det V: random)
    e = np.sort(rng.uniform(0.0, 12.0, (6000, 2)), axis=1)
    sv = np.concatenate([np.ones((6000, 1)), 10.0 ** -e], axis=1)
    sv[:500, 2] = 1e-12
    U, V = _orth(rng, 6000), _orth(rng, 6000)
    out.append(np.einsum("nij,nj,nkj->nik", U, sv, V))
    # rank 2: to rounding (a product of factors) and exactly (sums of two integer outer products)
    U, V = _orth(rng, 1500), _orth(rng, 1500)
    out.append(np.einsum("nij,nj,nkj->nik", U, np.concatenate([rng.uniform(0.1, 2.0, (1500, 2)), np.zeros((1500, 1))], axis=1), V))
    a, b, c, d = (rng.integers(-9, 10, (1500, 3)).astype(np.float64) for _ in range(4))
    out.append(np.einsum("ni,nj->nij", a, b) + np.einsum("ni,nj->nij", c, d))
    # rank 1: exactly and to rounding; zero
    out.append(np.einsum("ni,nj->nij", a[:1000], b[:1000]))
    out.append(np.einsum("ni,nj->nij", *rng.normal(size=(2, 1000, 3))))
    out.append(np.zeros((1, 3, 3)))
    # repeated singular values: (1,1,1), (2,2,1), (2,1,1), both signs
    U, V = _orth(rng, 3000), _orth(rng, 3000)
    rep = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 1.0], [2.0, 1.0, 1.0]])[rng.integers(0, 3, 3000)]
    out.append(np.einsum("nij,nj,nkj->nik", U, rep, V))
    out.append(np.stack([np.eye(3), -np.eye(3), np.diag([1.0, 1.0, -1.0]), np.diag([3.0, 0.0, 0.0]), np.diag([0.0, 0.0, 3.0])]))
    base = np.concatenate(out)
    pick = rng.permutation(base.shape[0])[:1000]
    return np.concatenate([base, base[pick] * 1e-150, base[pick] * 1e100])


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rot3") / "rot3_driver"
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "rot3_driver.cpp"), "-o", str(exe)])
    A = sweep_matrices()
    raw = subprocess.run([str(exe)], input=np.ascontiguousarray(A).tobytes(), capture_output=True, check=True).stdout
    res = np.frombuffer(raw, dtype=np.float64).reshape(A.shape[0], 42)
    return A, res


def _worst(name, v, A):
    k = int(np.argmax(v))
    return f"{name}: worst {v[k]:.3e} at matrix {k}\n{A[k]}"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no HIP compiler")
def test_svd3_against_numpy(sweep):
    A, res = sweep
    n = A.shape[0]
    assert n >= 19000 and np.isfinite(res).all()
    U, s, V = res[:, :9].reshape(n, 3, 3), res[:, 9:12], res[:, 12:21].reshape(n, 3, 3)
    ref = np.linalg.svd(A, compute_uv=False)
    s1 = ref[:, 0]
    fro = np.linalg.norm(A.reshape(n, 9), axis=1)
    eye = np.eye(3)[None]
    dU = np.abs(np.einsum("nji,njk->nik", U, U) - eye).reshape(n, 9).max(1)
    dV = np.abs(np.einsum("nji,njk->nik", V, V) - eye).reshape(n, 9).max(1)
    assert dU.max() <= 1e-14, _worst("U^T U - I", dU, A)
    assert dV.max() <= 1e-14, _worst("V^T V - I", dV, A)
    rec = np.abs(np.einsum("nij,nj,nkj->nik", U, s, V) - A).reshape(n, 9).max(1)
    assert (rec <= 1e-14 * fro).all(), _worst("U s V^T - A over |A|", rec / np.maximum(fro, 1e-300), A)
    ds = np.abs(s - ref).max(1)
    assert (ds <= 1e-14 * s1).all(), _worst("s - numpy over s1", ds / np.maximum(s1, 1e-300), A)
    assert (np.diff(s, axis=1) <= 0).all() and (s >= 0).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no HIP compiler")
def test_polar_factor_and_kabsch_against_numpy(sweep):
    """The polar factor where polar3_rotation accepts the matrix, against U V^T of numpy's SVD.  Bound: both are the exact polar factor
    of a matrix within c eps |A| of A (numpy's SVD, and the scaled Newton iteration, are backward stable; the iteration stops at a
    change below 4e-16), and the polar factor of a real 3 x 3 matrix moves by at most 2 |dA|_F / (s2 + s3) (Mathias; Higham, Functions
    of Matrices, theorem 8.9).  With c = 32 for each route: 64 eps 2 s1 / (s2 + s3), plus the 1e-14 the factors themselves are held to.
    Kabsch: a proper rotation whose trace(R^T S) is the optimum d1 + d2 + sign(det S) d3.  R itself may be off by the bound above, but the
    trace is stationary there (second order), so it is held to the 1e-14 s1 of the singular values; where d3 is within rounding of zero
    (<= 1e-13 s1) either sign is an optimum to that level and 2 d3 is allowed for."""
    A, res = sweep
    n = A.shape[0]
    ok = res[:, 21] == 1.0
    Rp, trp = res[:, 22:31].reshape(n, 3, 3), res[:, 31]
    Rk, trk = res[:, 32:41].reshape(n, 3, 3), res[:, 41]
    U, d, Vt = np.linalg.svd(A)
    det = np.linalg.slogdet(A)[0]                        # the sign alone: the determinant itself leaves the range at 1e-150 and 1e+100
    # accepted only with a positive determinant; accepted for every well-conditioned matrix with one
    assert not (ok & (det < 0) & (d[:, 2] > 1e-10 * d[:, 0])).any()
    well = (det > 0) & (d[:, 2] > 1e-3 * d[:, 0]) & (d[:, 0] < 1e50) & (d[:, 0] > 1e-50)
    assert ok[well].all()
    # (the nearest PROPER rotation U diag(1, 1, det(U V^T)) V^T: the same matrix wherever the determinant is more than rounding; where
    # it is not, the polar iteration saw a positive one and numpy's factors may belong to a neighbour with a negative one)
    UVt = np.einsum("nij,njk->nik", U, Vt)
    flip = np.where(np.linalg.det(UVt) < 0, -1.0, 1.0)
    UVt = UVt + np.einsum("n,ni,nj->nij", flip - 1.0, U[:, :, 2], Vt[:, 2, :])
    eps = 2.0 ** -52
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 64 * eps * 2 * d[:, 0] / (d[:, 1] + d[:, 2]) + 1e-14
    dev = np.abs(Rp - UVt).reshape(n, 9).max(1)
    bad = ok & ~(dev <= tol)
    assert not bad.any(), _worst("polar - U V^T over its bound", np.where(ok, dev / tol, 0.0), A)
    dtr = np.abs(trp - d.sum(1))
    assert (dtr[ok] <= 1e-14 * d[ok, 0]).all(), _worst("polar trace", np.where(ok, dtr / np.maximum(d[:, 0], 1e-300), 0.0), A)
    print(f"polar accepted {ok.sum()} of {n}; worst deviation / bound {np.where(ok, dev / tol, 0.0).max():.3f}")
    # Kabsch
    eye = np.eye(3)[None]
    orth = np.abs(np.einsum("nji,njk->nik", Rk, Rk) - eye).reshape(n, 9).max(1)
    assert orth.max() <= 1e-14 * 4, _worst("kabsch R^T R - I", orth, A)
    dk = np.linalg.det(Rk)
    assert (np.abs(dk - 1) <= 1e-13).all(), _worst("det R - 1", np.abs(dk - 1), A)
    sgn = np.where(det < 0, -1.0, 1.0)
    opt = d[:, 0] + d[:, 1] + sgn * d[:, 2]
    slack = 1e-14 * d[:, 0] + np.where(d[:, 2] <= 1e-13 * d[:, 0], 2 * d[:, 2], 0.0)
    got = np.einsum("nij,nij->n", Rk, A)
    assert (np.abs(got - opt) <= slack).all(), _worst("trace(R^T S) - optimum over s1", np.abs(got - opt) / np.maximum(d[:, 0], 1e-300), A)
    assert (np.abs(trk - opt) <= slack).all(), _worst("returned trace - optimum over s1", np.abs(trk - opt) / np.maximum(d[:, 0], 1e-300), A)
