"""The compact passes of a coordinate-separable model (GINGR_OPT_SEPARABLE): detection at finalize, the weighted
Gram blocks scattered into the dense G / rhs, the three-workgroup posterior solve and the fit pass over the compact basis -- against
numpy, against the oracle and against the dense passes (option 0).

Tolerances.  G / rhs: the tightest bound of tests/test_gpu_parity.py::test_weighted_gram_every_tile_count (1e-8 relative; the sums
here are a few thousand float64 products, ~1e-13).  Updates: the rule of tests/test_gpu_bench_workload_parity.py::_check_one_update
(fit 1e-5, sigma2 1e-8, alpha 1e-4).  Wherever the dense path must have run the comparison with option 0 is bit for bit."""
import ctypes
from ctypes import c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests.test_gpu_bench_workload_parity import _check_one_update, rel

pytestmark = pytest.mark.gpu

W = 0.1


# ------------------------------------------------------------------------------------------------------------------ helpers
def _points(M, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 40, (M, 3))


def _target(mo, seed, n=None):
    rng = np.random.default_rng(seed)
    t = mo.instance(rng.normal(0, 0.7, mo.rank)) + rng.normal(0, 0.5, (mo.M, 3))
    return t[rng.permutation(mo.M)[: n or mo.M]]


def _gaussian(ctx, M, r, seed=1):
    import gingr_amd as ga
    model = ga.GPMMTriangleMesh3D(ctx, _points(M, seed), relativeTolerance=0.0, maxRank=r).Gaussian(60.0, 30.0)
    host = model.to_host()
    mo = go.PDM(host.reference, host.mean, np.ascontiguousarray(host.basis), host.variance)
    assert mo.rank == r
    return model, mo


def _separable_basis(M, counts, seed):
    """An orthonormal basis whose column k lives on one coordinate: counts[d] columns on coordinate d, the classes interleaved."""
    rng = np.random.default_rng(seed)
    cols = []
    for d, n in enumerate(counts):
        if n:
            q, _ = np.linalg.qr(rng.normal(0, 1, (M, n)))
            for k in range(n):
                u = np.zeros(3 * M)
                u[d::3] = q[:, k]
                cols.append((k, d, u))
    cols.sort(key=lambda c: (c[0], c[1]))
    U = np.stack([c[2] for c in cols], axis=1)
    lam = np.sort(rng.uniform(20.0, 400.0, U.shape[1]))[::-1].copy()
    return U, lam


def _uploaded(M, U, lam, seed):
    import gingr_amd as ga
    rng = np.random.default_rng(seed)
    mo = go.PDM(ref=_points(M, seed), mean=rng.normal(0, 0.1, (M, 3)), U=np.ascontiguousarray(U), lam=lam)
    return ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam), mo


def _flags(f):
    sep, compact, cnt = c_int32(), c_int32(), (c_int32 * 3)()
    assert f._lib.gingr_model_separable(f.dev_model.handle, ctypes.byref(sep), cnt, ctypes.byref(compact)) == 0
    return bool(sep.value), tuple(cnt), bool(compact.value)


class _Option:
    """GINGR_OPT_SEPARABLE of the shared context for the length of a block"""

    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        from gingr_amd import _native as nat
        self.opt = nat.OPT_SEPARABLE
        self.before = self.ctx.get_option(self.opt)
        self.ctx.set_option(self.opt, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.opt, self.before)


def _fitter(ctx, model, x, mo, **kw):
    from gingr_amd.sharded import ShardedFitter
    f = ShardedFitter(ctx, model, x, **kw)
    f.set_state(np.zeros(mo.rank), ctx.cpd_initial_sigma2(mo.ref + mo.mean, x))
    return f


def _state_of(f):
    a, sc, fit = f.get_state()
    return a.copy(), float(sc.sigma2), fit.copy(), int(sc.status), int(sc.iteration)


def _same_bits(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)


def _column_classes(mo):
    cls = []
    for k in range(mo.rank):
        nz = [d for d in range(3) if np.any(mo.U[d::3, k] != 0.0)]
        assert len(nz) <= 1
        cls.append(nz[0] if nz else 0)
    return np.array(cls)


def _phase1_system(ctx, f, mo):
    """dense G [rp][rp] and rhs [rp] of exchange segment 1 after phases 0 and 1 of one CPD update, with P1 / PX of phase 0"""
    from gingr_amd import _native as nat
    from gingr_amd.sharded import as_torch
    p = nat.CpdParams(W, 1.0)
    for ph in range(2):
        assert f._lib.gingr_fitter_cpd_phase_async(f.handle, ctypes.byref(p), ph) == 0
    ctx.synchronize()
    ptr, offs, cnts = c_void_p(), (c_int64 * 2)(), (c_int64 * 2)()
    assert f._lib.gingr_fitter_exchange(f.handle, ctypes.byref(ptr), offs, cnts) == 0
    seg = as_torch(ptr.value, offs[1] + cnts[1], ctx.device)[offs[1]:].cpu().numpy()
    rp = (mo.rank + 15) // 16 * 16
    return seg[: rp * rp].reshape(rp, rp).copy(), seg[rp * rp: rp * rp + rp].copy(), f.get_cpd_stats()


# ------------------------------------------------------------------------------------------------------------ basic behaviour
@pytest.mark.parametrize("M", [257, 1000])
@pytest.mark.parametrize("r", [3, 7, 48, 100, 112])
def test_gaussian_model_gram_and_updates(ctx, M, r):
    """Flag set; dense G / rhs of one phase 1 against numpy sum_i w_i Q_i^T Q_i with exact zeros between the classes; five updates on
    either path against the oracle.  Prints the largest difference between the two paths (a record, not a gate)."""
    model, mo = _gaussian(ctx, M, r)
    x = _target(mo, 7 + r, n=(3 * M) // 4)
    f = _fitter(ctx, model, x, mo)
    sep, counts, compact = _flags(f)
    assert sep and compact and sum(counts) == r and max(counts) <= 48
    s2 = f.get_state()[1].sigma2
    G, rhs, stats = _phase1_system(ctx, f, mo)
    f.close()
    Q = mo.U * np.sqrt(mo.lam)[None, :]
    w = stats["P1"] / (s2 * 1.0)
    e = w[:, None] * (stats["PX"] / stats["P1"][:, None] - mo.ref - mo.mean)
    G_ref = (Q * np.repeat(w, 3)[:, None]).T @ Q
    rhs_ref = Q.T @ e.reshape(-1)
    e_G, e_rhs = rel(G[:r, :r], G_ref), rel(rhs[:r], rhs_ref)
    print(f"M={M} r={r}: rel G {e_G:.2e}, rel rhs {e_rhs:.2e}")
    assert e_G < 1e-8 and e_rhs < 1e-8
    cls = _column_classes(mo)
    cross = cls[:, None] != cls[None, :]
    assert np.all(G[:r, :r][cross] == 0.0) and not np.any(np.signbit(G[:r, :r][cross]))
    assert np.all(G[r:, :] == 0.0) and np.all(G[:, r:] == 0.0) and np.all(rhs[r:] == 0.0)
    ends = {}
    for opt in (-1, 0):
        with _Option(ctx, opt):
            f = _fitter(ctx, model, x, mo)
            for k in range(5):
                _check_one_update(f, mo, x, W, f"M={M} r={r} option {opt} step {k}")
            ends[opt] = _state_of(f)
            f.close()
    d_a, d_fit = rel(ends[-1][0], ends[0][0]), rel(ends[-1][2], ends[0][2])
    d_s2 = abs(ends[-1][1] - ends[0][1]) / ends[0][1]
    print(f"M={M} r={r}: compact against dense after 5 updates: alpha {d_a:.2e}, fit {d_fit:.2e}, sigma2 {d_s2:.2e}")


# -------------------------------------------------------------------------------------------------------- uneven classes
def _five_updates(ctx, model, x, mo, opt, **kw):
    with _Option(ctx, opt):
        f = _fitter(ctx, model, x, mo, **kw)
        flags = _flags(f)
        f.update_cpd(W, 1.0, 5)
        out = _state_of(f)
        f.close()
    return flags, out


def test_uploaded_basis_with_an_empty_class_runs_compact(ctx):
    """Class counts (48, 1, 0): the compact path runs; the coordinate without columns is reference + mean (no global transform)."""
    M = 300
    U, lam = _separable_basis(M, (48, 1, 0), seed=3)
    model, mo = _uploaded(M, U, lam, seed=4)
    x = _target(mo, 5)
    flags, got = _five_updates(ctx, model, x, mo, -1, global_transform=0)
    assert flags == (True, (48, 1, 0), True)
    _, want = _five_updates(ctx, model, x, mo, 0, global_transform=0)
    assert got[3] == want[3] == 0 and got[4] == want[4] == 5
    assert rel(got[0], want[0]) < 1e-9 and rel(got[2], want[2]) < 1e-11 and abs(got[1] - want[1]) < 1e-9 * want[1]
    assert np.allclose(got[2][:, 2], (mo.ref + mo.mean)[:, 2], rtol=0.0, atol=1e-12)
    st = go.initial_state(mo, ctx.cpd_initial_sigma2(mo.ref + mo.mean, x), global_transformation=go.NO_TRANSFORMS)
    for _ in range(5):
        st = go.cpd_update(mo, x, st, w=W)
    assert rel(got[2], st.fit) < 1e-5 and rel(got[0], st.alpha) < 1e-4 and abs(got[1] - st.sigma2) < 1e-8 * st.sigma2


def test_uploaded_basis_with_a_class_past_the_plane_width_stays_dense(ctx):
    """Class counts (49, 1, 1): separable, but no compact basis -- the results are those of option 0, bit for bit."""
    M = 300
    U, lam = _separable_basis(M, (49, 1, 1), seed=6)
    model, mo = _uploaded(M, U, lam, seed=7)
    x = _target(mo, 8)
    flags, got = _five_updates(ctx, model, x, mo, -1)
    assert flags == (True, (49, 1, 1), False)
    _same_bits(got, _five_updates(ctx, model, x, mo, 0)[1])


# ----------------------------------------------------------------------------------------------------------- not separable
@pytest.mark.parametrize("kind", ["dense", "one_foreign_entry"])
def test_not_separable_models_keep_the_dense_path(ctx, kind):
    M, rng = 300, np.random.default_rng(11)
    if kind == "dense":
        U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, 30)))
        lam = np.sort(rng.uniform(20.0, 400.0, 30))[::-1].copy()
    else:
        U, lam = _separable_basis(M, (10, 10, 10), seed=12)
        k = 7
        d = int(np.flatnonzero([np.any(U[c::3, k] != 0.0) for c in range(3)])[0])
        U[3 * 100 + (d + 1) % 3, k] = 1e-300
    model, mo = _uploaded(M, U, lam, seed=13)
    x = _target(mo, 14)
    flags, got = _five_updates(ctx, model, x, mo, -1)
    assert flags == (False, (0, 0, 0), False)
    _same_bits(got, _five_updates(ctx, model, x, mo, 0)[1])


def test_negative_zero_entries_count_as_zero(ctx):
    M = 300
    U, lam = _separable_basis(M, (10, 9, 8), seed=15)
    U[U == 0.0] = -0.0
    model, mo = _uploaded(M, U, lam, seed=16)
    x = _target(mo, 17)
    f = _fitter(ctx, model, x, mo)
    assert _flags(f) == (True, (10, 9, 8), True)
    for k in range(2):
        _check_one_update(f, mo, x, W, f"-0.0 basis, step {k}")
    f.close()


# -------------------------------------------------------------------------------------------------------------- exclusions
def _excluded_run(ctx, model, x, mo, opt, what):
    from gingr_amd import _native as nat
    with _Option(ctx, opt):
        f = _fitter(ctx, model, x, mo)
        assert _flags(f)[2]
        p = nat.CpdParams(W, 1.0)
        if what == "landmark":
            pid = np.array([5], dtype=np.int32)
            xyz = np.ascontiguousarray(x[:1] + 0.3)
            cov = np.ascontiguousarray(np.diag([0.5, 1.0, 2.0]).reshape(1, 9))
            assert f._lib.gingr_fitter_set_landmarks(f.handle, 1, nat.iptr(pid), nat.dptr(xyz), nat.dptr(cov)) == 0
            f.update_cpd(W, 1.0, 3)
        else:
            z = np.random.default_rng(21).normal(0, 1, mo.rank)
            assert f._lib.gingr_fitter_update_cpd_sample_async(f.handle, ctypes.byref(p), nat.dptr(z)) == 0
        out = _state_of(f)
        f.close()
    return out


@pytest.mark.parametrize("what", ["landmark", "sampled_proposal"])
def test_landmarks_and_sampled_proposals_take_the_dense_path(ctx, what):
    """One landmark set: every update is dense.  A sampled proposal (from the initial state) is dense as well."""
    model, mo = _gaussian(ctx, 257, 48, seed=2)
    x = _target(mo, 19)
    _same_bits(_excluded_run(ctx, model, x, mo, -1, what), _excluded_run(ctx, model, x, mo, 0, what))


def test_two_logical_shards_take_the_dense_path(ctx):
    import torch
    from gingr_amd import _native as nat
    from gingr_amd.sharded import NUM_PHASES, NUM_SEGMENTS, ShardedFitter
    model, mo = _gaussian(ctx, 1000, 48, seed=3)
    x = _target(mo, 23)
    s2 = ctx.cpd_initial_sigma2(mo.ref + mo.mean, x)

    def allreduce(tensors):
        ctx.synchronize()
        tot = torch.stack(tensors).sum(0)
        for t in tensors:
            t.copy_(tot)
        torch.cuda.synchronize()

    outs = []
    for opt in (-1, 0):
        with _Option(ctx, opt):
            shards = [ShardedFitter(ctx, model, x, rank=r, world=2, all_reduce=None, defer_setup=True) for r in range(2)]
            allreduce([s.gram_tensor() for s in shards])
            for s in shards:
                s.finish_setup()
                assert not _flags(s)[2]
                s.set_state(np.zeros(mo.rank), s2)
            p = nat.CpdParams(W, 1.0)
            for _ in range(2):
                for ph in range(NUM_PHASES):
                    for s in shards:
                        assert s._lib.gingr_fitter_cpd_phase_async(s.handle, ctypes.byref(p), ph) == 0
                    if ph < NUM_SEGMENTS:
                        allreduce([s._segment(ph) for s in shards])
            outs.append([_state_of(s) for s in shards])
            for s in shards:
                s.close()
    for a, b in zip(outs[0], outs[1]):
        _same_bits(a, b)


# --------------------------------------------------------------------------------------------------------------- failures
def test_nan_observation_weight_gives_the_same_status_on_both_paths(ctx):
    """The caller's pairs with one NaN variance (weight 1 / NaN): the posterior fails, with the same status and error code."""
    from gingr_amd import _native as nat
    model, mo = _gaussian(ctx, 257, 48, seed=2)
    x = _target(mo, 29)
    pid = np.arange(mo.M, dtype=np.int32)
    xyz = np.ascontiguousarray(mo.ref + mo.mean + 0.5)
    var = np.full(mo.M, 2.0)
    var[17] = np.nan
    seen = []
    for opt in (-1, 0):
        with _Option(ctx, opt):
            f = _fitter(ctx, model, x, mo)
            assert _flags(f)[2]
            f.update_cpd(W, 1.0, 1)   # (the fit pass with the quarter boxes, as in a CPD run)
            assert f._lib.gingr_fitter_set_pairs(f.handle, mo.M, nat.iptr(pid), nat.dptr(xyz), nat.dptr(var)) == 0
            assert f._lib.gingr_fitter_update_pairs_async(f.handle, 1) == 0
            _, sc, _ = f.get_state()
            err = c_int32()
            assert f._lib.gingr_fitter_last_update_error(f.handle, ctypes.byref(err)) == 0
            seen.append((int(sc.status), int(sc.iteration), int(err.value)))
            f.close()
    assert seen[0] == seen[1] and seen[0][2] != 0
