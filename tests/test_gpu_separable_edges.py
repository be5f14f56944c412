"""The compact passes of a coordinate-separable model (fitter_phases.hip: use_compact) at their class, row and solve edges, through
the C ABI only: gram_tri_kernel<3, true, 1> and the scatter branch of phase1_finalize_kernel element by element, the three-workgroup
posterior_solve_lds_kernel<2> on injected block systems and its per-block failure codes, sweep_fit_boxes_kernel<3, 4, true> with the
quarter boxes it leaves, the posterior memo across the compact / dense seam, and the exclusions bit for bit against
GINGR_OPT_SEPARABLE = 0.  Cases, references and bounds: tests/separable_cases.py (asserted on the host by
test_separable_cases_host.py); nothing here takes a tolerance from device output.

Row order.  Every model's reference is a line cloud (separable_cases.line_reference) whose k-d leaf order is the caller's order, so
the slabs and 16-row steps of gram_compact_plan fall on the rows the cases mark.

Reach (group c).  One predicate, use_compact, chooses the Gram pass, the solve and the fit pass of an update.  After phase 1 a finite
value is written into one pair of entries of G BETWEEN two classes, in the exchange segment.  posterior_solve_lds_kernel<2> gathers
the three diagonal blocks and never reads it: the committed alpha is that of the block systems.  The dense solve reads it: with the
option at 0 the same value changes alpha.  So where the block answer comes back, the three-block solve ran, and with it -- same
predicate, same update -- the compact Gram pass whose G and rhs the case has just checked.

Measured on an MI355X.  Every test prints its own figures with their bounds; the largest ratio figure / bound per group was collated
from the prints of one run of this file (no code here produces the aggregate):

    group                                     figure                  MI355X     bound      ratio   at
    a  Gram, pairs                            G, one entry            4.25e-09   3.68e-08   0.115   M = 17, (17, 15, 16), grouped 2-0-1
    a  Gram, pairs                            rhs, one entry          2.61e-09   3.03e-08   0.086   M = 17, (17, 15, 16), interleaved
    b  Gram, CPD                              G, one entry            2.03e-15   1.87e-13   0.011   M = 193, (48, 47, 17), random
    b  Gram, CPD                              rhs, one entry          1.51e-13   1.34e-11   0.011   M = 193, (48, 47, 17), random
    c  reach (block alpha, value between)     backward                3.06e-16   1.99e-14   0.015   a class of 17 columns
    c  reach, option 0 (must exceed 1)        forward                 --         --         3.2e5   the smallest over the cases
    d  three-block solve                      forward, zero           4.66e-16   2.45e-13   0.0019  block of 48
    d  three-block solve                      forward, ill            7.78e-10   4.75e-06   0.0002  block of 33
    d  three-block solve                      backward, graded_up     3.03e-16   7.06e-14   0.0043  block of 1
    d  three-block solve                      backward, graded_down   2.26e-16   8.74e-14   0.0026  block of 33
    e  failures                               status, iteration, error code and alpha equal to the dense solve's in every case;
                                              the non-SPD block beside the NaN block reported GINGR_ERR_NOT_SPD on both paths
    f  fit, one coordinate                    fit                     2.74e-17   5.74e-17   0.478   M = 10881, (48, 1, 0), the one-column class
    f  next update's statistics               den / P1 / PX           2.0e-13 / 1.9e-13 / 1.1e-13 against 1e-10 (M = 1 and 10881)
(Per-entry bounds: the row is the entry with the largest ratio.)
"""
import ctypes
import functools
from ctypes import c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import posterior_solve_cases as pc
from tests import separable_cases as sc
from tests.test_gpu_cpd_pair_pass_variants import REL_STATS, maxrel, rel
from tests.test_gpu_posterior_solve_variants import Injector
from tests.test_gpu_separable_model import _Option, _flags, _same_bits, _state_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")]

W, LAMBDA = 0.1, 2.0
SIGMA2 = 1.0


# ------------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=3)
def _parts(M, counts, order):
    ref, mean = sc.line_reference(M)
    U, lam, classes = sc.basis(M, counts, order)
    return ref, mean, U, lam, classes


def _model(parts):
    import gingr_amd as ga
    return ga.PointDistributionModel(parts[0], parts[1], parts[2], parts[3])


def _target(parts, seed, extra=7, noise=0.3):
    """every template point with a target within `noise`, `extra` more near points drawn from the template, shuffled"""
    rng = np.random.default_rng(seed)
    y = parts[0] + parts[1]
    x = np.concatenate([y, y[rng.integers(0, y.shape[0], extra)]]) + rng.normal(0, noise, (y.shape[0] + extra, 3))
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


def _fitter(ctx, model, x, alpha, sigma2=SIGMA2, transform=0):
    from gingr_amd.sharded import ShardedFitter
    f = ShardedFitter(ctx, model, x, global_transform=transform)
    f.set_state(alpha, sigma2)
    return f


def _segment1(ctx, f):
    """exchange segment 1 (G [rp rp], rhs [rp], ...) as a device tensor: read and written in place between phases 1 and 2"""
    from gingr_amd.sharded import as_torch
    ptr, offs, cnts = c_void_p(), (c_int64 * 2)(), (c_int64 * 2)()
    assert f._lib.gingr_fitter_exchange(f.handle, ctypes.byref(ptr), offs, cnts) == 0
    return as_torch(ptr.value, offs[1] + cnts[1], ctx.device)[offs[1]:]


def _phase(f, flavour, ph):
    from gingr_amd import _native as nat
    if flavour == "pairs":
        assert f._lib.gingr_fitter_pairs_phase_async(f.handle, ph) == 0
    else:
        p = nat.CpdParams(W, LAMBDA)
        assert f._lib.gingr_fitter_cpd_phase_async(f.handle, ctypes.byref(p), ph) == 0


def _last_error(f):
    err = c_int32(-1)
    assert f._lib.gingr_fitter_last_update_error(f.handle, ctypes.byref(err)) == 0
    return int(err.value)


def _worst(err, bound):
    """(largest err / bound, the error and the bound of that entry)"""
    err, bound = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    if err.size == 0:
        return 0.0, 0.0, 0.0
    out = np.zeros_like(err)
    np.divide(err, bound, out=out, where=bound > 0)
    out[(bound == 0) & (err > 0)] = np.inf
    k = int(np.argmax(out))
    return float(out[k]), float(err[k]), float(bound[k])


def _plus_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


def _block_figures(G, rhs, lam, classes, alpha):
    """per class: forward and backward figure of alpha (taken back through the alpha map) against the extended-precision block solve
    of (G, rhs), with 1000 x the figure of the plain float64 route on the same block (np.linalg.cholesky, two triangular solves, the
    map and back; floored at n 2^-53) -- the rule of test_gpu_posterior_solve_variants.py::test_real_state_readback"""
    a_ref = sc.block_solve(G, rhs, classes)
    cmap = pc.alpha_map_ld(lam)
    c64 = (lam / (lam + pc.EPS)) ** 2
    rows = []
    for d, cols in enumerate(sc.class_columns(classes)):
        n = len(cols)
        if n == 0:
            continue
        N = np.eye(n, dtype=pc.LD) + G[np.ix_(cols, cols)].astype(pc.LD)
        ref = {"a": a_ref[cols], "N": N, "L": None, "rhs": rhs[cols]}
        L64 = np.linalg.cholesky(np.eye(n) + G[np.ix_(cols, cols)])
        a64 = pc.backward_sub_t(L64, pc.forward_sub(L64, rhs[cols]))
        f64 = pc.figures(ref, (c64[cols] * a64).astype(pc.LD) / cmap[cols], None, None)
        got = pc.figures(ref, alpha[cols].astype(pc.LD) / cmap[cols], None, None)
        for k in ("forward", "backward"):
            rows.append((d, n, k, got[k], 1000.0 * f64[k] if f64[k] > 0.0 else n * 2.0 ** -53))
    return rows


# --------------------------------------------------------------------------------------- a, b, c: Gram, rhs, scatter; reach
def _gram_run(ctx, parts, flavour, option, M, seed, inject):
    """One fitter: phases 0 and 1, G / rhs of segment 1; `inject` = (i, j, value or None): written symmetrically into G before phase 2
    (None: chosen here from the diagonal, returned).  -> dict"""
    import torch
    from gingr_amd import _native as nat
    ref, mean, U, lam, classes = parts
    r, rp = len(classes), sc.rp_of(len(classes))
    out = {}
    with _Option(ctx, option):
        f = _fitter(ctx, _model(parts), _target(parts, seed), np.zeros(r))
        try:
            assert _flags(f) == (True, tuple(int(np.count_nonzero(classes == d)) for d in range(3)), True)
            if flavour == "pairs":
                pid, var, empty = sc.marker_pairs(M)
                xyz = np.ascontiguousarray((ref + mean)[pid] + np.random.default_rng(seed + 1).normal(0, 1.0, (len(pid), 3)))
                assert f._lib.gingr_fitter_set_pairs(f.handle, len(pid), nat.iptr(pid), nat.dptr(xyz), nat.dptr(np.ascontiguousarray(var))) == 0
                obs, w = np.empty((M, 3)), np.empty(M)
                assert f._lib.gingr_fitter_get_pair_observations(f.handle, nat.dptr(obs), nat.dptr(w)) == 0
                none = np.setdiff1d(np.arange(M), pid)
                assert _plus_zero(w[none]) and np.all(w[pid] > 0) and w.max() == 1e6  # (1 / 1e-6 is exact to rounding: 1e6)
                out.update(obs=obs, w=w)
            for ph in range(2):
                _phase(f, flavour, ph)
            ctx.synchronize()
            seg = _segment1(ctx, f)
            h = seg.cpu().numpy()
            G, rhs = h[: rp * rp].reshape(rp, rp).copy(), h[rp * rp: rp * rp + rp].copy()
            out.update(G=G, rhs=rhs)
            if flavour == "cpd":
                st = f.get_cpd_stats()
                _, _, fit = f.get_state()
                out.update(P1=st["P1"], PX=st["PX"], fit=fit)
            if inject is not None:
                i, j, v = inject
                if v is None:
                    v = 0.25 * float(np.sqrt((1.0 + G[i, i]) * (1.0 + G[j, j])))
                seg[i * rp + j] = v
                seg[j * rp + i] = v
                torch.cuda.synchronize(ctx.device)  # in place before phase 2 reads it
                _phase(f, flavour, 2)
                alpha, s, _ = f.get_state()
                out.update(alpha=alpha.copy(), status=int(s.status), error=_last_error(f), value=v)
        finally:
            f.close()
    return out


def _check_gram_case(ctx, M, counts, order, flavour):
    parts = _parts(M, counts, order)
    ref, mean, U, lam, classes = parts
    r, rp = len(classes), sc.rp_of(len(classes))
    seed = 100 + M + sum(counts)
    cols = sc.class_columns(classes)
    live = [d for d in range(3) if len(cols[d])]
    inject = (int(cols[live[0]][-1]), int(cols[live[-1]][0]), None) if len(live) >= 2 else None
    run = _gram_run(ctx, parts, flavour, -1, M, seed, inject)
    G, rhs = run["G"], run["rhs"]
    Q = sc.scaled_basis(U, lam)
    nslabs = len(sc.slabs(M))
    if flavour == "pairs":
        w, obs = run["w"], run["obs"]
    else:
        w, obs = sc.cpd_weight(run["P1"], SIGMA2, LAMBDA), sc.cpd_observation(run["fit"], run["P1"], run["PX"])
        assert np.all(np.isfinite(w)) and np.all(w > 0)
    e = sc.observation_e(w, obs, ref, mean)
    G_ref, rhs_ref, bG, brhs = sc.gram_bounds(Q, classes, w, e, obs, ref, mean, nslabs)
    same = classes[:, None] == classes[None, :]
    eG = np.abs(np.asarray(G[:r, :r].astype(pc.LD) - G_ref, dtype=np.float64))
    er = np.abs(np.asarray(rhs[:r].astype(pc.LD) - rhs_ref, dtype=np.float64))
    (fG, gG, hG), (fr, gr, hr) = _worst(eG[same], bG[same]), _worst(er, brhs)
    print(f"\n  gram {flavour} M={M} counts={counts} {order}: rows with weight {np.count_nonzero(w)} slabs {nslabs} | "
          f"G err/bound {fG:.3f} ({gG:.2e} / {hG:.2e}; largest |G| {np.abs(G).max():.2e}) | rhs err/bound {fr:.3f} ({gr:.2e} / {hr:.2e})")
    assert fG <= 1.0 and fr <= 1.0, (fG, fr)
    assert np.array_equal(G, G.T)                                                  # symmetric bit for bit
    assert _plus_zero(G[:r, :r][~same])                                            # +0.0 between the classes
    assert _plus_zero(G[r:, :]) and _plus_zero(G[:, r:]) and _plus_zero(rhs[r:])   # +0.0 padding
    if inject is None:
        return
    # ---- c: the block systems' alpha comes back although G holds a value between two classes: the three-block solve ran, and the same
    # predicate (use_compact) chose the compact Gram pass of this update, whose G / rhs were checked above
    assert run["status"] == 0 and run["error"] == 0 and np.all(np.isfinite(run["alpha"]))
    rows = _block_figures(G[:r, :r], rhs[:r], lam, classes, run["alpha"])
    for d, n, k, fig, bound in rows:
        print(f"    reach, option -1: class {d} ({n} columns) {k} {fig:.2e} bound {bound:.2e}")
    assert all(fig <= bound for _, _, _, fig, bound in rows), rows
    dense = _gram_run(ctx, parts, flavour, 0, M, seed, (inject[0], inject[1], run["value"]))
    moved = [fig / bound for _, _, k, fig, bound in _block_figures(G[:r, :r], rhs[:r], lam, classes, dense["alpha"]) if k == "forward"]
    print(f"    reach, option 0: value {run['value']:.3e} at ({inject[0]}, {inject[1]}): forward / bound {max(moved):.2e}, status {dense['status']}, error {dense['error']}")
    assert max(moved) > 1.0 and not np.array_equal(dense["alpha"], run["alpha"])  # the dense solve used the value (or failed on it)


GRAM_CASES = [(257, c, "interleaved") for c in sc.COUNTS]
GRAM_CASES += [(M, c, o) for c in ((48, 47, 17), (17, 15, 16)) for M in sc.ROWS if sc.admits(M, c) for o in sc.ORDERS
               if (M, c, o) not in GRAM_CASES]
GRAM_CASES += [(1, (1, 1, 1), "interleaved")] + [(M, (3, 2, 1), "interleaved") for M in (15, 16, 17)]


@pytest.mark.parametrize("M,counts,order", GRAM_CASES, ids=[f"{M}-{'.'.join(map(str, c))}-{o}" for M, c, o in GRAM_CASES])
def test_gram_rhs_scatter_and_reach_pairs(ctx, M, counts, order):
    """a + c: the isotropic-pairs flavour with vertices and one whole slab without a pair, variances over twelve decades and the
    largest weights on the first and last row of every slab."""
    _check_gram_case(ctx, M, counts, order, "pairs")


CPD_GRAM_CASES = [(193, (48, 47, 17), "random"), (10881, (48, 47, 17), "grouped_201"), (257, (48, 1, 0), "interleaved")]


@pytest.mark.parametrize("M,counts,order", CPD_GRAM_CASES, ids=[f"{M}-{'.'.join(map(str, c))}-{o}" for M, c, o in CPD_GRAM_CASES])
def test_gram_rhs_scatter_and_reach_cpd(ctx, M, counts, order):
    """b + c: w = P1 / (sigma^2 lambda) with lambda = 2 from the statistics of phase 0 (gingr_fitter_get_cpd_stats)."""
    _check_gram_case(ctx, M, counts, order, "cpd")


# ------------------------------------------------------------------------------------------------ d: the three-block solve
BLOCK_M = 257


def _block_parts(counts):
    return _parts(BLOCK_M, counts, "random")


def _block_system(classes, case):
    blocks = [(np.zeros((0, 0)), np.zeros(0)) if c is None else pc.make_case(c[0], c[1])[:2] for c in case]
    return sc.scatter_blocks(classes, blocks)


@pytest.mark.parametrize("case", sc.BLOCK_CASES, ids=["-".join("none" if c is None else f"{c[0]}{c[1]}" for c in case) for case in sc.BLOCK_CASES])
def test_three_block_solve_on_injected_systems(ctx, case):
    """posterior_solve_lds_kernel<2>: a different family of posterior_solve_cases.make_case in each class, scattered to the class
    positions of a randomly ordered separable basis; per block the forward and backward figure against the extended-precision
    solve_all of that block, bounds gpu_bound(family, figure, block size)."""
    counts = sc.block_counts(case)
    parts = _block_parts(counts)
    lam, classes = parts[3], parts[4]
    r = len(classes)
    assert pc.route_of(r, False, compact=pc.uses_compact(r, counts)) == "posterior_solve_lds_kernel<2>"
    G, rhs = _block_system(classes, case)
    cmap = pc.alpha_map_ld(lam)
    inj = Injector(ctx, r, parts=parts[:4])
    failures = []
    try:
        assert _flags(inj.sf) == (True, counts, True)
        alpha, status = inj.update(G, rhs)
        assert status == 0 and np.all(np.isfinite(alpha))
        print()
        for cols, c in zip(sc.class_columns(classes), case):
            if c is None:
                continue
            fam, n = c
            fig = pc.figures(pc.reference(fam, n), alpha[cols].astype(pc.LD) / cmap[cols], None, None)
            for k in ("forward", "backward"):
                bound = pc.gpu_bound(fam, k, n)
                print("    %-30s %-12s n=%-3d %-9s %.2e  bound %.2e  float64 %.2e" % ("posterior_solve_lds_kernel<2>", fam, n, k, fig[k], bound,
                                                                                      pc.F64_FIGURES[fam][k]))
                if not fig[k] <= bound:
                    failures.append((fam, n, k, fig[k], bound))
    finally:
        inj.close()
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ e: failures per block
FAIL_SIZES = (48, 17, 31)
HEALTHY = (("well", 48), ("graded_up", 17), ("diagonal", 31))
# name -> (family replaced per class or None, class whose rhs gets a NaN or None, both kinds of failure at once)
FAILURES = {
    "notpd_class0": (("notpd", None, None), None, False),
    "notpd_class2": ((None, None, "notpd"), None, False),
    "notpd_last_at_48": (("notpd_last", None, None), None, False),
    "nan_rhs_class1": ((None, None, None), 1, False),
    "notpd_class0_beside_nan_class1": (("notpd", None, None), 1, True),
}


def _update_from(inj, alpha0, G, rhs, iteration):
    """Injector.update from a state with coefficients alpha0 -> (alpha, status, iteration, error code)"""
    nat = inj.nat
    inj.sf.set_state(alpha0, inj.sigma2, iteration=iteration)
    inj.inject = (G, rhs, None)
    cp = nat.CpdParams(0.1, 1.0)
    rc = inj.sf._lib.gingr_fitter_update_sharded_async(inj.sf.handle, 0, ctypes.byref(cp), None, 1, None, inj.cb, None)
    inj.inject = None
    if inj.cb_error is not None:
        raise inj.cb_error
    assert rc == 0, rc
    alpha, s, fit = inj.sf.get_state()
    return alpha.copy(), int(s.status), int(s.iteration), _last_error(inj.sf), fit.copy()


@pytest.mark.parametrize("name", list(FAILURES))
def test_block_failures_match_the_dense_solve(ctx, name):
    """One block not positive definite or one right-hand side not finite: status, iteration, error code and the bits of the unchanged
    alpha are those of the dense solve on the same injected system, at iteration 0 (state unchanged) and later (ModelFlexibilityError);
    a healthy update afterwards on the same fitter gives the bits of a fresh one."""
    from gingr_amd import _native as nat
    replaced, nan_class, either = FAILURES[name]
    parts = _block_parts(FAIL_SIZES)
    classes = parts[4]
    r = len(classes)
    case = tuple((fam or h[0], h[1]) for fam, h in zip(replaced, HEALTHY))
    G, rhs = _block_system(classes, case)
    if nan_class is not None:
        rhs[sc.class_columns(classes)[nan_class][3]] = np.nan
    G_ok, rhs_ok = _block_system(classes, HEALTHY)
    alpha0 = np.random.default_rng(8).normal(0, 0.3, r)
    seen = {}
    for opt in (-1, 0):
        with _Option(ctx, opt):
            inj = Injector(ctx, r, parts=parts[:4])
            try:
                assert _flags(inj.sf)[2]
                outs = [_update_from(inj, alpha0, G, rhs, it)[:4] for it in (0, 1)]
                after = _update_from(inj, alpha0, G_ok, rhs_ok, 1)
                fresh = Injector(ctx, r, parts=parts[:4])
                try:
                    want = _update_from(fresh, alpha0, G_ok, rhs_ok, 1)
                finally:
                    fresh.close()
            finally:
                inj.close()
        print(f"\n  {name}, option {opt}: (status, iteration, error) at iteration 0 {outs[0][1:]}, later {outs[1][1:]}; healthy afterwards {after[1:4]}")
        assert after[1] == 0 and after[3] == 0
        _same_bits(after, want)
        seen[opt] = outs
    for (a_c, st_c, it_c, err_c), (a_d, st_d, it_d, err_d), later in zip(seen[-1], seen[0], (False, True)):
        assert np.array_equal(a_c, alpha0) and np.array_equal(a_d, alpha0)     # the bits of the unchanged alpha
        assert (st_c, it_c) == (st_d, it_d)
        assert st_c == (3 if later else 0)                                     # ModelFlexibilityError later, state unchanged at iteration 0
        if either:
            assert err_c in (nat.ERR_NOT_SPD, nat.ERR_NONFINITE) and err_d in (nat.ERR_NOT_SPD, nat.ERR_NONFINITE)
        else:
            assert err_c == err_d == (nat.ERR_NONFINITE if nan_class is not None else nat.ERR_NOT_SPD)


# ------------------------------------------------------------------------------------------------ f: fit pass and its boxes
FIT_CASES = [(M, c) for c in ((48, 1, 0), (0, 48, 48), (48, 47, 17)) for M in (1, 17, 65, 193, 257, 10881)]


@pytest.mark.parametrize("M,counts", FIT_CASES, ids=[f"{M}-{'.'.join(map(str, c))}" for M, c in FIT_CASES])
def test_fit_pass_and_the_boxes_it_leaves(ctx, M, counts):
    """One compact update without a global transform: every coordinate of the fit within the fit bound of ref + mean + Q alpha (alpha
    as read back); a coordinate whose class is empty is ref + mean bit for bit.  Then a second update, whose CPD passes cull with the
    quarter boxes the fit pass left: its P1, PX and den (the statistics of the evaluation AT the read-back fit) against the C
    restatement on that fit with the bounds of tests/test_gpu_cpd_pair_pass_variants.py -- a box too small would cull pairs that count."""
    parts = _parts(M, counts, "interleaved")
    ref, mean, U, lam, classes = parts
    r = len(classes)
    x = _target(parts, 300 + M)
    f = _fitter(ctx, _model(parts), x, np.zeros(r))
    try:
        assert _flags(f) == (True, counts, True)
        f.update_cpd(W, 1.0, 1)
        alpha, s, fit = f.get_state()
        assert int(s.status) == 0 and _last_error(f) == 0 and alpha.any()
        sigma2 = float(s.sigma2)
        fit = fit.copy()
        f.update_cpd(W, 1.0, 1)
        ctx.synchronize()
        stats = f.get_cpd_stats()
        assert int(f.get_state()[1].status) == 0
    finally:
        f.close()
    want_fit, bound = sc.fit_reference(ref, mean, sc.scaled_basis(U, lam), alpha, classes)
    fig, fig_err, fig_bound = _worst(np.abs(np.asarray(fit.astype(pc.LD) - want_fit, dtype=np.float64)), bound)
    for d in range(3):
        if counts[d] == 0:
            assert np.array_equal(fit[:, d], (ref + mean)[:, d])
    want = co.cpd_stats(fit, x, sigma2, W)
    assert want.P1.min() > 1e-3 and want.den.min() > 1e-12, (want.P1.min(), want.den.min())  # (relative errors over ALL elements mean something)
    figs = {"den": maxrel(stats["den"], want.den), "P1": maxrel(stats["P1"], want.P1), "PX": rel(stats["PX"], want.PX)}
    print(f"\n  fit M={M} counts={counts}: fit err/bound {fig:.3f} ({fig_err:.2e} / {fig_bound:.2e}) | next update at sigma2 {sigma2:.4f}: " +
          " ".join(f"{k} {v:.2e}" for k, v in figs.items()) + f" bound {REL_STATS:.0e}")
    assert fig <= 1.0, fig
    assert max(figs.values()) < REL_STATS, figs


# ------------------------------------------------------------------------------------------------ g: memo seam
def _logpdf(f, mesh):
    from gingr_amd import _native as nat
    cp = nat.CpdParams(W, 1.0)
    out = ctypes.c_double(float("nan"))
    m = nat.f64(mesh)
    assert f._lib.gingr_fitter_posterior_logpdf_cpd(f.handle, ctypes.byref(cp), nat.dptr(m), ctypes.byref(out)) == 0
    return float(out.value)


def _seam_case():
    parts = _parts(257, (48, 47, 17), "random")
    r = len(parts[4])
    rng = np.random.default_rng(41)
    alpha0 = rng.normal(0, 0.2, r)
    x = _target(parts, 42)
    mesh = parts[0] + parts[1] + rng.normal(0, 0.2, parts[0].shape)
    return parts, r, alpha0, x, mesh


def _script(ctx, steps, transform=1):
    """One fresh fitter (created under the option of the first step), then the steps in order: ("opt", v), ("set",), ("update",),
    ("query",).  -> (states after every update, values of every query)"""
    from gingr_amd import _native as nat
    parts, r, alpha0, x, mesh = _seam_case()
    before = ctx.get_option(nat.OPT_SEPARABLE)
    states, values = [], []
    f = None
    try:
        for step in steps:
            if step[0] == "opt":
                ctx.set_option(nat.OPT_SEPARABLE, step[1])
                continue
            if f is None:
                f = _fitter(ctx, _model(parts), x, alpha0, transform=transform)
                assert _flags(f)[2]
            if step[0] == "set":
                f.set_state(alpha0, SIGMA2)
            elif step[0] == "update":
                f.update_cpd(W, 1.0, 1)
                states.append(_state_of(f))
            else:
                values.append(_logpdf(f, mesh))
    finally:
        if f is not None:
            f.close()
        ctx.set_option(nat.OPT_SEPARABLE, before)
    return states, values


def test_memo_does_not_mix_compact_and_dense_sums(ctx):
    """A query runs the dense passes (allow_alt), an update the compact ones, and the posterior memo hands phase-1 results only to a
    caller that would have computed them the same way (the key holds use_compact): every sequence gives the bits of its own path."""
    S, U_, Q = ("set",), ("update",), ("query",)
    alone, _ = _script(ctx, [("opt", -1), S, U_])
    dense_alone, _ = _script(ctx, [("opt", 0), S, U_])
    _, lp_alone = _script(ctx, [("opt", -1), S, Q])
    assert alone[0][3] == 0 and dense_alone[0][3] == 0 and np.isfinite(lp_alone[0])
    differ = not all(np.array_equal(a, b) for a, b in zip(alone[0], dense_alone[0]))
    print(f"\n  memo seam: the compact and the dense update differ in their bits: {differ}; logpdf {lp_alone[0]:.6f}")
    assert differ  # (otherwise nothing below could tell the two paths apart)
    # query, then update: the update recomputes phase 1 on its own path
    st, lp = _script(ctx, [("opt", -1), S, Q, U_])
    assert lp[0] == lp_alone[0]
    _same_bits(st[0], alone[0])
    # update, then the same state again: query (dense sums), update (compact sums again)
    want2, _ = _script(ctx, [("opt", -1), S, U_, S, U_])
    _same_bits(want2[1], alone[0])
    st, lp = _script(ctx, [("opt", -1), S, U_, S, Q, U_])
    assert lp[0] == lp_alone[0]
    _same_bits(st[0], alone[0])
    _same_bits(st[1], alone[0])
    # update, query, update in a row: the second update starts from the first one's state
    two, _ = _script(ctx, [("opt", -1), S, U_, U_])
    st, _ = _script(ctx, [("opt", -1), S, U_, Q, U_])
    _same_bits(st[1], two[1])
    # the option flipped between two updates from the same set_state, both ways
    st, _ = _script(ctx, [("opt", -1), S, U_, ("opt", 0), S, U_])
    _same_bits(st[0], alone[0])
    _same_bits(st[1], dense_alone[0])
    st, _ = _script(ctx, [("opt", 0), S, U_, ("opt", -1), S, U_])
    _same_bits(st[0], dense_alone[0])
    _same_bits(st[1], alone[0])
    # the query is dense under either option
    _, lp0 = _script(ctx, [("opt", 0), S, Q])
    assert lp0[0] == lp_alone[0]


# ------------------------------------------------------------------------------------------------ h: exclusions
def _group_of_one(option):
    import gingr_amd as ga
    from gingr_amd import _native as nat
    parts, r, alpha0, x, _ = _seam_case()
    g = ga.DeviceGroup([0])
    try:
        assert g._lib.gingr_ctx_set_option(g.ctx_handle(0), nat.OPT_SEPARABLE, option) == 0
        g.upload_model(parts[0], parts[1], parts[2], parts[3])
        g.set_target(x)
        g.set_options(1, 1.0)
        g.set_state(alpha0, SIGMA2)
        g.update_cpd(W, 1.0, 2)
        a, s, fit = g.get_state()
        return a.copy(), float(s.sigma2), fit.copy(), int(s.status), int(s.iteration)
    finally:
        g.close()


def _pairs_with_one_covariance_pair(ctx, option):
    from gingr_amd import _native as nat
    parts, r, alpha0, x, _ = _seam_case()
    M = parts[0].shape[0]
    pid, var, _ = sc.marker_pairs(M)
    xyz = np.ascontiguousarray((parts[0] + parts[1])[pid] + np.random.default_rng(43).normal(0, 1.0, (len(pid), 3)))
    cp, cx = np.array([11], dtype=np.int32), np.ascontiguousarray((parts[0] + parts[1])[[11]] + 0.7)
    cc = np.ascontiguousarray(np.array([[0.5, 0.1, 0.0], [0.1, 1.0, 0.2], [0.0, 0.2, 2.0]]).reshape(1, 9))
    with _Option(ctx, option):
        f = _fitter(ctx, _model(parts), x, alpha0, transform=1)
        try:
            assert _flags(f)[2]
            assert f._lib.gingr_fitter_set_pairs(f.handle, len(pid), nat.iptr(pid), nat.dptr(xyz), nat.dptr(np.ascontiguousarray(var))) == 0
            assert f._lib.gingr_fitter_set_pairs_cov(f.handle, 1, nat.iptr(cp), nat.dptr(cx), nat.dptr(cc)) == 0
            assert f._lib.gingr_fitter_update_pairs_async(f.handle, 2) == 0
            return _state_of(f)
        finally:
            f.close()


def _mh_step(ctx, option):
    from gingr_amd import _native as nat
    from tests.test_gpu_posterior_solve_variants import _triangle_strip
    parts, r, alpha0, x, _ = _seam_case()
    with _Option(ctx, option):
        f = _fitter(ctx, _model(parts), x, alpha0, transform=1)
        try:
            assert _flags(f)[2]
            f.set_meshes(_triangle_strip(parts[0].shape[0]), _triangle_strip(x.shape[0]))
            f.set_state(alpha0, SIGMA2)
            cp = nat.CpdParams(W, 1.0)
            req, res, alpha = nat.MhRequest(), nat.MhResult(), np.empty(r)
            req.flavour, req.kind, req.cpd, req.eval_sdev, req.eval_points, req.need_forward = 0, 0, ctypes.pointer(cp), 5.0, 0, 1
            z = nat.f64(np.random.default_rng(44).normal(0, 1, r))
            req.z = nat.dptr(z)
            assert f._lib.gingr_fitter_mh_step(f.handle, ctypes.byref(req), nat.dptr(alpha), None, ctypes.byref(res)) == 0
            assert res.scalars.status == 0 and res.forward_status == 0
            return alpha.copy(), float(res.scalars.sigma2), float(res.log_value), float(res.log_q_forward), float(res.dist_sum)
        finally:
            f.close()


def _query_alone(ctx, option):
    return _script(ctx, [("opt", option), ("set",), ("query",)])[1]


@pytest.mark.parametrize("what", ["device_group_of_one", "one_covariance_pair", "mh_step", "logpdf_query"])
def test_exclusions_keep_the_dense_bits(ctx, what):
    """What use_compact excludes gives, on a model that keeps its compact basis, the bits of GINGR_OPT_SEPARABLE = 0."""
    run = {"device_group_of_one": lambda o: _group_of_one(o), "one_covariance_pair": lambda o: _pairs_with_one_covariance_pair(ctx, o),
           "mh_step": lambda o: _mh_step(ctx, o), "logpdf_query": lambda o: _query_alone(ctx, o)}[what]
    got, want = run(-1), run(0)
    assert all(np.all(np.isfinite(np.asarray(v))) for v in got)
    _same_bits(got, want)
