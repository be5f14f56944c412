"""GPU tests of the low-rank Bayesian coherent point drift (gingr_bcpd_create_lowrank; gingr_amd/csrc/bcpd_lowrank.hip,
classic.BCPD(lowRank=...)): single iterations against the numpy restatement over G := L L^T (tests/bcpd_lowrank_restatement.py), L the
factor the device holds; the factor against the classic low-rank task's; the distance from the true dense route; a template past the
dense limit; determinism, the stop rule, the wrapper, refusals and leaks.  The bounds are those tests/test_gpu_bcpd.py holds the dense
route to: 1e-9 relative for point sets and vectors, 1e-8 for variances, sigma_m^2 to 1e-9 max K_mm ABSOLUTE (K_mm = |l_m|^2 / lambda
here), 1e-6 for whole registrations."""
import functools
import gc

import numpy as np
import pytest

from tests import bcpd_lowrank_restatement as blr
from tests import bcpd_restatement as br
from tests import lowrank_cpd_restatement as lr

pytestmark = pytest.mark.gpu

W_OUTLIER = 0.05

# (name, M, N, beta, tolerance, maxColumns, w)
ALGEBRA = [
    ("pair", 130, 150, 6.0, 1e-2, 0, W_OUTLIER),     # k = 98: no multiple of 16, two column blocks, M no multiple of 32
    ("pair", 130, 150, 6.0, 1e-8, 0, W_OUTLIER),     # k = M
    ("pair", 500, 420, 10.0, 1e-4, 0, W_OUTLIER),    # k = 200
    ("pair", 700, 600, 12.0, 1e-12, 0, W_OUTLIER),   # the ceiling of 512 columns: all 36 block pairs
    ("pair", 500, 420, 10.0, 1e-8, 1, W_OUTLIER),    # a single column
    ("hull", 1500, 1125, 25.0, 1e-2, 0, W_OUTLIER),  # k = 31: one block
    ("g6", 216, 194, 1.5, 1e-4, 0, 0.0),             # the grid of test_gpu_bcpd.py without outliers
]


@functools.lru_cache(maxsize=None)
def inputs(name, M, N):
    if name == "g6":
        y, x = br.grid_case(6)
    elif name == "g7":
        y, x = br.grid_case(7)
    elif name == "hull":
        y, x = lr.hull(M, N)
    else:
        y, x = lr.pair(M, N, 7 + M, noise=0.3)
    assert y.shape == (M, 3) and x.shape == (N, 3)
    y.setflags(write=False)
    x.setflags(write=False)
    return y, x


def make(ctx, y, x, beta, tol, max_columns, w=W_OUTLIER):
    from gingr_amd import classic as cl
    return cl.BCPD(ctx, y, x, w=w, lambda_=br.PARAMS["lambda_"], gamma=br.PARAMS["gamma"], k=br.PARAMS["kappa"], beta=beta,
                   lowRank=cl.LowRankG(tol, max_columns))


def inject(reg, st):
    reg.set_state(st.yhat, st.sig, st.alpha, st.s, st.R, st.t, st.sigma2)


def compare(got, want, p, label=""):
    """the bounds of test_gpu_bcpd.py::compare, with max K_mm = max |l_m|^2 / lambda"""
    fig = dict(yhat=br.rel(got["yhat"], want.yhat), vhat=br.rel(got["vhat"], want.vhat), uhat=br.rel(p.y + got["vhat"], p.y + want.vhat),
               alpha=br.rel(got["alpha"], want.alpha), nu=br.rel(got["nu"], want.nu), nu_prime=br.rel(got["nu_prime"], want.nu_prime),
               sigma_diag=float(np.abs(got["sigma_diag"] - want.sig).max() / p.kmax),
               s=abs(got["s"] - want.s) / abs(want.s), R=float(np.abs(got["R"] - want.R).max()), t=br.rel(got["t"], want.t),
               sigma2=abs(got["sigma2"] - want.sigma2) / abs(want.sigma2), sigma_bar2=abs(got["sigma_bar2"] - want.sigma_bar2) / want.sigma_bar2)
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()), f"min_nu={want.nu.min():.2e}")
    for k in ("yhat", "vhat", "uhat", "alpha", "nu", "nu_prime", "sigma_diag", "t", "s", "R"):
        assert fig[k] < 1e-9, (label, k, fig[k])
    assert fig["sigma2"] < 1e-8 and fig["sigma_bar2"] < 1e-8, (label, fig["sigma2"], fig["sigma_bar2"])
    assert got["sigma_diag"].min() >= 0.0, label                # a sum of squares
    return fig


# --------------------------------------------------------------------------------------------------- single iterations
@pytest.mark.parametrize("name,M,N,beta,tol,max_columns,w", ALGEBRA)
def test_single_iterations_from_the_restatements_states(ctx, name, M, N, beta, tol, max_columns, w):
    """Three iterations, each injected from the state the Woodbury route of the restatement over G := L L^T left."""
    y, x = inputs(name, M, N)
    reg = make(ctx, y, x, beta, tol, max_columns, w)
    try:
        info, L = reg.lowRankInfo, reg.factor()
        assert L.shape == (M, info["columns"])
        if (M, tol) == (130, 1e-2):
            assert info["columns"] == 98, info
        if (M, tol) == (130, 1e-8):
            assert info["columns"] == M and info["tolerance_reached"], info
        if tol == 1e-12:
            assert info["columns"] == 512 and not info["tolerance_reached"], info
        if max_columns == 1:
            assert info["columns"] == 1 and not info["tolerance_reached"], info
        if name == "hull":
            assert info["columns"] == 31, info
        p = blr.Problem(y, x, L, w=w, beta=beta, **br.PARAMS)
        st = p.initial()
        for it in range(3):
            inject(reg, st)
            reg.Iteration()
            st = p.iterate(st, "woodbury")
            compare(reg.state(), st, p, label=f"{name} M {M} k {info['columns']} from {it}")
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------------ one factor build
def test_the_factor_is_the_classic_low_rank_tasks(ctx):
    from gingr_amd import classic as cl
    for name, M, N, beta, tol, max_columns in [("pair", 130, 150, 6.0, 1e-2, 0), ("pair", 500, 420, 10.0, 1e-8, 17)]:
        y, x = inputs(name, M, N)
        reg = make(ctx, y, x, beta, tol, max_columns)
        classic = cl.CPDFactory(ctx, y, lambda_=2.0, beta=beta, w=W_OUTLIER).registerNonRigidly(x, lowRank=cl.LowRankG(tol, max_columns))
        try:
            assert set(reg.lowRankInfo) == {"columns", "tolerance_reached", "residual_fraction", "factor_bytes"}
            assert reg.lowRankInfo == classic.lowRankInfo
            assert np.array_equal(reg.factor(), classic.factor())
        finally:
            reg.close()
            classic.close()


# --------------------------------------------------------------------------------------------- against the true dense route
def test_free_run_against_the_true_dense_route(ctx):
    """grid_case(7), beta 2, tolerance 1e-8, w = 0.1: ten iterations of a low-rank handle against ten of a dense handle.  The bound is ten times
    the distance of the two routes in the restatement (CPU against CPU, true G against the oracle's factor, 327 columns), because the
    device's own rounding of both routes sits below it.  Measured on the CPU after ten iterations: yhat 4.3e-10, s 9.0e-10,
    sigma2 3.1e-9 (relative; a single step from the initial state differs by 4.1e-11 in uhat)."""
    from gingr_amd import classic as cl
    y, x = inputs("g7", 343, 308)
    kw = dict(w=0.1, beta=2.0, **br.PARAMS)
    oL = lr.factor(y, 2.0, 1e-8)
    assert oL.shape[1] == 327
    a, b = br.Problem(y, x, **kw).run(10, keep=(10,))[10], blr.Problem(y, x, oL, **kw).run(10, keep=(10,))[10]
    d_ref = (br.rel(b.yhat, a.yhat), abs(b.s - a.s) / a.s, abs(b.sigma2 - a.sigma2) / a.sigma2)
    print("CPU, low-rank against dense after ten iterations: yhat %.2e s %.2e sigma2 %.2e" % d_ref)
    dkw = dict(w=0.1, lambda_=br.PARAMS["lambda_"], gamma=br.PARAMS["gamma"], k=br.PARAMS["kappa"], beta=2.0)
    dense, low = cl.BCPD(ctx, y, x, **dkw), cl.BCPD(ctx, y, x, lowRank=cl.LowRankG(1e-8), **dkw)
    try:
        gd, gl = dense.Registration(10, tolerance=0.0), low.Registration(10, tolerance=0.0)
        sd, sl = dense.state(), low.state()
        d_dev = (br.rel(gl, gd), abs(sl["s"] - sd["s"]) / sd["s"], abs(sl["sigma2"] - sd["sigma2"]) / sd["sigma2"])
        print("device, low-rank against dense after ten iterations: yhat %.2e s %.2e sigma2 %.2e" % d_dev, low.lowRankInfo)
        for dev, ref in zip(d_dev, d_ref):
            assert dev <= 10.0 * ref, (d_dev, d_ref)
    finally:
        dense.close()
        low.close()


# ------------------------------------------------------------------------------------------------- past the dense limit
def _free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def test_past_the_dense_limit(ctx):
    """33 001 template points: the dense create refuses with its text, the low-rank one builds to the tolerance, holds no M x M buffer
    (a dense handle would take 26 GB) and meets the bounds of the single iterations against the k-space restatement, whose assignment
    goes by slabs.  No M x M array on either side."""
    from gingr_amd import classic as cl, GingrNativeError
    from gingr_amd import _native as nat
    M, N, beta = 33001, 2000, 25.0
    y, x = inputs("hull", M, N)
    with pytest.raises(GingrNativeError) as e:
        cl.BCPD(ctx, y, x, w=W_OUTLIER, beta=beta)
    assert e.value.code == nat.ERR_BAD_ARGUMENT and "bcpd_create: template too large (M <= 32768" in str(e.value)
    gc.collect()
    before = _free_bytes()
    reg = make(ctx, y, x, beta, 1e-4, 0)
    try:
        held = before - _free_bytes()
        info = reg.lowRankInfo
        print(f"M {M}: {info}, device memory held {held / 2**20:.0f} MiB")
        assert info["tolerance_reached"] and info["residual_fraction"] < 1e-4 and 16 < info["columns"] < 512, info
        assert held < 1 << 30, held
        p = blr.Problem(y, x, reg.factor(), w=W_OUTLIER, beta=beta, dense=False, **br.PARAMS)
        st = p.initial()
        for it in range(2):
            inject(reg, st)
            reg.Iteration()
            st = p.iterate(st, "lowrank")
            compare(reg.state(), st, p, label=f"hull M {M} k {info['columns']} from {it}")
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------------------- determinism
def test_two_handles_give_the_same_bits(ctx):
    y, x = inputs("pair", 500, 420)
    out = []
    for _ in range(2):
        reg = make(ctx, y, x, 10.0, 1e-4, 0)
        try:
            for _ in range(5):
                reg.Iteration()
            out.append(reg.state())
        finally:
            reg.close()
    for k in ("yhat", "vhat", "sigma_diag", "alpha", "nu", "nu_prime", "R", "t"):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert out[0]["sigma2"] == out[1]["sigma2"] and out[0]["s"] == out[1]["s"] and out[0]["sigma_bar2"] == out[1]["sigma_bar2"]


# ------------------------------------------------------------------------------------------------------ loop and wrapper
def test_stop_rule_and_wrapper(ctx):
    from gingr_amd import classic as cl
    y, x = inputs("g6", 216, 194)
    kw = dict(w=0.1, lambda_=br.PARAMS["lambda_"], gamma=br.PARAMS["gamma"], k=br.PARAMS["kappa"], beta=1.5, lowRank=cl.LowRankG(1e-4))
    reg = cl.BCPD(ctx, y, x, **kw)
    try:
        p = blr.Problem(y, x, reg.factor(), w=0.1, beta=1.5, **br.PARAMS)
        want, iterations, converged = p.registration(100, 1e-6)
        assert converged and 10 < iterations < 100
        got = reg.Registration(100, tolerance=1e-6)
        assert reg.converged and reg.iterations == iterations
        assert br.rel(got, want.yhat) < 1e-6
        a = reg.Registration(12)
    finally:
        reg.close()
    b = cl.BCPDRegistration(ctx, y, max_iterations=12, **kw).register(x)
    assert a.shape == (216, 3) and np.array_equal(a, b)
    assert cl.BCPDRegistration(ctx, y).lowRank is None


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    from gingr_amd import classic as cl, GingrNativeError
    from gingr_amd import _native as nat
    y, x = br.grid_case(3)
    good = dict(w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=1.5)
    for bad in (cl.LowRankG(1.0), cl.LowRankG(-0.1), cl.LowRankG(float("nan")), cl.LowRankG(1e-8, 513)):
        with pytest.raises(GingrNativeError) as e:
            cl.BCPD(ctx, y, x, lowRank=bad, **good)
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "bcpd_create_lowrank" in str(e.value), (bad.relativeTolerance, bad.maxColumns)
    flat = x.copy()
    flat[:, 2] = 0.25
    for change in (dict(w=1.0), dict(w=-0.1), dict(lambda_=0.0), dict(gamma=0.0), dict(k=0.0), dict(beta=0.0)):
        with pytest.raises(GingrNativeError) as e:
            cl.BCPD(ctx, y, x, lowRank=cl.LowRankG(), **{**good, **change})
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "bcpd_create" in str(e.value), change
    for yy, xx in [(y[:0], x), (y, x[:0]), (y, flat)]:
        with pytest.raises(GingrNativeError) as e:
            cl.BCPD(ctx, yy, xx, lowRank=cl.LowRankG(), **good)
        assert e.value.code == nat.ERR_BAD_ARGUMENT, (yy.shape, xx.shape)
    # tolerance 0 and maxColumns = 512 are the ends of the valid ranges; kappa = +inf is allowed
    reg = cl.BCPD(ctx, y, x, lowRank=cl.LowRankG(0.0, 512), **{**good, "k": np.inf})
    assert reg.lowRankInfo["columns"] == 27
    reg.close()
    dense = cl.BCPD(ctx, y, x, **good)
    try:
        assert dense.lowRankInfo is None
        with pytest.raises(GingrNativeError) as e:
            dense.factor()
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "bcpd_get_factor" in str(e.value)
    finally:
        dense.close()


def test_unreachable_target_point_reports_nonfinite_and_the_handle_survives(ctx):
    """the flag path of the dense route (test_gpu_bcpd.py): w = 0 and a target point out of reach of every template point"""
    from gingr_amd import GingrNativeError
    from gingr_amd import _native as nat
    y, x = inputs("g6", 216, 194)
    far = np.array(x)
    far[17] += 1e6
    reg = make(ctx, y, far, 1.5, 1e-4, 0, w=0.0)
    try:
        p = blr.Problem(y, far, reg.factor(), w=0.0, beta=1.5, **br.PARAMS)
        near = blr.Problem(y, x, p.L, w=0.0, beta=1.5, **br.PARAMS)
        st = near.run(10, keep=(10,))[10]                         # a state whose sigma2 is small against 1e6
        with np.errstate(all="ignore"):
            assert not np.isfinite(p.assignment(st)[1]).all()
        inject(reg, st)
        with pytest.raises(GingrNativeError) as e:
            reg.Iteration()
        assert e.value.code == nat.ERR_NONFINITE
        wide = st.copy()
        wide.sigma2 = 1e12                                        # every point within reach again
        inject(reg, wide)
        reg.Iteration()
        got, want = reg.state(), p.iterate(wide, "woodbury")
        # (the similarity step of this iteration is not comparable: see test_gpu_bcpd.py)
        assert np.isfinite(got["yhat"]).all() and np.isfinite(got["sigma2"]) and got["sigma2"] > 0 and got["s"] > 0
        for k, v in (("nu", want.nu), ("nu_prime", want.nu_prime), ("vhat", want.vhat), ("alpha", want.alpha)):
            assert br.rel(got[k], v) < 1e-9, (k, br.rel(got[k], v))
        assert np.abs(got["sigma_diag"] - want.sig).max() < 1e-9 * p.kmax
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------------------------ leaks
def test_handles_release_their_device_memory(ctx):
    y, x = inputs("hull", 1500, 1125)

    def cycle():
        reg = make(ctx, y, x, 25.0, 1e-8, 0)
        reg.Iteration()
        assert np.isfinite(reg.sigma2())
        reg.close()

    cycle()                                   # warm-up: code objects, allocator pools
    gc.collect()
    before = _free_bytes()
    for _ in range(15):
        cycle()
    gc.collect()
    after = _free_bytes()
    assert before - after < 64 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
