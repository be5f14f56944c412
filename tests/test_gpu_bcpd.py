"""GPU tests of the Bayesian coherent point drift (gingr_amd/csrc/bcpd.hip, classic.BCPD) against the Woodbury route of its numpy
restatement (tests/bcpd_restatement.py): the initial state, single iterations from the restatement's own states (with rows whose
nu_m is zero), free runs, the stop rule, the wrapper, the refusals, and the bits of the benchmark's CPD kernels, which this feature
must not change.  Tolerances are those test_gpu_classic_cpd.py holds the non-rigid CPD to: 1e-9 relative for point sets and vectors,
1e-8 relative for variances, 1e-6 for whole registrations; sigma_m^2 is compared to 1e-9 max K_mm ABSOLUTE, so that rows with nu_m = 0
(where sigma_m^2 is largest) count in full."""
import functools
import os

import numpy as np
import pytest

from tests import bcpd_restatement as br

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bcpd_unchanged_cpd_kernels.npz")
STATES = (0, 1, 10, 40)


@functools.lru_cache(maxsize=None)
def case(name, w):
    """(problem, {iteration: state}) -- computed once, shared, never modified"""
    if name == "g6":
        y, x = br.grid_case(6)
    elif name == "g7":
        y, x = br.grid_case(7)
    elif name == "g7cut":
        y, x = br.grid_case(7, cut=True)
    elif name == "m65n1":
        rng = np.random.default_rng(65)
        y = rng.normal(0, 1.5, (65, 3))
        x = np.array([[0.3, -0.2, 0.1]])
    elif name == "m1n3":
        rng = np.random.default_rng(13)
        y = np.array([[0.2, 0.1, -0.3]])
        x = rng.normal(0, 1.0, (3, 3))
    else:
        raise KeyError(name)
    p = br.Problem(y, x, w=w, beta=1.5, **br.PARAMS)
    degenerate = name in ("m65n1", "m1n3")
    # one target point or one template point: S_xu is zero but for rounding, the rotation is undefined and s = 0 afterwards, so only
    # the iteration from the initial state exists
    states = {0: p.initial()} if degenerate else p.run(max(STATES), keep=STATES)
    return p, states


def make(ctx, p):
    from gingr_amd import classic as cl
    return cl.BCPD(ctx, p.y, p.x, w=p.w, lambda_=p.lam, gamma=p.gamma, k=p.kappa, beta=p.beta)


def inject(reg, st):
    reg.set_state(st.yhat, st.sig, st.alpha, st.s, st.R, st.t, st.sigma2)


def figures(got, want, p):
    """the deviation of every quantity of an iteration, on the scale `compare` holds it to"""
    kmax = float(np.diag(p.G).max() / p.lam)
    return dict(yhat=br.rel(got["yhat"], want.yhat), vhat=br.rel(got["vhat"], want.vhat), alpha=br.rel(got["alpha"], want.alpha),
                nu=br.rel(got["nu"], want.nu), nu_prime=br.rel(got["nu_prime"], want.nu_prime),
                sigma_diag=float(np.abs(got["sigma_diag"] - want.sig).max() / kmax),
                s=abs(got["s"] - want.s) / max(abs(want.s), 1e-300), R=float(np.abs(got["R"] - want.R).max()), t=br.rel(got["t"], want.t),
                sigma2=abs(got["sigma2"] - want.sigma2) / max(abs(want.sigma2), 1e-300), Nhat=abs(got["Nhat"] - want.Nhat) / want.Nhat,
                sigma_bar2=abs(got["sigma_bar2"] - want.sigma_bar2) / want.sigma_bar2)


def compare(got, want, p, degenerate=False, label=""):
    fig = figures(got, want, p)
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()), f"min_nu={want.nu.min():.2e}")
    for k in ("yhat", "alpha", "nu", "nu_prime", "sigma_diag", "t", "Nhat"):
        assert fig[k] < 1e-9, (label, k, fig[k])
    # v^ is compared on the scale of the shape it moves (u^ = y + v^ is the point set; v^ alone is a difference of two of them)
    assert br.rel(p.y + got["vhat"], p.y + want.vhat) < 1e-9, (label, "uhat")
    assert fig["vhat"] < 1e-9 and fig["sigma_bar2"] < 1e-8, (label, fig["vhat"], fig["sigma_bar2"])
    if degenerate:
        # S_xu is zero but for rounding: s = 0 on that scale, R is some rotation, and with one target point sigma2 itself is what
        # rounding leaves of xPx - 2 PX . y^ + nu |y^|^2, so it is held to the scale of the terms it is the difference of
        assert abs(got["s"] - want.s) < 1e-12 and abs(np.linalg.det(got["R"]) - 1.0) < 1e-12, (label, got["s"], want.s)
        scale = max(want.sigma2, float((p.x ** 2).sum(1).mean()) / 3.0)
        assert abs(got["sigma2"] - want.sigma2) < 1e-8 * scale, (label, got["sigma2"], want.sigma2)
    else:
        assert fig["sigma2"] < 1e-8 and fig["s"] < 1e-9 and fig["R"] < 1e-9, (label, fig["sigma2"], fig["s"], fig["R"])
    return fig


# ------------------------------------------------------------------------------------------------------- initial state
@pytest.mark.parametrize("name,w", [("g6", 0.1), ("g7cut", 0.0)])
def test_initial_state_and_first_iteration(ctx, name, w):
    p, states = case(name, w)
    reg = make(ctx, p)
    try:
        st0 = states[0]
        got = reg.state()
        assert abs(got["sigma2"] - st0.sigma2) < 1e-12 * st0.sigma2
        assert np.array_equal(got["yhat"], p.y) and np.array_equal(got["sigma_diag"], np.ones(p.M))
        assert np.array_equal(got["alpha"], np.full(p.M, 1.0 / p.M)) and got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3))
        reg.Iteration()
        got, want = reg.state(), states[1]
        nu, nup = reg.correspondenceWeights()
        assert np.array_equal(nu, got["nu"]) and np.array_equal(nup, got["nu_prime"])
        assert br.rel(nu, want.nu) < 1e-9 and br.rel(nup, want.nu_prime) < 1e-9
        xbar = want.PX.sum(0) / want.Nhat                       # t = xbar - s R ubar: xbar back from the device's own transform
        ubar = (got["nu"][:, None] * (p.y + got["vhat"])).sum(0) / got["Nhat"]
        assert br.rel(got["t"] + got["s"] * got["R"] @ ubar, xbar) < 1e-9
        compare(got, want, p, label=f"{name} w={w} first")
    finally:
        reg.close()


# --------------------------------------------------------------------------------------------------- single iterations
@pytest.mark.parametrize("name,w", [("g6", 0.1), ("g6", 0.0), ("g7", 0.1), ("g7", 0.0), ("g7cut", 0.1), ("g7cut", 0.0),
                                    ("m65n1", 0.0), ("m1n3", 0.1), ("m1n3", 0.0)])
def test_single_iterations_from_the_restatements_states(ctx, name, w):
    """g6: M = 216, N = 194 (no multiple of 64, one tile of the pair passes); g7: M = 343, N = 308 or 166 (past a 256 tile: two chunks,
    six Cholesky panels with padding); the states after 10 and 40 iterations of the full-overlap runs hold rows with nu_m = 0
    (g6, exactly) and 7e-10 (g7)."""
    p, states = case(name, w)
    degenerate = len(states) == 1
    reg = make(ctx, p)
    try:
        for it, st in sorted(states.items()):
            inject(reg, st)
            reg.Iteration()
            compare(reg.state(), p.iterate(st), p, degenerate, label=f"{name} w={w} from {it}")
    finally:
        reg.close()


def test_kappa_infinite_keeps_the_mixing_weights(ctx):
    y, x = br.grid_case(6)
    p = br.Problem(y, x, w=0.1, beta=1.5, lambda_=10.0, gamma=0.3, kappa=np.inf)
    reg = make(ctx, p)
    try:
        reg.Iteration()
        got = reg.state()
        assert np.array_equal(got["alpha"], np.full(p.M, 1.0 / p.M))
        compare(got, p.iterate(p.initial()), p, label="kappa=inf")
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------------------- free runs
@pytest.mark.parametrize("name", ["g6", "g7"])
def test_free_run_follows_the_restatement_and_repeats_its_bits(ctx, name):
    p, states = case(name, 0.1)
    want = states[40]
    reg = make(ctx, p)
    try:
        a = reg.Registration(40, tolerance=0.0)
        assert reg.iterations == 40 and not reg.converged
        sa = reg.state()
        print(name, "free run: yhat", br.rel(a, want.yhat), "s", abs(sa["s"] - want.s), "sigma2", abs(sa["sigma2"] - want.sigma2) / want.sigma2)
        assert br.rel(a, want.yhat) < 1e-6 and abs(sa["s"] - want.s) < 1e-6
        b = reg.Registration(40, tolerance=0.0)
        sb = reg.state()
        assert np.array_equal(a, b)
        for k in ("vhat", "sigma_diag", "alpha", "nu", "nu_prime", "R", "t"):
            assert np.array_equal(sa[k], sb[k]), k
        assert sa["s"] == sb["s"] and sa["sigma2"] == sb["sigma2"] and sa["sigma_bar2"] == sb["sigma_bar2"]
    finally:
        reg.close()


def test_stop_rule_stops_where_the_restatement_stops(ctx):
    p, _ = case("g6", 0.1)
    want, iterations, converged = p.registration(100, 1e-6)
    assert converged and 10 < iterations < 100
    reg = make(ctx, p)
    try:
        got = reg.Registration(100)                               # tolerance = 1e-6, the default
        assert reg.converged and reg.iterations == iterations
        assert br.rel(got, want.yhat) < 1e-6
    finally:
        reg.close()


def test_registration_wrapper_returns_what_the_class_returns(ctx):
    from gingr_amd import classic as cl
    p, _ = case("g6", 0.1)
    kw = dict(w=p.w, lambda_=p.lam, gamma=p.gamma, k=p.kappa, beta=p.beta)
    reg = cl.BCPD(ctx, p.y, p.x, **kw)
    try:
        a = reg.Registration(12)
    finally:
        reg.close()
    b = cl.BCPDRegistration(ctx, p.y, max_iterations=12, **kw).register(p.x)
    assert a.shape == (p.M, 3) and np.array_equal(a, b)
    d = cl.BCPDRegistration(ctx, p.y)
    assert (d.w, d.lambda_, d.gamma, d.k, d.beta, d.max_iterations) == (0, 2.0, 1.0, 1.0, 2.0, 100)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_create_refuses_bad_arguments(ctx):
    from gingr_amd import classic as cl, GingrNativeError
    from gingr_amd import _native as nat
    y, x = br.grid_case(3)
    good = dict(w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=1.5)
    flat = x.copy()
    flat[:, 2] = 0.25                                             # a target in a plane: its bounding box has no volume
    bad = [dict(w=-0.1), dict(w=1.0), dict(w=np.nan), dict(lambda_=0.0), dict(lambda_=-1.0), dict(gamma=0.0), dict(k=0.0), dict(k=-2.0),
           dict(beta=0.0), dict(beta=-1.5)]
    for change in bad:
        with pytest.raises(GingrNativeError) as e:
            cl.BCPD(ctx, y, x, **{**good, **change})
        assert e.value.code == nat.ERR_BAD_ARGUMENT and "bcpd_create" in str(e.value), change
    for yy, xx, kw in [(y[:0], x, good), (y, x[:0], good), (y, flat, good), (y, x[:1], good), (np.zeros((32769, 3)), x, good)]:
        with pytest.raises(GingrNativeError) as e:
            cl.BCPD(ctx, yy, xx, **kw)
        assert e.value.code == nat.ERR_BAD_ARGUMENT, (yy.shape, xx.shape)
    cl.BCPD(ctx, y, flat, **{**good, "w": 0.0}).close()           # without outliers the volume is not needed
    cl.BCPD(ctx, y, x, **{**good, "k": np.inf}).close()


def test_unreachable_target_point_reports_nonfinite_and_the_handle_survives(ctx):
    from gingr_amd import GingrNativeError
    from gingr_amd import _native as nat
    p, states = case("g6", 0.0)
    x = p.x.copy()
    x[17] += 1e6                                                  # w = 0: den_n + c = 0 for this point
    far = br.Problem(p.y, x, w=0.0, beta=1.5, **br.PARAMS)
    st = states[10]                                               # a state whose sigma2 is small against 1e6
    with np.errstate(all="ignore"):
        assert not np.isfinite(far.assignment(st)[1]).all()       # the restatement's nu' is NaN there too (0 / 0)
    reg = make(ctx, far)
    try:
        inject(reg, st)
        with pytest.raises(GingrNativeError) as e:
            reg.Iteration()
        assert e.value.code == nat.ERR_NONFINITE
        wide = st.copy()
        wide.sigma2 = 1e12                                        # every point within reach again
        inject(reg, wide)
        reg.Iteration()
        got, want = reg.state(), far.iterate(wide)
        # What this iteration is held to: the soft assignment and the deformation, at the usual bounds.  Its similarity step is not
        # comparable: at sigma2 = 1e12 every e_mn is 1 to twelve digits except towards the far point, S_xu is a rank-one matrix plus
        # 1e-12 of structure, and the rotation about its dominant direction is decided by that structure (in the restatement a
        # relative change of 1e-11 of yhat moves R by 1e-3).  R, s, t, yhat and sigma2 are checked for being finite and proper.
        assert np.isfinite(want.sigma2) and np.isfinite(got["yhat"]).all() and np.isfinite(got["sigma2"]) and got["sigma2"] > 0
        assert abs(np.linalg.det(got["R"]) - 1.0) < 1e-12 and np.isfinite(got["t"]).all() and got["s"] > 0
        for k, w in (("nu", want.nu), ("nu_prime", want.nu_prime), ("vhat", want.vhat), ("alpha", want.alpha)):
            assert br.rel(got[k], w) < 1e-9, (k, br.rel(got[k], w))
        assert np.abs(got["sigma_diag"] - want.sig).max() < 1e-9 * np.diag(far.G).max() / far.lam
        assert abs(got["Nhat"] - want.Nhat) < 1e-9 * want.Nhat and abs(got["sigma_bar2"] - want.sigma_bar2) < 1e-8 * want.sigma_bar2
    finally:
        reg.close()


# ------------------------------------------------------------------------------------- the benchmark's kernels: same bits
def unchanged_inputs():
    rng = np.random.default_rng(2024)
    Y = rng.normal(0, 10, (300, 3))
    X = 1.05 * Y[rng.permutation(300)[:257]] + np.array([0.5, -1.0, 0.25]) + rng.normal(0, 0.2, (257, 3))
    return Y, X


def unchanged_results(ctx):
    """what tests/golden/bcpd_unchanged_cpd_kernels.npz records (from a build of the commit before this feature)"""
    from gingr_amd import classic as cl
    Y, X = unchanged_inputs()
    out = {}
    st = ctx.cpd_stats(Y, X, 4.0, 0.1)
    for k in ("den", "P1", "PX", "Pt1"):
        out["stats_" + k] = st[k]
    out["stats_scalars"] = np.array([st["Np"], st["xPx"], st["trPXY"], st["yPy"], st["sigma2_next"], st["c"]])
    for kind, name in ((cl.RIGID, "rigid"), (cl.NONRIGID, "nonrigid")):
        reg = cl.RigidCPD(cl.CPDFactory(ctx, Y, lambda_=2.0, beta=6.0, w=0.1), X, kind)
        try:
            for _ in range(3):
                ty, s2 = reg.Iteration()
            out[name + "_ty"], out[name + "_sigma2"] = ty, np.array([s2])
        finally:
            reg.close()
    return out


def test_benchmark_cpd_kernels_keep_their_bits(ctx):
    want = np.load(GOLDEN)
    got = unchanged_results(ctx)
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert np.array_equal(want[k], got[k]), k
