"""GPU tests of the kernel warp (gingr_amd/csrc/kernel_warp.hip; gingr_classic_cpd_transform_points, gingr_bcpd_transform_points,
gingr_bcpd_get_coefficients; classic.RigidCPD.transformPoints, classic.BCPD.transformPoints / deformationCoefficients): the fitted
map of every kind of task at points off the template against the formula in np.longdouble with the device's own coefficients, under
the bound of tests/kernel_warp_restatement.py:

    |dev_p - ref_p|_inf <= |A|_inf [(2 M u + 4e-13) S_p + 8 u (|z_p|_inf + S_p)] + 16 u (|ref_p|_inf + |t|_inf),  S_p = max_d sum_m g_pm |c_md|

(2 M u: a sum of M terms in any fixed order; 4e-13: the exponential is within an ulp of that of an argument that carries 2 u relative
error and is at most 745 before the result is zero).  Every test prints the largest observed / bound ratio."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from tests import bcpd_restatement as br
from tests import kernel_warp_restatement as kw
from tests import lowrank_cpd_restatement as lr

pytestmark = pytest.mark.gpu

BETA, LAMBDA, W_OUTLIER = 6.0, 2.0, 0.05
BCPD_PARAMS = dict(w=0.1, lambda_=10.0, gamma=0.3, k=1.0)
MULTI_M = 3 * kw.CHUNK + 17                     # three whole chunks of centres and a fourth of 17
KINDS = ["rigid", "affine", "nonrigid", "nonrigid-lowrank", "bcpd", "bcpd-lowrank"]


@functools.lru_cache(maxsize=None)
def pair(M, N):
    y, x = lr.pair(M, N, 7 + M, noise=0.3)
    y.setflags(write=False)
    x.setflags(write=False)
    return y, x


def make(ctx, kind, y, x, beta=BETA, low_rank=None):
    from gingr_amd import classic as cl
    if kind.startswith("bcpd"):
        return cl.BCPD(ctx, y, x, beta=beta, lowRank=low_rank or (cl.LowRankG(1e-8) if kind.endswith("lowrank") else None), **BCPD_PARAMS)
    f = cl.CPDFactory(ctx, y, LAMBDA, beta, W_OUTLIER)
    if kind == "rigid":
        return f.registerRigidly(x)
    if kind == "affine":
        return f.registerAffine(x)
    return f.registerNonRigidly(x, low_rank or (cl.LowRankG(1e-8) if kind.endswith("lowrank") else None))


def iterate(reg, n):
    for _ in range(n):
        reg.Iteration()


def device_map(reg, kind):
    """(coefficients (M, 3) or an empty set of centres, A, t) as the device holds them"""
    if kind.startswith("bcpd"):
        s, R, t = reg.transform()
        return reg.template, reg.deformationCoefficients(), s * R, t
    if kind.startswith("nonrigid"):
        return reg.cpd.template, reg.W(), None, None
    s, B, t = reg.transform()
    return np.zeros((0, 3)), np.zeros((0, 3)), s * B, t


def check(reg, kind, Z, label):
    Y, C, A, t = device_map(reg, kind)
    beta = reg.beta if kind.startswith("bcpd") else reg.cpd.beta
    got = reg.transformPoints(Z)
    assert got.shape == Z.shape and np.isfinite(got).all(), label
    r = kw.ratio(got, Z, Y, C, beta, A, t)
    print(f"{label}: observed / bound = {r:.3f}")
    assert r <= 1.0, (label, r)
    return got


# ------------------------------------------------------------------------------------------------- 1  the pass alone, every kind
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_against_the_longdouble_formula(ctx, kind):
    y, x = pair(130, 110)
    reg = make(ctx, kind, y, x)
    try:
        iterate(reg, 3)
        got = check(reg, kind, kw.queries(300, y, 31), kind)
        assert np.abs(got - kw.queries(300, y, 31)).max() > 1e-3            # the map moves the points
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------- 2  tile and chunk edges
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_tile_edges_of_centres_and_queries(ctx, M):
    y, x = pair(M, 40 if M == 1 else 200)
    reg = make(ctx, "nonrigid", y, x)
    try:
        iterate(reg, 1)
        for P in (1, 255, 256, 257):
            check(reg, "nonrigid", kw.queries(P, y, 50 + P), f"M={M} P={P}")
    finally:
        reg.close()


@pytest.fixture(scope="module")
def multi(ctx):
    """the multi-chunk task: a low-rank non-rigid CPD of 3 chunks + 17 template points under 32 factor columns, one iteration"""
    from gingr_amd import classic as cl
    y, x = pair(MULTI_M, 500)
    reg = make(ctx, "nonrigid-lowrank", y, x, low_rank=cl.LowRankG(1e-8, 32))
    iterate(reg, 1)
    yield reg
    reg.close()


def test_chunk_edges(multi):
    assert kw.plan(257, MULTI_M)[0] == 4
    for P in (1, 255, 256, 257):
        check(multi, "nonrigid-lowrank", kw.queries(P, multi.cpd.template, 60 + P), f"M={MULTI_M} P={P}")


# ------------------------------------------------------------------------------------------------- 3  consistency at the template
def test_dense_nonrigid_map_of_the_template_is_ty(ctx):
    """One Maximization from the template: TY = Y + G W (one row of G against W, sixteen lanes) against z + sum_m g(z, y_m) W_m at
    z = y: the same kernel entries in two summation orders, hence twice the summation and exponential terms of the bound."""
    y, x = pair(257, 200)
    reg = make(ctx, "nonrigid", y, x)
    try:
        ty = reg.Iteration()[0]
        got, W = reg.transformPoints(y), reg.W()
        ref, S = kw.warp_reference(y, y, W, BETA)
        b = kw.bound(y, y.shape[0], S, ref, sum_factor=2.0)
        r = float((np.abs(got - ty).max(1) / b).max())
        print(f"T(Y) against TY: observed / bound = {r:.3f}; max |T(Y) - TY| = {np.abs(got - ty).max():.2e}")
        assert r <= 1.0
        assert kw.ratio(ty, y, y, W, BETA, sum_factor=2.0) <= 1.0 and kw.ratio(got, y, y, W, BETA) <= 1.0
    finally:
        reg.close()


def test_dense_bcpd_coefficients(ctx):
    """c of the device after one iteration from an injected state of the restatement: G c = v^ with the device's own v^, at most 16 x
    the restatement's residual (a different elimination order) with a floor at the bound of a float64 product G c; and c against the
    restatement's, at most max(16 delta_ref, the 1e-9 bar on v^ carried through c = (c2 / lambda) (r - nu o v^)) of max |c|."""
    y, x = br.grid_case(5)
    p = br.Problem(y, x, beta=1.5, w=BCPD_PARAMS["w"], **br.PARAMS)
    st = p.run(3, keep=(3,))[3]
    c_ref, cq_ref, vhat_ref, new = kw.bcpd_coefficients(p, st)
    res_ref = kw.coefficient_residual(p.G, c_ref, vhat_ref)
    delta_ref = float(np.abs(c_ref - cq_ref).max() / np.abs(c_ref).max())
    from gingr_amd import classic as cl
    reg = cl.BCPD(ctx, y, x, w=p.w, lambda_=p.lam, gamma=p.gamma, k=p.kappa, beta=p.beta)
    try:
        reg.set_state(st.yhat, st.sig, st.alpha, st.s, st.R, st.t, st.sigma2)
        reg.Iteration()
        c, vhat = reg.deformationCoefficients(), reg.state()["vhat"]
        res = kw.coefficient_residual(p.G, c, vhat)
        floor = float(((2.0 * p.M * kw.U + 4e-13) * (p.G @ np.abs(c)).max()) / np.abs(vhat).max())
        print(f"|G c - vhat| / max|vhat|: device {res:.2e}, restatement {res_ref:.2e}, floor {floor:.2e}")
        assert res <= max(16 * res_ref, floor)
        c2 = st.s ** 2 / st.sigma2
        carried = 1e-9 * (c2 / p.lam) * float(new.nu.max()) * float(np.abs(vhat_ref).max()) / float(np.abs(c_ref).max())
        dev = float(np.abs(c - c_ref).max() / np.abs(c_ref).max())
        print(f"c against the restatement: {dev:.2e} of max |c| (16 delta_ref = {16 * delta_ref:.2e}, carried bar {carried:.2e})")
        assert dev <= max(16 * delta_ref, carried)
        # and the map at the template is the shape the iteration left
        s, R, t = reg.transform()
        assert kw.ratio(reg.transformPoints(y), y, y, c, p.beta, s * R, t) <= 1.0
        assert br.rel(reg.transformPoints(y), reg.points()) < 1e-9
    finally:
        reg.close()


def test_lowrank_bcpd_coefficients(ctx):
    """The low-rank route: L L^T c = v^ with the device's factor, c and v^ -- with v^ off by e the residual is
    (I + (c2 / lambda) L L^T diag nu) e, so the 1e-9 bar on v^ is carried through that matrix (c2 = s^2 / sigma2 of the state that went
    into the iteration) -- and the map at the template against the shape the iteration left: T(y_m) - y^_m = s R ((G - L L^T) c)_m,
    the factor's residual row by row, plus the bound of the sum."""
    from gingr_amd import classic as cl
    y, x = pair(130, 110)
    reg = make(ctx, "bcpd-lowrank", y, x, low_rank=cl.LowRankG(1e-2))          # k < M: G - L L^T is not rounding alone
    try:
        iterate(reg, 2)
        before = reg.state()
        iterate(reg, 1)
        L, c, st = reg.factor(), reg.deformationCoefficients(), reg.state()
        assert 1 < L.shape[1] < y.shape[0]
        c2, lam = before["s"] ** 2 / before["sigma2"], BCPD_PARAMS["lambda_"]
        amp = float(np.abs(np.eye(y.shape[0]) + (c2 / lam) * (L @ L.T) * st["nu"][None, :]).sum(1).max())
        res = kw.coefficient_residual(L @ L.T, c, st["vhat"])
        print(f"|L L^T c - vhat| / max|vhat| = {res:.2e} (carried bar {1e-9 * amp:.2e}), {L.shape[1]} columns")
        assert res <= 1e-9 * amp
        A, t = st["s"] * st["R"], st["t"]
        got = reg.transformPoints(y)
        ref, S = kw.warp_reference(y, y, c, BETA, A, t)
        nA = float(np.abs(A).sum(1).max())
        gap = np.abs((kw.gauss(y, y, BETA) - L @ L.T) @ c).max(1) * nA
        # T(y_m) - y^_m = A ((G - L L^T) c)_m + A (L L^T c - v^)_m, each side computed within the bound of its own sum
        allowed = (gap + np.abs(L @ L.T @ c - st["vhat"]).max(1) * nA) * (1 + 1e-9) + 2 * kw.bound(y, y.shape[0], S, ref, A, t)
        err = np.abs(got - st["yhat"]).max(1)
        print(f"T(Y) against yhat: max {err.max():.2e}, the factor's share up to {gap.max():.2e}; observed / allowed = {(err / allowed).max():.3f}")
        assert (err <= allowed).all() and gap.max() > 1e3 * kw.bound(y, y.shape[0], S, ref, A, t).max()
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------- 4  a query is a pure function of the point
def test_a_query_does_not_depend_on_the_call(ctx, multi):
    from gingr_amd import classic as cl
    Z = kw.queries(700, multi.cpd.template, 71)
    all_at_once = multi.transformPoints(Z)
    for i in (0, 255, 256, 699):
        assert np.array_equal(multi.transformPoints(Z[i:i + 1])[0], all_at_once[i]), i
    assert np.array_equal(multi.transformPoints(Z), all_at_once)
    y, x = pair(MULTI_M, 500)
    other = make(ctx, "nonrigid-lowrank", y, x, low_rank=cl.LowRankG(1e-8, 32))
    try:
        iterate(other, 1)
        assert np.array_equal(other.transformPoints(Z), all_at_once)
    finally:
        other.close()
    buf = Z.copy()                                                           # out == in through the ABI
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert multi._lib.gingr_classic_cpd_transform_points(multi._h, 700, p, p) == 0
    assert np.array_equal(buf, all_at_once)


# ------------------------------------------------------------------------------------------------- 5  clamp and reach
def similarity_exact(Z, s, R, t):
    """s ((R0 x + R1 y) + R2 z) + t in the order of the device, one rounding per operation"""
    return np.stack([s * ((R[d, 0] * Z[:, 0] + R[d, 1] * Z[:, 1]) + R[d, 2] * Z[:, 2]) + t[d] for d in range(3)], 1)


@pytest.mark.parametrize("kind", ["nonrigid", "bcpd"])
def test_far_queries_come_back_as_the_head_alone(ctx, kind):
    rng = np.random.default_rng(5)
    y = rng.uniform(0.0, 1.0, (100, 3))
    x = y[rng.permutation(100)[:90]] + rng.normal(0, 0.01, (90, 3))
    reg = make(ctx, kind, y, x, beta=0.05)
    try:
        iterate(reg, 2)
        near = kw.queries(60, y, 6, margin=0.1)
        for far in (10.0, 1e9):             # 10: the exponential underflows unclamped; 1e9: the argument leaves the table's range, clamped
            Z = np.concatenate([near, np.array([[far, 0.5, 0.5], [0.5, -far, 0.5], [far, far, -far]])])
            got = check(reg, kind, Z, f"{kind} beta=0.05 with queries {far:g} away")
            want = Z[60:] if kind == "nonrigid" else similarity_exact(Z[60:], *reg.transform())
            assert np.array_equal(got[60:], want), (kind, far)
        assert np.abs(got[:60] - (near if kind == "nonrigid" else similarity_exact(near, *reg.transform()))).max() > 1e-6   # near ones do move
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------- 6  state rule and arguments
@pytest.mark.parametrize("kind", ["rigid", "nonrigid", "bcpd"])
def test_state_rule_and_arguments(ctx, kind):
    from gingr_amd import _native as nat
    y, x = pair(130, 110)
    Z = kw.queries(5, y, 9)
    reg = make(ctx, kind, y, x)
    entry = reg._lib.gingr_bcpd_transform_points if kind == "bcpd" else reg._lib.gingr_classic_cpd_transform_points

    def refused(call, code):
        with pytest.raises(nat.GingrNativeError) as e:
            call()
        assert e.value.code == code, (kind, e.value.code)

    try:
        refused(lambda: reg.transformPoints(Z), nat.ERR_STATE)                 # before the first iteration
        assert entry(reg._h, 0, None, None) == 0                                # ... where P = 0 succeeds all the same
        if kind == "bcpd":
            refused(reg.deformationCoefficients, nat.ERR_STATE)
        iterate(reg, 1)
        first = reg.transformPoints(Z)
        if kind == "bcpd":
            reg.set_state(sigma2=reg.sigma2())
        else:
            reg.set_state(*reg.state())
        refused(lambda: reg.transformPoints(Z), nat.ERR_STATE)                 # after set_state with no iteration since
        if kind == "bcpd":
            refused(reg.deformationCoefficients, nat.ERR_STATE)
        iterate(reg, 1)
        assert reg.transformPoints(Z).shape == (5, 3) and not np.array_equal(reg.transformPoints(Z), first)
        if kind == "bcpd":
            assert reg.deformationCoefficients().shape == (130, 3)
        assert reg.transformPoints(np.zeros((0, 3))).shape == (0, 3)            # P = 0
        assert entry(reg._h, 0, None, None) == 0
        out = np.empty_like(Z)
        po, pz = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for a in (out, Z))
        assert entry(reg._h, -1, pz, po) == nat.ERR_BAD_ARGUMENT
        assert entry(reg._h, 5, None, po) == nat.ERR_BAD_ARGUMENT and entry(reg._h, 5, pz, None) == nat.ERR_BAD_ARGUMENT
        if kind == "bcpd":
            assert reg._lib.gingr_bcpd_get_coefficients(reg._h, None) == nat.ERR_BAD_ARGUMENT
        with pytest.raises(ValueError):
            reg.transformPoints(np.zeros((4, 2)))
    finally:
        reg.close()


def test_a_failed_iteration_leaves_no_map(ctx):
    """w = 0 and a target point out of reach of every template point: the iteration reports GINGR_ERR_NONFINITE (the flag path of
    test_gpu_bcpd.py), the entries GINGR_ERR_STATE until an iteration succeeds again"""
    from gingr_amd import _native as nat
    from gingr_amd import classic as cl
    y, x = br.grid_case(5)
    far = x.copy()
    far[17] += 1e6
    Z = kw.queries(5, y, 9)
    reg = cl.BCPD(ctx, y, far, beta=1.5, **{**BCPD_PARAMS, "w": 0.0})
    try:
        reg.Iteration()                                                        # from the wide initial variance: every point in reach
        assert reg.transformPoints(Z).shape == (5, 3)
        reg.set_state(sigma2=1e-3)
        with pytest.raises(nat.GingrNativeError) as e:
            reg.Iteration()
        assert e.value.code == nat.ERR_NONFINITE
        for call in (lambda: reg.transformPoints(Z), reg.deformationCoefficients):
            with pytest.raises(nat.GingrNativeError) as e:
                call()
            assert e.value.code == nat.ERR_STATE
        reg.reset()
        reg.Iteration()
        assert np.isfinite(reg.transformPoints(Z)).all()
    finally:
        reg.close()


@pytest.mark.parametrize("kind", ["rigid", "nonrigid", "bcpd"])
def test_register_with_points(ctx, kind):
    from gingr_amd import classic as cl
    y, x = pair(130, 110)
    Z = kw.queries(40, y, 10)
    if kind == "bcpd":
        wrapper = cl.BCPDRegistration(ctx, y, beta=BETA, max_iterations=4, **BCPD_PARAMS)
    else:
        wrapper = (cl.RigidCPDRegistration if kind == "rigid" else cl.NonRigidCPDRegistration)(ctx, y, LAMBDA, BETA, W_OUTLIER, max_iterations=4)
    reg = make(ctx, kind, y, x)
    try:
        want = reg.Registration(4)
        plain = wrapper.register(x)
        assert isinstance(plain, np.ndarray) and np.array_equal(plain, want)    # as before
        warped, moved = wrapper.register(x, Z)
        assert np.array_equal(warped, want) and np.array_equal(moved, reg.transformPoints(Z))
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------- 7  no leaks
def _free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


LEAK_BIG_P, LEAK_CYCLES = 1 << 20, 3


def test_transform_points_releases_its_device_memory(ctx):
    """20 calls at P = 5 000 on one handle, then destroy; and, so that what the pass holds is far above what the figure can resolve,
    LEAK_CYCLES times create / 20 calls at P = 2^20 / destroy for both handle types.  The allowance is half of ONE handle's warp
    workspace at that size (72 MiB: the staging buffer, the planes, the partials): a handle that kept its buffers would show
    2 LEAK_CYCLES workspaces = 12 x the allowance, a buffer allocated anew on every call 240 x."""
    y, x = pair(257, 200)
    small, big = kw.queries(5000, y, 12), kw.queries(LEAK_BIG_P, y, 13)
    chunks, slab, _ = kw.plan(LEAK_BIG_P, y.shape[0])
    workspace = 8 * (chunks * 3 * slab + 2 * 3 * slab)
    assert workspace > 64 << 20

    def cycle(Z, calls):
        for kind in ("nonrigid", "bcpd"):
            reg = make(ctx, kind, y, x)
            iterate(reg, 1)
            for _ in range(calls):
                assert reg.transformPoints(Z).shape == Z.shape
            reg.close()

    cycle(big, 1)                             # warm-up: code objects, allocator pools
    gc.collect()
    before = _free_bytes()
    cycle(small, 20)
    for _ in range(LEAK_CYCLES):
        cycle(big, 20)
    gc.collect()
    after = _free_bytes()
    print(f"free device memory: {before - after} bytes fewer than at the start; allowance {workspace // 2} (one workspace: {workspace})")
    assert before - after < workspace // 2, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
