"""CPU side of the kernel warp (gingr_amd/csrc/kernel_warp.hip): its numpy restatement (tests/kernel_warp_restatement.py) against the
formula in np.longdouble under the bound every device result is held to; the coefficients of the Bayesian CPD, c with v^ = G c, on
the states of tests/bcpd_restatement.py; the non-rigid CPD's TY = Y + G W as the warp of the template; the planner
(gingr_amd/csrc/kernel_warp_plan.h), compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone
driver (tests/c/kernel_warp_plan_driver.cpp); and the three entries in the header and the loader."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import bcpd_restatement as br
from tests import kernel_warp_restatement as kw
from tests import lowrank_cpd_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_classic_cpd_transform_points", "gingr_bcpd_transform_points", "gingr_bcpd_get_coefficients"]
EDGE_M = [1, 255, 256, 257, 3 * kw.CHUNK + 17]


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("M", EDGE_M)
@pytest.mark.parametrize("P", [1, 300])
def test_blocked_float64_warp_stays_inside_the_bound(M, P):
    Y, C = kw.centres(M, 100 + M)
    Z = kw.queries(P, Y, 7 + P)
    R = go.euler_to_rot(0.3, -0.2, 0.5)
    worst = {}
    for name, beta, A, t in [("identity", 1.0, None, None), ("similarity", 2.5, 1.3 * R, np.array([3.0, -4.0, 5.0]))]:
        worst[name] = kw.ratio(kw.warp_blocked(Z, Y, C, beta, A, t), Z, Y, C, beta, A, t)
    print(f"M={M} P={P} observed / bound: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_bound_refuses_a_wrong_result():
    """the bound is tight enough to see one chunk's partial left out, or one centre of 6 161"""
    Y, C = kw.centres(3 * kw.CHUNK + 17, 5)
    Z = kw.queries(40, Y, 6)
    assert kw.ratio(Z + kw.gauss(Z, Y[kw.CHUNK:], 1.0) @ C[kw.CHUNK:], Z, Y, C, 1.0) > 1e3
    near, rest = Y[-2:-1] + 0.01, np.arange(Y.shape[0]) != Y.shape[0] - 2  # a query next to a centre of the last chunk, that centre left out
    assert np.abs(C[-2]).min() > 0 and kw.ratio(near + kw.gauss(near, Y[rest], 1.0) @ C[rest], near, Y, C, 1.0) > 1e3


# --------------------------------------------------------------------------------------------- BCPD: the coefficients
def bcpd_states():
    y, x = br.grid_case(5)
    p = br.Problem(y, x, w=0.1, beta=1.5, **br.PARAMS)
    yield "grid", p, p.run(3, keep=(3,))[3]
    y, x = br.cloud_case(200, 180, 3)
    p = br.Problem(y, x, w=0.1, beta=1.5, **br.PARAMS)
    yield "cloud", p, br.crafted_state(p, 4)


def test_bcpd_coefficients_reproduce_the_deformation():
    """G c = v^ on both routes.  With v^ off by e the residual is (I + (c2 / lambda) G diag nu) e, so the bar on v^ of the BCPD tests
    (1e-9) is carried through that matrix; the two forms of c (through nu o v^ and through d^1/2 o q) differ by the error of the
    solves with A = I + D^1/2 K D^1/2, 8 cond(A) u each on the scale of nu o v^."""
    for name, p, st in bcpd_states():
        for route in ("woodbury", "literal"):
            c, cq, vhat, new = kw.bcpd_coefficients(p, st, route)
            c2 = st.s ** 2 / st.sigma2
            amp = float(np.abs(np.eye(p.M) + (c2 / p.lam) * p.G * new.nu[None, :]).sum(1).max())
            res = kw.coefficient_residual(p.G, c, vhat)
            print(f"{name} {route}: |G c - vhat| / max|vhat| = {res:.2e} (carried bar {1e-9 * amp:.2e})")
            assert res <= 1e-9 * amp, (name, route, res)
            if cq is not None:
                dh = np.sqrt(c2 * new.nu)
                condA = np.linalg.cond(np.eye(p.M) + dh[:, None] * (p.G / p.lam) * dh[None, :])
                delta = float(np.abs(c - cq).max() / np.abs(c).max())
                allowed = 16 * condA * kw.U * (c2 / p.lam) * float(np.abs(new.nu[:, None] * vhat).max()) / float(np.abs(c).max())
                print(f"{name}: spread of the two forms of c, delta_ref = {delta:.2e} (allowed {allowed:.2e})")
                assert delta <= allowed, (name, delta, allowed)


def test_bcpd_coefficients_are_the_gp_regression_weights():
    """g(z, Y) c = g(z, Y) G^-1 v^ where G can be inverted: a jittered 3 x 4 x 5 grid of spacing 1 with beta = 0.6"""
    rng = np.random.default_rng(11)
    y = np.stack(np.meshgrid(np.arange(3.0), np.arange(4.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 3) + rng.normal(0, 0.1, (60, 3))
    x = 1.05 * (y + 0.2 * np.sin(0.9 * y[:, (1, 2, 0)])) @ go.euler_to_rot(0.1, -0.1, 0.2).T + rng.normal(0, 0.02, (60, 3))
    p = br.Problem(y, x, w=0.1, beta=0.6, **br.PARAMS)
    cond = np.linalg.cond(p.G)
    assert cond < 1e3
    c, _, vhat, _ = kw.bcpd_coefficients(p, p.run(3, keep=(3,))[3])
    gz = kw.gauss(kw.queries(200, y, 12), y, 0.6)
    want = gz @ np.linalg.solve(p.G, vhat)
    # c - G^-1 v^ = G^-1 (G c - v^), and numpy's solve is good to a few cond(G) u
    allowed = float(np.abs(gz).sum(1).max()) * (float(np.abs(np.linalg.inv(p.G)).sum(1).max()) * float(np.abs(p.G @ c - vhat).max())
                                                + 16 * cond * kw.U * float(np.abs(np.linalg.solve(p.G, vhat)).max()))
    err = float(np.abs(gz @ c - want).max())
    print(f"cond(G) = {cond:.1f}: |g c - g G^-1 vhat| = {err:.2e}, allowed {allowed:.2e}, max |g G^-1 vhat| = {np.abs(want).max():.2e}")
    assert err <= allowed and allowed < 1e-9 * np.abs(want).max()


# --------------------------------------------------------------------------------------------- non-rigid CPD: TY = T(Y)
def test_nonrigid_step_is_the_warp_of_the_template():
    Y, X = lr.pair(130, 110, 137, noise=0.3)
    beta, lam = 6.0, 2.0
    G = kw.gauss(Y, Y, beta)
    s2 = go.classic_cpd_initial_sigma2(Y, X)
    TY, _, W = go.classic_cpd_maximization_nonrigid(X, Y, go.classic_cpd_expectation(X, Y, s2, 0.05), s2, G, lam)
    r = kw.ratio(TY, Y, Y, W, beta, sum_factor=2.0)
    got = kw.warp_blocked(Y, Y, W, beta)
    print(f"oracle TY against the longdouble warp: observed / bound = {r:.3f}; restatement against TY: {np.abs(got - TY).max():.2e}")
    assert r <= 1.0 and kw.ratio(got, Y, Y, W, beta) <= 1.0


# ---------------------------------------------------------------------------------------------------------- the planner
PLAN_P = [1, 255, 256, 257, 300, 700, 5000, 10 ** 6]
PLAN_M = [0, 1, 255, 256, 257, kw.CHUNK - 1, kw.CHUNK, kw.CHUNK + 1, 3 * kw.CHUNK + 17, 10 ** 5, 5 * 10 ** 7]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("kernel_warp_plan") / "kernel_warp_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "kernel_warp_plan_driver.cpp"),
                           "-o", str(exe)])
    cases = [(P, M) for P in PLAN_P for M in PLAN_M]
    rows = np.ascontiguousarray(cases, dtype=np.int64)
    flat = np.frombuffer(subprocess.run([str(exe)], input=rows.tobytes(), capture_output=True, check=True).stdout, dtype=np.int64)
    out, at = {}, 0
    for case in cases:
        head = [int(v) for v in flat[at:at + 8]]
        chunks, slabs = head[0], head[3]
        ch = flat[at + 8:at + 8 + 2 * chunks].reshape(chunks, 2)
        sl = flat[at + 8 + 2 * chunks:at + 8 + 2 * chunks + 3 * slabs].reshape(slabs, 3)
        out[case] = (head, ch, sl)
        at += 8 + 2 * chunks + 3 * slabs
    assert at == flat.size
    return out


def test_chunks_tile_the_padded_centres_and_do_not_depend_on_p(plans):
    for (P, M), (head, ch, _) in plans.items():
        chunks, length = head[0], head[1]
        assert length == kw.CHUNK and length % kw.TILE == 0 and chunks == -(-M // length) == head[7], (P, M)
        assert (chunks - 1) * length < M <= chunks * length or M == 0, (P, M)                  # the padded centres; no chunk is empty
        assert [int(v) for v in ch[:, 0]] == [c * length for c in range(chunks)], (P, M)
        assert [int(v) for v in ch[:, 1]] == [min(M, (c + 1) * length) for c in range(chunks)], (P, M)
        assert np.array_equal(ch, plans[(1, M)][1]), (P, M)                                    # a function of M alone
        assert (chunks, head[2], head[3]) == kw.plan(P, M), (P, M)                             # the restatement's planner is this one


def test_slabs_tile_the_queries(plans):
    for (P, M), (head, _, sl) in plans.items():
        slab, slabs = head[2], head[3]
        assert slabs >= 1 and int(sl[:, 1].sum()) == P and int(sl[:, 1].min()) >= 1, (P, M)
        assert [int(v) for v in sl[:, 0]] == [s * slab for s in range(slabs)], (P, M)
        assert all(int(n) == slab for n in sl[:-1, 1]) and int(sl[-1, 1]) <= slab, (P, M)
        assert slabs == 1 or slab % kw.TILE == 0, (P, M)                                       # whole tiles unless one slab takes all
        assert all(int(g) == -(-int(n) // kw.TILE) for _, n, g in sl) and int(sl[:, 2].max()) <= kw.MAX_SLAB // kw.TILE, (P, M)


def test_workspace_sizes_are_bounded(plans):
    for (P, M), (head, _, _) in plans.items():
        chunks, _, slab, _, partial, cloud, ws, grid_y = head
        assert partial == chunks * 3 * slab and cloud == 3 * slab and ws == 8 * (partial + 2 * cloud), (P, M)
        assert slab <= kw.MAX_SLAB and grid_y <= 65535, (P, M)
        assert partial <= max(kw.MAX_PARTIAL_DOUBLES, chunks * 3 * kw.TILE), (P, M)           # 128 MiB, or one tile of queries
    assert plans[(10 ** 6, 10 ** 5)][0][3] > 1 and plans[(10 ** 6, 10 ** 5)][0][6] <= (128 << 20) + 2 * 24 * kw.MAX_SLAB
    assert plans[(700, 5 * 10 ** 7)][0][2] == kw.TILE and plans[(700, 5 * 10 ** 7)][0][3] == 3


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert _native.SIGNATURES["gingr_bcpd_transform_points"] == _native.SIGNATURES["gingr_classic_cpd_transform_points"]
    from gingr_amd import classic as cl
    assert all(hasattr(cl.RigidCPD, n) for n in ("transformPoints",)) and all(hasattr(cl.BCPD, n) for n in ("transformPoints", "deformationCoefficients"))
