"""Host side of the posterior-solve variant tests (posterior_solve_cases.py): the guards of every family, the route table, the
self-check of the extended-precision reference against mpmath, the density restatement and the alpha map against the oracle, the
float64 figures the GPU bounds hang on, and the check that those bounds bite.  No GPU."""
import numpy as np
import pytest

from tests import posterior_solve_cases as pc
from oracle import gingr_oracle as go

pytestmark = pytest.mark.skipif(not pc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")


# ------------------------------------------------------------------------------------------------ route table
def test_route_table_names_every_instance_at_both_edges():
    for name, (select, first, last) in pc.EXPECTED.items():
        ranks = pc.EIG_RANKS if "eig" in name else pc.RANKS
        hit = [r for r in ranks if select(r) == name]
        assert first in hit and last in hit and len(hit) >= 2, (name, hit)
        assert min(hit) == first and max(hit) == last, (name, hit)  # the range the launcher gives, no rank outside it
    # each threshold has a rank on both sides
    for lo in (112, 128, 240, 256, 384):
        assert lo in pc.RANKS and lo + 1 in pc.RANKS
    for lo, hi in ((15, 17), (31, 33)):
        assert lo in pc.RANKS and hi in pc.RANKS and 16 in pc.RANKS
    named = {n.replace(" (sampled)", "") for n in pc.EXPECTED}
    assert len(named) + len(pc.UNREACHABLE) == 16  # every instance behind the four launchers (the dense routes and the eigen route included)


def test_three_block_solve_is_selected_by_use_compact_alone():
    """posterior_solve_lds_kernel<2>: a deterministic CPD or isotropic-pairs update of a single-shard separable model that keeps its
    compact basis (rp <= 112, at most 48 columns per coordinate), without landmarks and not behind a query -- and nothing else."""
    name = "posterior_solve_lds_kernel<2>"

    def route(r, counts, **kw):
        return pc.route_of(r, kw.get("sampled", False), compact=pc.uses_compact(r, counts, **kw))

    assert route(49, (48, 1, 0)) == name and route(96, (0, 48, 48)) == name and route(112, (48, 47, 17)) == name
    assert route(100, (34, 33, 33), flavour="pairs") == name
    assert pc.even_classes(112) == (38, 37, 37) and pc.even_classes(1) == (1, 0, 0) and pc.even_classes(113) == (38, 38, 37)
    dense = "posterior_solve_lds_kernel<0>"
    assert route(51, (49, 1, 1)) == dense          # a class past the plane's width
    assert route(30, None) == dense                 # not separable
    assert route(113, (38, 38, 37)) == "posterior_solve_lds_kernel<1>"  # rp = 128: no compact basis is kept
    for kw in ({"landmarks": True}, {"sampled": True}, {"query": True}, {"shards": 2}, {"device_group": True}, {"option": 0},
               {"flavour": "icp"}, {"flavour": "icp_surface"}, {"flavour": "pairs", "covariance_pairs": True}):
        assert route(100, (34, 33, 33), **kw) == dense, kw


def test_global_workspace_density_kernel_has_no_caller():
    for r in range(1, 513):
        for kind in ("sharded", "fresh", "cached"):
            assert pc.density_route_of(r, kind) not in pc.UNREACHABLE, (r, kind)


def test_sampled_solve_never_takes_the_dense_route():
    for r in pc.RANKS:
        assert pc.route_of(r, True) != "dense_spd_solve3"
        if pc.rp_of(r) > 256:
            assert pc.route_of(r, True) == "posterior_solve_wide_kernel<32>"


# ------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("r", [r for r in pc.RANKS if r <= 256 or r in pc.FULL_ABOVE_256])
def test_family_guards(r):
    G, _, _, _ = pc.make_case("well", r)
    assert np.array_equal(G, G.T)
    if r >= 2:
        assert 1e2 <= pc.cond_of(G) <= 2e3
        c = pc.cond_of(pc.make_case("ill", r)[0])
        assert 1e7 <= c <= 1e9, (r, c)
    for fam in ("graded_up", "graded_down"):
        G = pc.make_case(fam, r)[0]
        d = np.diag(G)
        assert np.array_equal(G, G.T) and np.all(np.linalg.eigvalsh(G) > 0)
        if r >= 2:
            assert (d[-1] / d[0] if fam == "graded_up" else d[0] / d[-1]) == pytest.approx(1e12, rel=1e-6)
    G = pc.make_case("diagonal", r)[0]
    assert np.count_nonzero(G - np.diag(np.diag(G))) == 0 and len(set(np.diag(G))) == r
    assert not pc.make_case("zero", r)[0].any()
    for fam in pc.BAD_FAMILIES:
        G = pc.make_case(fam, r)[0]
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(np.eye(r) + G)
        with pytest.raises(np.linalg.LinAlgError):
            pc.cholesky_left((np.eye(r) + G).astype(pc.LD))
    if r >= 2:  # the second copy fails at the last real column and nowhere before
        G = pc.make_case("notpd_last", r)[0]
        pc.cholesky_left((np.eye(r) + G)[:r - 1, :r - 1].astype(pc.LD))
        assert np.linalg.eigvalsh(np.eye(r) + pc.make_case("notpd", r)[0])[0] == pytest.approx(-0.5, rel=1e-9)


def test_model_guards():
    for r in (1, 2, 113, 512):
        ref, mean, U, lam = pc.model_parts(r)
        assert ref.shape[0] >= max(200, -(-r // 3) + 7) and ref.shape[0] % 2 == 1
        assert np.abs(U.T @ U - np.eye(r)).max() < 1e-13
        assert lam.min() >= 1e-1 and lam.max() <= 1e4
        if r >= 2:
            assert lam.min() == 1e-1 and lam.max() == 1e4


# ------------------------------------------------------------------------------------------------ reference self-check
@pytest.mark.parametrize("r", [1, 2, 15, 16, 17, 31, 33, 48])
@pytest.mark.parametrize("family", ["well", "ill", "graded_up", "graded_down", "diagonal"])
def test_reference_against_mpmath(family, r):
    """a and a + L^-T z of the longdouble reference against mpmath at 50 digits: within 100 r eps_longdouble cond(I + G)."""
    import mpmath as mp  # (part of the reference's self-check: a missing mpmath is a failure, not a skip)
    mp.mp.dps = 50
    G, rhs, z, _ = pc.make_case(family, min(r, 48))
    n = G.shape[0]
    N = mp.matrix(G.tolist()) + mp.eye(n)  # (the sum in mpmath: 1 + g is not a float64 in general)
    L = mp.cholesky(N)
    a = mp.lu_solve(N, mp.matrix(rhs.tolist()))
    x = mp.lu_solve(L.T, mp.matrix(z.tolist()))
    S = pc.stot_cached(n)
    out = pc.solve_all(G, rhs, z, S, pc.qte_of(S, pc.make_case(family, n)[3]), pc.LD)
    bound = 100.0 * n * float(np.finfo(pc.LD).eps) * pc.cond_of(G)

    def err(v_ld, v_mp):
        d = mp.matrix([mp.mpf(float(t)) + mp.mpf(float(t - pc.LD(float(t)))) for t in v_ld]) - v_mp
        return float(mp.norm(d) / mp.norm(v_mp))

    assert err(out["a"], a) <= bound, (family, n, err(out["a"], a), bound)
    assert err(out["s"], a + x) <= bound, (family, n, err(out["s"], a + x), bound)
    # the density: u = K^-1 (qte - S a), -u^T N u / 2 - n / 2 log(2 pi), all of it in mpmath from the same float64 inputs
    qte = pc.qte_of(S, pc.make_case(family, n)[3])
    Smp = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Smp[i, j] = mp.mpf(float(S[i, j])) + mp.mpf(float(S[i, j] - pc.LD(float(S[i, j]))))
    u = mp.lu_solve(Smp + mp.mpf(pc.EPS) * N, mp.matrix(qte.tolist()) - Smp * a)
    want = -(u.T * N * u)[0] / 2 - mp.mpf(n) / 2 * mp.log(2 * mp.pi)
    got = mp.mpf(float(out["logpdf"])) + mp.mpf(float(out["logpdf"] - pc.LD(float(out["logpdf"]))))
    condK = float(np.linalg.cond(np.asarray(S, dtype=np.float64) + pc.EPS * (np.eye(n) + G)))
    assert float(abs(got - want) / abs(want)) <= bound + 100.0 * n * float(np.finfo(pc.LD).eps) * condK, (family, n, float(got), float(want))


# ------------------------------------------------------------------------------------------------ restatements against the oracle
def _small_state(r=7, M=40, seed=3):
    rng = np.random.default_rng(seed)
    ref = rng.normal(0, 30, (M, 3))
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    lam = np.sort(10.0 ** rng.uniform(-1, 3, r))[::-1].copy()
    mo = go.PDM(ref=ref, mean=np.zeros((M, 3)), U=U, lam=lam)
    st = go.initial_state(mo, 50.0, global_transformation=go.NO_TRANSFORMS)
    pids = np.arange(M)
    pts = mo.instance(rng.normal(0, 1, r)) + rng.normal(0, 1.0, (M, 3))
    var = rng.uniform(0.5, 5.0, M)
    Q = U * np.sqrt(lam)[None, :]
    W3 = np.repeat(1.0 / var, 3)
    G = Q.T @ (W3[:, None] * Q)
    rhs = Q.T @ (W3 * (pts - ref).reshape(-1))
    return mo, st, pids, pts, var, Q, G, rhs, rng


def test_density_restatement_against_oracle():
    mo, st, pids, pts, var, Q, G, rhs, rng = _small_state()
    mesh = mo.instance(rng.normal(0, 1, mo.rank)) + rng.normal(0, 0.2, (mo.M, 3))
    want = go.posterior_logpdf_of_mesh(mo, st, pids, pts, var, mesh=mesh)
    qte = Q.T @ (mesh - mo.ref - mo.mean).reshape(-1)
    got = pc.solve_all(G, rhs, np.zeros(mo.rank), (Q.T @ Q).astype(pc.LD), qte, pc.LD)["logpdf"]
    assert abs(float(got) - want) <= 1e-9 * abs(want), (float(got), want)


@pytest.mark.parametrize("sampled", [False, True])
def test_alpha_map_against_oracle(sampled):
    mo, st, pids, pts, var, Q, G, rhs, rng = _small_state()
    z = rng.normal(0, 1, mo.rank) if sampled else None
    new = go.update_from_observations(mo, st, pids, pts, var, sigma2_next=1.0, z=z)
    assert new.status == 0
    out = pc.solve_all(G, rhs, z if sampled else np.zeros(mo.rank), (Q.T @ Q).astype(pc.LD), np.zeros(mo.rank), pc.LD)
    want = np.asarray(pc.alpha_map_ld(mo.lam) * (out["s"] if sampled else out["a"]), dtype=np.float64)
    assert np.linalg.norm(new.alpha - want) <= 1e-9 * np.linalg.norm(want)


# ------------------------------------------------------------------------------------------------ the figures the GPU bounds hang on
@pytest.fixture(scope="module")
def measured():
    return pc.measure_float64_figures()


def test_float64_figures(measured):
    """Prints the table (family x figure, maximum over the ranks) and holds the committed copy to it within a factor 2."""
    print()
    for fam in pc.FAMILIES:
        print(f'    "{fam}": {{' + ", ".join(f'"{k}": {measured[fam][k]:.2e}' for k in pc.FIGURE_NAMES) + "},")
    for fam in pc.FAMILIES:
        for k in pc.FIGURE_NAMES:
            got, have = measured[fam][k], pc.F64_FIGURES[fam][k]
            assert (got == 0.0 and have == 0.0) or 0.5 * have <= got <= 2.0 * have, (fam, k, got, have)


def test_bound_conditions():
    """The caps on the GPU bounds: if the float64 route alone breaks one, the family is wrong, not the cap."""
    for fam in pc.FAMILIES:
        for k in ("backward", "sample_backward"):
            if (fam, k) == ("ill", "sample_backward"):
                # The sample's figure is taken against a_ref, so it carries the forward error of a: u cond |a| in the directions where
                # L^T is O(1), over |L| |s - a_ref| = sqrt(cond) |s - a_ref|, i.e. u sqrt(cond).  With the guard's cond >= 1e7 that is
                # >= 3.5e-13 for ANY backward-stable float64 route, so 1000 x it cannot stay below 1e-10; the cap of this one entry is the
                # derived 1000 u sqrt(cond) instead.
                cond = pc.cond_of(pc.make_case("ill", 113)[0])
                assert 0.9e8 <= cond <= 1.1e8 and pc.gpu_bound(fam, k, 512) < 1000.0 * 2.0 ** -53 * np.sqrt(cond), (fam, k)
                continue
            assert pc.gpu_bound(fam, k, 512) < 1e-10, (fam, k)
    assert pc.gpu_bound("well", "forward", 512) < 1e-9 and pc.gpu_bound("well", "sample_forward", 512) < 1e-9


def _shift_one_pivot(L):
    """One pivot 1e-9 (relative) off: the largest one, which carries weight in every norm of the figures."""
    k = int(np.argmax(np.diag(L)))
    L[k, k] *= 1.0 + 1e-9
    return L


@pytest.mark.parametrize("r", [17, 113, 257])
@pytest.mark.parametrize("family", ["well", "ill", "graded_up", "graded_down"])
def test_bounds_bite(family, r):
    """A float64 route with one pivot shifted by 1e-9 must break the GPU bound of its family (host only)."""
    fig = pc.float64_route(family, r, damage=_shift_one_pivot)
    over = {k: v / pc.gpu_bound(family, k, r) for k, v in fig.items()}
    assert max(over.values()) > 1.0, (family, r, over)
    assert over["backward"] > 1.0 or over["sample_backward"] > 1.0, (family, r, over)


# ------------------------------------------------------------------------------------------------ family 6 and the read-back models
def test_eigen_family_guards():
    lam = pc.model_parts(512)[3]
    ratios = np.concatenate([lam / s2 for s2 in pc.EIG_SIGMA2])
    assert ratios.min() == pytest.approx(1e-3) and ratios.max() == pytest.approx(1e5)
    assert pc.EIG_MAX_RANK in pc.EIG_RANKS and pc.EIG_MAX_RANK + 1 in pc.EIG_RANKS  # both sides of eig_ready
    assert 128 in pc.EIG_RANKS and 129 in pc.EIG_RANKS
    for r in (5, 64):
        _, _, U, lam = pc.eig_model_parts(r, orthonormal=False)
        S = np.asarray(pc.stot_ld(U, lam), dtype=np.float64)
        d = np.sqrt(np.diag(S))
        off = np.abs(S / d[:, None] / d[None, :] - np.eye(r)).max()
        assert off > 1e-2, off  # S_tot is a full matrix
        for s2 in pc.EIG_SIGMA2:
            ref, f64 = pc.eig_reference(r, s2, orthonormal=False)
            assert f64["forward"] < 1e-13 and f64["backward"] < 1e-15
            # the map and its inverse are each other's: alpha = C C a_ref comes back to a_ref
            Sl = ref["S"]
            C = np.linalg.solve(np.asarray(Sl, dtype=np.float64) + pc.EPS * np.eye(r), np.asarray(Sl, dtype=np.float64))
            back = pc.undo_alpha_map(C @ (C @ np.asarray(ref["a"], dtype=np.float64)), Sl, lam, False)
            assert float(np.max(np.abs(back - ref["a"]) / np.abs(ref["a"]))) < 1e-9


def test_readback_model_guards():
    for r in pc.READBACK_RANKS:
        _, _, U, lam, target, mesh = pc.readback_model_parts(r)
        assert lam.min() >= 1e-3 and lam.max() <= 1e6 and (r < 2 or (lam.min() == 1e-3 and lam.max() == 1e6))
        assert target.shape == mesh.shape == (U.shape[0] // 3, 3)
    assert {16, 17, 112, 113, 128, 129, 256, 385} <= set(pc.READBACK_RANKS)
