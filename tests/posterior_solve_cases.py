"""Cases, dispatch restatement and extended-precision reference for the r x r posterior algebra of gingr_amd/csrc/gp.hip:
a = (I + G)^-1 rhs, the sampled proposal a + L^-T z and the log transition density.  Plain module, imported by
test_posterior_solve_host.py (CPU) and test_gpu_posterior_solve_variants.py (GPU).

Attribution.  The library has no per-variant launch counter, so WHICH kernel instance a rank exercises rests on the restatement of
the launchers' predicates below (route_of / density_route_of: launch_posterior_solve, launch_posterior_logpdf, fitter_logpdf_finish's
`rp >= 128 -> sync`, and the two single-shard callers in fitter_mh.hip).  EXPECTED names every instance with the two ranks of RANKS
on the edges of its range; the host test asserts the table, so a moved threshold fails there instead of silently testing another
branch (the device of regime_of in test_gpu_cpd_pair_pass_variants.py).

posterior_logpdf_lds_kernel<true> (rp > 112 without the hand-over words) is selected by no caller: the row-shard entry passes the
words from rp = 128 on and the single-shard entries always do.  The table records it as unreachable and asserts that.

Reference.  np.longdouble (64-bit mantissa): left-looking Cholesky, column at a time; a; L^-T z; the density restated from
oracle.gingr_oracle.posterior_logpdf_of_mesh in terms of (G, rhs, S_tot, qte):
    posterior model  Qp = Q0 Nn,  Nn Nn^T = (I + G)^-1;   coefficients(mesh) c = (Qp^T Qp + eps I)^-1 Qp^T d,  d = e - Q0 a
    Qp^T Qp = Nn^T S_tot Nn,  Qp^T d = Nn^T (qte - S_tot a) = Nn^T b
    =>  c = Nn^-1 K^-1 b,  K = S_tot + eps (I + G),   |c|^2 = u^T (I + G) u,  u = K^-1 b,   logpdf = -|c|^2 / 2 - r / 2 log(2 pi)
(K u = b  <=>  K (u + a) = qte + eps rhs: the second system of gp.hip.)

Alpha map.  The solve's a is not exported; the committed alpha is.  With NoTransforms, step length 1, the zero state and orthonormal
basis columns the post-solve map is the ridge projection twice, alpha_k = (lam_k / (lam_k + eps))^2 a_k (confirmed against
oracle.update_from_observations by the host test); outputs are taken back to a through the same map in extended precision.
"""
import functools
import math

import numpy as np

LD = np.longdouble
EPS = 1e-5  # GINGR_COEFF_NOISE
LOG_2PI = np.log(LD(2) * np.arccos(LD(-1)))

RANKS = [1, 2, 15, 16, 17, 31, 33, 96, 111, 112, 113, 127, 128, 129, 143, 144, 145, 239, 240, 241, 255, 256, 257, 272, 383, 384, 385,
         400, 497, 511, 512]
EIG_RANKS = [1, 5, 64, 128, 129, 192, 193, 300, 512]
# all families at these; above 256 the others carry family 1 and the closed forms only (time of the extended-precision reference)
FULL_ABOVE_256 = (257, 384, 385, 512)


EIG_MAX_RANK = 192  # kSymEigColsMaxN (gp.h)


def rp_of(r):
    return (r + 15) // 16 * 16


def have_extended():
    return np.finfo(LD).eps < 2e-19


# ------------------------------------------------------------------------------------------------ dispatch restatement
COMPACT_COLS = 48  # kCompactCols (gp.h)


def keeps_compact_basis(r, class_counts, shards=1):
    """model_detect_separable: a separable model (class_counts: columns per coordinate, None when some column has no class) keeps
    its compact basis on one shard, at the ranks of the triangle kernel, with every class inside a plane's width."""
    return class_counts is not None and shards == 1 and rp_of(r) <= 112 and max(class_counts) <= COMPACT_COLS


def uses_compact(r, class_counts, flavour="cpd", sampled=False, landmarks=False, covariance_pairs=False, query=False, shards=1,
                 device_group=False, option=-1):
    """use_compact (fitter_phases.hip): flavour 'cpd', 'pairs', 'icp' or 'icp_surface'; query: a log-density, covariance or
    posterior-model query, or a Metropolis-Hastings step (allow_alt); option: GINGR_OPT_SEPARABLE."""
    if not keeps_compact_basis(r, class_counts, shards) or option == 0 or device_group:
        return False
    if not (flavour == "cpd" or (flavour == "pairs" and not covariance_pairs)):
        return False
    return not landmarks and not sampled and not query


def even_classes(r):
    return tuple((r + 2 - d) // 3 for d in range(3))


def route_of(r, sampled, factor_cached=False, eig=False, compact=False):
    """launch_posterior_solve / phase2_solve_and_commit.  eig: point-cloud ICP without landmarks, deterministic.  compact: uses_compact
    of the update (never together with eig, sampled or factor_cached: those are flavours and callers it excludes)."""
    rp = rp_of(r)
    if eig and not sampled and r <= EIG_MAX_RANK:  # (eig_ready: model.hip decomposes S_tot only up to kSymEigColsMaxN columns)
        return "posterior_solve_eig_kernel"
    if sampled and factor_cached:  # nf_valid: only the split density kernel (rp <= 112, through gingr_fitter_mh_step) leaves the factor
        assert rp <= 112
        return "posterior_sample_cached_kernel"
    if compact:
        assert rp <= 112 and not sampled
        return "posterior_solve_lds_kernel<2>"
    if rp > 240 and not sampled:
        return "dense_spd_solve3"
    if r <= 128:
        return "posterior_solve_lds_kernel<0>" if rp <= 112 else "posterior_solve_lds_kernel<1>"
    return "posterior_solve_wide_kernel<64>" if rp <= 256 else "posterior_solve_wide_kernel<32>"


def density_route_of(r, route_kind):
    """launch_posterior_logpdf.  route_kind: 'sharded' (fitter_logpdf_finish: fx and sync only from rp = 128 on), 'fresh' (the
    single-shard callers fitter_mh.hip:117/260: fx and sync always), 'cached' (fx_valid of the live memo slot: set by a fresh query
    ONLY when the posterior memo holds this state, post_stage == 2 -- a state the host set with gingr_fitter_set_state or one a
    Metropolis-Hastings step tagged; otherwise the next query is fresh again)."""
    rp = rp_of(r)
    in_lds = rp <= 112
    if route_kind == "cached":
        return "posterior_logpdf_cached_kernel<false>" if in_lds else "posterior_logpdf_cached_kernel<true>"
    has_sync = True if route_kind == "fresh" else rp >= 128
    assert route_kind in ("fresh", "sharded")
    if in_lds and has_sync:
        return "posterior_logpdf_split_kernel"
    if rp > 384 and has_sync:
        return "dense_spd_solve3 x2 + logpdf_finish_kernel"
    if not in_lds and has_sync:
        return "posterior_logpdf_wide_kernel<64>" if rp <= 256 else "posterior_logpdf_wide_kernel<32>"
    return "posterior_logpdf_lds_kernel<false>" if in_lds else "posterior_logpdf_lds_kernel<true>"


# instance -> (selector, first rank, last rank) of RANKS (EIG_RANKS for the eigen route) that must select it
EXPECTED = {
    "posterior_solve_lds_kernel<0>": (lambda r: route_of(r, False), 1, 112),
    "posterior_solve_lds_kernel<1>": (lambda r: route_of(r, False), 113, 128),
    # a separable model with its columns dealt evenly to the coordinates (a Gaussian kernel's): CPD or isotropic pairs, nothing excluded
    "posterior_solve_lds_kernel<2>": (lambda r: route_of(r, False, compact=uses_compact(r, even_classes(r))), 1, 112),
    "posterior_solve_wide_kernel<64>": (lambda r: route_of(r, False), 129, 240),
    "posterior_solve_wide_kernel<64> (sampled)": (lambda r: route_of(r, True) + " (sampled)", 129, 256),
    "posterior_solve_wide_kernel<32> (sampled)": (lambda r: route_of(r, True) + " (sampled)", 257, 512),
    "dense_spd_solve3": (lambda r: route_of(r, False), 241, 512),
    "posterior_solve_eig_kernel": (lambda r: route_of(r, False, eig=True), 1, 192),
    "posterior_sample_cached_kernel": (lambda r: route_of(r, True, factor_cached=rp_of(r) <= 112), 1, 112),
    "posterior_logpdf_split_kernel": (lambda r: density_route_of(r, "fresh"), 1, 112),
    "posterior_logpdf_lds_kernel<false>": (lambda r: density_route_of(r, "sharded"), 1, 112),
    "posterior_logpdf_wide_kernel<64>": (lambda r: density_route_of(r, "sharded"), 113, 256),
    "posterior_logpdf_wide_kernel<32>": (lambda r: density_route_of(r, "sharded"), 257, 384),
    "dense_spd_solve3 x2 + logpdf_finish_kernel": (lambda r: density_route_of(r, "sharded"), 385, 512),
    "posterior_logpdf_cached_kernel<false>": (lambda r: density_route_of(r, "cached"), 1, 112),
    "posterior_logpdf_cached_kernel<true>": (lambda r: density_route_of(r, "cached"), 113, 512),
}
UNREACHABLE = ("posterior_logpdf_lds_kernel<true>",)
# EXPECTED restates the dispatch; it says nothing about coverage (test_gpu_posterior_solve_variants.py lists what reaches what).


# ------------------------------------------------------------------------------------------------ model
def model_parts(r):
    """(ref, mean, U, lam): M = max(200, ceil(r / 3) + 7) + 1 points (off every step length), U from a QR, lam log-uniform in
    [1e-1, 1e4] with both ends present from rank 2 on."""
    rng = np.random.default_rng(1000 + r)
    M = max(200, -(-r // 3) + 7) + 1
    ref = rng.normal(0, 30, (M, 3))
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    lam = 10.0 ** rng.uniform(-1, 4, r)
    if r >= 2:
        lam[rng.integers(r)] = 1e-1
        lam[(np.argmin(lam) + 1 + rng.integers(r - 1)) % r] = 1e4
    lam = np.sort(lam)[::-1].copy()
    return ref, np.zeros((M, 3)), np.ascontiguousarray(U), lam


def stot_ld(U, lam):
    """S_tot = Q0^T Q0 of the uploaded basis Q0 = U sqrt(lam) (float64, as uploaded), the product in extended precision."""
    Q = (U * np.sqrt(lam)[None, :]).astype(LD)
    return Q.T @ Q


def alpha_map_ld(lam):
    c = lam.astype(LD) / (lam.astype(LD) + LD(EPS))
    return c * c


# ------------------------------------------------------------------------------------------------ families
FAMILIES = ("well", "ill", "graded_up", "graded_down", "zero", "diagonal")
BAD_FAMILIES = ("notpd", "notpd_last")


def families_at(r):
    if r > 256 and r not in FULL_ABOVE_256:
        return ("well", "zero", "diagonal")
    return FAMILIES


def _orth(rng, r):
    Q, R = np.linalg.qr(rng.normal(0, 1, (r, r)))
    return Q * np.sign(np.diag(R))[None, :]


def _spectrum(rng, r, lo, hi):
    s = 10.0 ** rng.uniform(lo, hi, r)
    if r >= 2:  # both ends present: the condition number does not depend on the draw
        s[0], s[-1] = 10.0 ** hi, 10.0 ** lo
    else:
        s[0] = 10.0 ** hi
    return s


def _sym(G):
    return np.ascontiguousarray(0.5 * (G + G.T))


@functools.lru_cache(maxsize=None)
def make_case(family, r):
    """(G, rhs, z, qte_dir): float64.  rhs = (I + G) a0 with a0 ~ N(0, 1), so that every entry of a carries weight; qte is built by
    the caller as S_tot (a0 + w) from qte_dir = a0 + w (b = S_tot w up to rounding: no cancellation in the density's right-hand side)."""
    rng = np.random.default_rng((FAMILIES + BAD_FAMILIES).index(family) * 10007 + r)
    if family in ("well", "notpd", "notpd_last"):
        B = _orth(rng, r)
        G = _sym((B * _spectrum(rng, r, -2, 3)[None, :]) @ B.T)
    elif family == "ill":
        B = _orth(rng, r)
        G = _sym((B * _spectrum(rng, r, -6, 8)[None, :]) @ B.T)
    elif family in ("graded_up", "graded_down"):
        X = rng.normal(0, 1, (r, r + 5))
        C = X @ X.T / (r + 5) + 0.1 * np.eye(r)
        d = 1.0 / np.sqrt(np.diag(C))
        C = C * d[:, None] * d[None, :]
        D = 10.0 ** np.linspace(-3, 3, r) if r > 1 else np.array([1e3])
        if family == "graded_down":
            D = D[::-1]
        G = _sym(C * D[:, None] * D[None, :])
    elif family == "zero":
        G = np.zeros((r, r))
    elif family == "diagonal":
        G = np.diag(0.25 + 0.5 * np.arange(r) + rng.uniform(0, 0.125, r))  # a distinct value per index
    else:
        raise KeyError(family)
    if family == "notpd":  # one eigenvalue of I + G at -0.5
        B = _orth(rng, r)
        s = _spectrum(rng, r, -2, 3)
        s[rng.integers(r)] = -1.5
        G = _sym((B * s[None, :]) @ B.T)
    if family == "notpd_last":  # leading minors untouched, the last pivot is -0.5
        L = np.linalg.cholesky(np.eye(r) + G)
        G = G.copy()
        G[r - 1, r - 1] -= L[r - 1, r - 1] ** 2 + 0.5
    a0 = rng.normal(0, 1, r)
    rhs = (np.eye(r) + G) @ a0 if family not in ("zero",) else a0.copy()
    z = rng.normal(0, 1, r)
    qdir = a0 + rng.normal(0, 1, r)
    for v in (G, rhs, z, qdir):
        v.setflags(write=False)
    return G, rhs, z, qdir


def qte_of(S_ld, qdir):
    return np.asarray(S_ld @ qdir.astype(LD), dtype=np.float64)


def cond_of(G):
    w = np.linalg.eigvalsh(np.eye(G.shape[0]) + G)
    return float(w[-1] / w[0])


# ------------------------------------------------------------------------------------------------ linear algebra, any dtype
def cholesky_left(A):
    """Left-looking Cholesky, column at a time with vectorised products; raises LinAlgError at a non-positive pivot."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} not positive")
        d = np.sqrt(v[0])
        L[j:, j] = v / d
        L[j, j] = d
    return L


def forward_sub(L, b):
    y = np.array(b, dtype=L.dtype)
    for j in range(L.shape[0]):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    return y


def backward_sub_t(L, y):
    """x = L^-T y"""
    x = np.array(y, dtype=L.dtype)
    for j in range(L.shape[0] - 1, -1, -1):
        x[j] /= L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def solve_all(G, rhs, z, S, qte, dtype, chol=None, damage=None):
    """The three outputs on one route: dtype longdouble = the reference; float64 with chol = np.linalg.cholesky = the plain route the
    GPU bounds are measured on.  damage(L) -> L: the deliberately wrong factor of the bite check."""
    r = G.shape[0]
    chol = chol or cholesky_left
    N = np.eye(r, dtype=dtype) + G.astype(dtype)
    L = chol(N)
    if damage is not None:
        L = damage(L.copy())
    a = backward_sub_t(L, forward_sub(L, rhs.astype(dtype)))
    s = a + backward_sub_t(L, z.astype(dtype))
    Sd = S.astype(dtype)
    K = Sd + dtype(EPS) * N
    Lk = chol(0.5 * (K + K.T))
    if damage is not None:
        Lk = damage(Lk.copy())
    b = qte.astype(dtype) - Sd @ a
    u = backward_sub_t(Lk, forward_sub(Lk, b))
    logpdf = dtype(-0.5) * (u @ (N @ u)) - dtype(0.5 * r) * dtype(LOG_2PI)
    return {"a": a, "s": s, "logpdf": logpdf, "L": L, "N": N}


@functools.lru_cache(maxsize=None)
def reference(family, r):
    """Extended-precision outputs of (family, r) plus the inputs: cached per (family, r), never modified."""
    ref, mean, U, lam = model_parts(r)
    S = stot_cached(r)
    G, rhs, z, qdir = make_case(family, r)
    qte = qte_of(S, qdir)
    out = solve_all(G, rhs, z, S, qte, LD)
    out.update(G=G, rhs=rhs, z=z, qte=qte, lam=lam)
    return out


@functools.lru_cache(maxsize=None)
def stot_cached(r):
    _, _, U, lam = model_parts(r)
    return stot_ld(U, lam)


# ------------------------------------------------------------------------------------------------ family 6: the eigen route
EIG_SIGMA2 = (0.1, 100.0)  # lam / sigma2 in [1, 1e5] and [1e-3, 1e2]: together [1e-3, 1e5]


def eig_model_parts(r, orthonormal=True):
    """model_parts(r), or the same with basis columns that are NOT orthonormal (gingr_model_upload does not ask for it: S_tot is a
    full matrix then): U (I + 0.5 W / sqrt(r)), W standard normal."""
    ref, mean, U, lam = model_parts(r)
    if not orthonormal:
        rng = np.random.default_rng(5000 + r)
        U = np.ascontiguousarray(U @ (np.eye(r) + 0.5 * rng.normal(0, 1, (r, r)) / np.sqrt(r)))
    return ref, mean, U, lam


def eig_rhs(r):
    rhs = np.random.default_rng(7000 + r).normal(0, 1, r)
    rhs.setflags(write=False)
    return rhs


def undo_alpha_map(alpha, S, lam, orthonormal):
    """a from alpha = C C a, C = (S_tot + eps I)^-1 S_tot: a = (I + eps S_tot^-1)^2 alpha in extended precision; with orthonormal
    columns S_tot is diagonal to rounding and the element-wise map serves (its off-diagonal part enters as eps dS / lam^2)."""
    alpha = np.asarray(alpha, dtype=LD)
    if orthonormal:
        return alpha / alpha_map_ld(lam)
    Ls = cholesky_left(S)
    for _ in range(2):
        alpha = alpha + LD(EPS) * backward_sub_t(Ls, forward_sub(Ls, alpha))
    return alpha


def eig_reference(r, sigma2, orthonormal=True):
    """(reference dict, float64 figures): a = (I + S_tot / sigma2)^-1 rhs in extended precision, and the forward / backward figures of
    the plain float64 route (np.linalg.cholesky, two triangular solves, the alpha map and back)."""
    _, _, U, lam = eig_model_parts(r, orthonormal)
    S = stot_ld(U, lam)
    rhs = eig_rhs(r)
    N = np.eye(r, dtype=LD) + S / LD(sigma2)
    L = cholesky_left(N)
    ref = {"a": backward_sub_t(L, forward_sub(L, rhs.astype(LD))), "N": N, "L": L, "rhs": rhs, "S": S, "lam": lam}
    S64 = np.asarray(S, dtype=np.float64)
    L64 = np.linalg.cholesky(np.eye(r) + S64 / sigma2)
    a64 = backward_sub_t(L64, forward_sub(L64, rhs))
    C64 = np.linalg.solve(S64 + EPS * np.eye(r), S64)
    f64 = figures(ref, undo_alpha_map(C64 @ (C64 @ a64), S, lam, orthonormal), None, None)
    return ref, f64


# ------------------------------------------------------------------------------------------------ layer B: a real CPD state
READBACK_RANKS = [1, 16, 17, 112, 113, 128, 129, 256, 385]
MH_RANKS = [r for r in READBACK_RANKS if r <= 112]  # the factor of I + G is left behind by the split kernel only (rp <= 112)
READBACK_SIGMA2 = 0.04  # small: the weights P1 / sigma2 put cond(I + G) above 1e6


def readback_model_parts(r):
    """A model whose lam spans [1e-3, 1e6] (both ends present from rank 2 on), the state's target and the queried mesh."""
    rng = np.random.default_rng(9000 + r)
    M = max(200, -(-r // 3) + 7) + 1
    ref = rng.normal(0, 30, (M, 3))
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    lam = 10.0 ** rng.uniform(-3, 6, r)
    if r >= 2:
        lam[0], lam[-1] = 1e6, 1e-3
    lam = np.sort(lam)[::-1].copy()
    # the target lies within sigma = 0.2 (READBACK_SIGMA2) of the zero state's fit (weights P1 / sigma2 of order one: G carries the spread of lam); with a
    # target an instance away every P1 underflows and the reference's own CPD posterior is not finite either
    target = ref + rng.normal(0, 0.1, (M, 3))
    mesh = ref + (U @ (np.sqrt(lam) * 0.1 * rng.normal(0, 1, r))).reshape(M, 3) + rng.normal(0, 0.2, (M, 3))
    return ref, np.zeros((M, 3)), np.ascontiguousarray(U), lam, target, mesh


def density_only(G, rhs, S, qte, dtype, chol=None):
    return solve_all(G, rhs, np.zeros(G.shape[0]), S, qte, dtype, chol=chol)


# ------------------------------------------------------------------------------------------------ figures
def _n(v):
    return np.sqrt(np.sum(np.asarray(v, dtype=LD) ** 2))


def figures(ref, a, s, logpdf):
    """The four figures of a route's outputs (a, s: coefficient space; any may be None) against the reference `ref`."""
    N, L = ref["N"], ref["L"]
    nN = _n(N)  # Frobenius: an upper bound of the 2-norm, the same for every route
    out = {}
    if a is not None:
        a = np.asarray(a, dtype=LD)
        out["forward"] = float(_n(a - ref["a"]) / _n(ref["a"]))
        out["backward"] = float(_n(N @ a - ref["rhs"].astype(LD)) / (nN * _n(a) + _n(ref["rhs"])))
    if s is not None:
        s = np.asarray(s, dtype=LD)
        d = s - ref["a"]
        out["sample_forward"] = float(_n(s - ref["s"]) / _n(ref["s"]))
        out["sample_backward"] = float(_n(L.T @ d - ref["z"].astype(LD)) / (_n(L) * _n(d) + _n(ref["z"])))
    if logpdf is not None:
        out["density"] = float(abs(LD(logpdf) - ref["logpdf"]) / abs(ref["logpdf"]))
    return out


FIGURE_NAMES = ("forward", "backward", "sample_forward", "sample_backward", "density")


def float64_route(family, r, damage=None):
    """np.linalg.cholesky, two triangular solves, the same density formula, the same alpha map -- and back through the map, as a
    device result is."""
    return float64_route_on(reference(family, r), stot_cached(r), damage)


def reference_on(G, rhs, z, S, qte, lam):
    """The extended-precision outputs of a system that is not one of the families (a real state's, copied out of the device)."""
    out = solve_all(G, rhs, z, S, qte, LD)
    out.update(G=G, rhs=rhs, z=z, qte=qte, lam=lam)
    return out


def float64_route_on(ref, S, damage=None):
    S64 = np.asarray(S, dtype=np.float64)
    o = solve_all(ref["G"], ref["rhs"], ref["z"], S64, ref["qte"], np.float64, chol=np.linalg.cholesky, damage=damage)
    c64 = (ref["lam"] / (ref["lam"] + EPS)) ** 2
    cm = alpha_map_ld(ref["lam"])
    a = (c64 * o["a"]).astype(LD) / cm
    s = (c64 * o["s"]).astype(LD) / cm
    return figures(ref, a, s, o["logpdf"])


def measure_float64_figures(ranks=None):
    """family -> figure -> maximum over the ranks of the float64 route's figure."""
    table = {f: {k: 0.0 for k in FIGURE_NAMES} for f in FAMILIES}
    for r in (ranks or RANKS):
        for fam in families_at(r):
            for k, v in float64_route(fam, r).items():
                table[fam][k] = max(table[fam][k], v)
    return table


# The float64 route's figures as measured by test_posterior_solve_host.py::test_float64_figures (maximum over RANKS).  The GPU bounds
# are 1000 x these ("1 000 x the spread"), so they are committed rather than re-measured on every GPU test; the host test
# re-measures them and fails when a committed figure is off by more than a factor 2 either way.
F64_FIGURES = {
    "well": {"forward": 7.07e-14, "backward": 8.08e-17, "sample_forward": 6.24e-14, "sample_backward": 8.00e-16, "density": 9.94e-16},
    "ill": {"forward": 4.75e-09, "backward": 1.50e-16, "sample_forward": 4.31e-09, "sample_backward": 2.54e-13, "density": 5.36e-11},
    "graded_up": {"forward": 6.86e-14, "backward": 7.06e-17, "sample_forward": 5.61e-14, "sample_backward": 4.34e-14, "density": 3.43e-15},
    "graded_down": {"forward": 2.44e-14, "backward": 8.74e-17, "sample_forward": 1.74e-14, "sample_backward": 1.79e-14, "density": 1.75e-15},
    "zero": {"forward": 2.45e-16, "backward": 1.23e-16, "sample_forward": 2.30e-16, "sample_backward": 3.04e-16, "density": 1.91e-16},
    "diagonal": {"forward": 4.10e-16, "backward": 2.05e-16, "sample_forward": 2.39e-16, "sample_backward": 3.28e-16, "density": 3.71e-16},
}


def gpu_bound(family, figure, r):
    """1000 x the float64 figure of (family, figure); floored at r 2^-53 where that figure is exactly zero."""
    f = F64_FIGURES[family][figure]
    return 1000.0 * f if f > 0.0 else r * 2.0 ** -53
