"""numpy restatement of the kernel warp (gingr_amd/csrc/kernel_warp.hip): the fitted map of a classic CPD or BCPD task at points off
the template,

    T(z) = A (z + sum_m g(z, y_m) c_m) + t,   g(a, b) = exp(-|a - b|^2 / (2 beta^2)),

with the plan's bookkeeping (kernel_warp_plan.h: chunks of CHUNK centres, partials added in chunk order), the reference formula in
np.longdouble, the accuracy bound the tests hold a float64 result to, and the coefficients of the Bayesian CPD,
c = (c2 / lambda) (r - nu o v^), in the names of tests/bcpd_restatement.py."""
import numpy as np

TILE, CHUNK_TILES = 256, 8
CHUNK = TILE * CHUNK_TILES
MAX_SLAB, MAX_PARTIAL_DOUBLES = 1 << 20, 1 << 24
U = 2.0 ** -53


def plan(P, M):
    """make_plan(P, M): (chunks, slab length, slabs)"""
    chunks = -(-M // CHUNK)
    cap = MAX_SLAB
    if chunks > 0:
        cap = max(TILE, min(cap, MAX_PARTIAL_DOUBLES // (3 * chunks) // TILE * TILE))
    slab = min(P, cap)
    return chunks, slab, (-(-P // slab) if P > 0 else 0)


def gauss(Z, Y, beta, dtype=np.float64):
    Z, Y = np.asarray(Z, dtype), np.asarray(Y, dtype)
    d = Z[:, None, :] - Y[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return np.exp(-d2 / (2 * dtype(beta) * dtype(beta)))


def head(A=None, t=None, dtype=np.float64):
    return (np.eye(3, dtype=dtype) if A is None else np.asarray(A, dtype)), (np.zeros(3, dtype) if t is None else np.asarray(t, dtype))


def warp_blocked(Z, Y, C, beta, A=None, t=None):
    """float64, the centres in the plan's chunks, the chunk partials added in chunk order, then `+ z`, then the head"""
    Z, Y, C = (np.asarray(a, np.float64) for a in (Z, Y, C))
    v = np.zeros_like(Z)
    for m0 in range(0, Y.shape[0], CHUNK):
        v = v + gauss(Z, Y[m0:m0 + CHUNK], beta) @ C[m0:m0 + CHUNK]
    A, t = head(A, t)
    return (Z + v) @ A.T + t[None, :]


def warp_reference(Z, Y, C, beta, A=None, t=None):
    """the formula in np.longdouble; returns (T(Z), S) with S_p = max_d sum_m g_pm |c_md|, the scale of the bound"""
    ld = np.longdouble
    Z, Y, C = (np.asarray(a, ld) for a in (Z, Y, C))
    out, S = np.empty(Z.shape, ld), np.empty(Z.shape[0], ld)
    A, t = head(A, t, ld)
    for p0 in range(0, Z.shape[0], 64):  # (slabs of queries: the P x M block in long double stays small)
        g = gauss(Z[p0:p0 + 64], Y, beta, ld)
        out[p0:p0 + 64] = (Z[p0:p0 + 64] + g @ C) @ A.T + t[None, :]
        S[p0:p0 + 64] = (g @ np.abs(C)).max(1) if Y.shape[0] else 0
    return out, S


def bound(Z, M, S, ref, A=None, t=None, sum_factor=1.0):
    """|dev_p - ref_p|_inf <= |A|_inf [(2 M u + 4e-13) S_p + 8 u (|z_p|_inf + S_p)] + 16 u (|ref_p|_inf + |t|_inf), per row;
    sum_factor = 2 where both sides are float64 sums of the same entries in different orders"""
    A, t = head(A, t)
    nA = float(np.abs(A).sum(1).max())
    Z = np.asarray(Z, np.float64)
    S, ref = np.asarray(S, np.float64), np.asarray(ref, np.float64)
    zmax, rmax = np.abs(Z).max(1), np.abs(ref).max(1)
    return nA * (sum_factor * (2.0 * M * U + 4e-13) * S + 8.0 * U * (zmax + S)) + 16.0 * U * (rmax + float(np.abs(t).max()))


def ratio(got, Z, Y, C, beta, A=None, t=None, sum_factor=1.0):
    """the largest |got_p - ref_p|_inf / bound_p over the rows (a row whose bound is 0 must be exact)"""
    ref, S = warp_reference(Z, Y, C, beta, A, t)
    err = np.abs(np.asarray(got, np.longdouble) - ref).max(1).astype(np.float64)
    b = bound(Z, np.asarray(Y).shape[0], S, ref, A, t, sum_factor)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ BCPD: the coefficients
def bcpd_coefficients(p, st, route="woodbury"):
    """One iteration of the tests/bcpd_restatement.py Problem `p` from the state `st`: returns (c, c', vhat, new state) with
    c = (c2 / lambda) (r - nu o vhat) and c' = (c2 / lambda) (r - d^1/2 o q), the same vector through the solve's q (A q = D^1/2 z;
    woodbury route only, else None).  c2 = s^2 / sigma2 and r are those that go INTO the iteration."""
    new = p.iterate(st, route)
    nu, PX = new.nu, new.PX
    c2 = st.s ** 2 / st.sigma2
    r = (PX - nu[:, None] * st.t[None, :]) @ st.R / st.s - nu[:, None] * p.y
    c = (c2 / p.lam) * (r - nu[:, None] * new.vhat)
    cq = None
    if route == "woodbury":
        K = p.G / p.lam
        dh = np.sqrt(c2 * nu)
        Am = np.eye(p.M) + dh[:, None] * K * dh[None, :]
        q = np.linalg.solve(Am, dh[:, None] * (K @ r))
        cq = (c2 / p.lam) * (r - dh[:, None] * q)
    return c, cq, new.vhat, new


def coefficient_residual(G, c, vhat):
    """max |G c - vhat| relative to max |vhat|"""
    return float(np.abs(G @ c - vhat).max() / np.abs(vhat).max())


# ------------------------------------------------------------------------------------------------ the tests' inputs
def centres(M, seed, side=8.0):
    """M centres uniform in a cube, coefficients N(0, 0.3^2) with every seventh row zero"""
    rng = np.random.default_rng(seed)
    Y = rng.uniform(-side / 2, side / 2, (M, 3))
    C = rng.normal(0, 0.3, (M, 3))
    C[::7] = 0.0
    return Y, C


def queries(P, Y, seed, margin=0.25):
    """P points uniform in the box of Y grown by `margin` of its extent on every side (a single centre: a box of side 2 about it)"""
    rng = np.random.default_rng(seed)
    Y = np.asarray(Y, np.float64)
    lo, hi = Y.min(0), Y.max(0)
    ext = np.where(hi > lo, hi - lo, 2.0)
    return rng.uniform(lo - margin * ext, hi + margin * ext, (P, 3))
