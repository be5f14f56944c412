"""Cases and extended-precision reference for landmarks_kernel (gingr_amd/csrc/gp_obs.hip): every observation with a full 3 x 3
covariance adds, for list entry l with model point p, pose (R, t, center) and covariance C_l,

    W_l = R^T C_l^-1 R,    G += Q_p^T W_l Q_p,    rhs += Q_p^T W_l v_l,    v_l = R^T (x_l - center - t) - (ref_p - center) - mean_p

to the posterior system.  Plain module, no tests in here: test_landmark_system_host.py (CPU) checks the builders and measures the
float64 route, test_gpu_landmark_system.py compares the device's G and rhs element by element.

Reference (`reference`): Q = U sqrt(lam) from the uploaded parts, rounded to float64 as the upload rounds it (model.hip: Q0 = U sqrt(lambda),
rows 3 p + d); the 3 x 3 inverses by mpmath at 60 digits; every other product and sum in np.longdouble; rows -1 skipped.  Gabs and
rhsabs are the same sums over the absolute values of the per-entry terms: the scale every deviation is divided by, so that cancellation
between entries does not inflate a figure.  The float64 route is the same function in float64 with np.linalg.inv (what
oracle.gingr_oracle.PDM._regression does); `deviation(route, ref)` is max |delta| / max Gabs resp. max rhsabs.

Every case carries a guard on its inputs alone (`check_guard`): the eigenvalue ratios of its covariance family, the number of chunks of
kLmChunk = 256 entries and the length of the last one, the positions of its -1 rows and which column class the padded rank falls in
(each lane owns kCols = 2 columns: the second is idle for rp <= 256, ragged for 256 < rp < 512, full at 512).
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from tests import posterior_solve_cases as pc

LD = np.longdouble
K_CHUNK = 256            # kLmChunk of gp_obs.hip
M_POINTS = 300
RANKS = (24, 264, 512)   # rp = 32, 272, 512
FAMILIES = ("iso", "well", "pancake", "needle", "graded")
NOMINAL = {"pancake": (1e4, 1e4, 1e-4), "needle": (1e4, 1e-2, 1e-2), "graded": (1e4, 1.0, 1e-4)}
ISO_SCALES = (1.0, 1e-2, 1e2, 7.0)

IDENTITY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
# R = Rz(0.25) Ry(-0.2) Rx(0.22): 0.39 rad about the axis (0.50, -0.66, 0.56); then a translation and a rotation centre off the origin
SKEW = ((0.25, -0.2, 0.22), (4.0, -7.0, 2.5), (11.0, 3.0, -6.0))   # euler, translation, center


def column_class(rp):
    return "one" if rp <= K_CHUNK else ("ragged" if rp < 2 * K_CHUNK else "two")


def euler_to_rot(euler):
    """R = Rz(phi) Ry(theta) Rx(psi), the convention of svd3.h / oracle.gingr_oracle.euler_to_rot, in float64"""
    phi, theta, psi = (float(e) for e in euler)
    cphi, sphi, cth, sth, cpsi, spsi = math.cos(phi), math.sin(phi), math.cos(theta), math.sin(theta), math.cos(psi), math.sin(psi)
    return np.array([[cth * cphi, spsi * sth * cphi - cpsi * sphi, spsi * sphi + cpsi * sth * cphi],
                     [cth * sphi, cpsi * cphi + spsi * sth * sphi, cpsi * sth * sphi - spsi * cphi],
                     [-sth, spsi * cth, cpsi * cth]])


# ------------------------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def model_parts(r):
    """(ref, mean, U, lam): 300 points, a non-zero mean, orthonormal U from a QR, lam graded from 1e4 down to 1e-1"""
    rng = np.random.default_rng(4000 + r)
    ref = rng.normal(0, 30, (M_POINTS, 3))
    mean = rng.normal(0, 2, (M_POINTS, 3))
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M_POINTS, r)))
    lam = 10.0 ** np.linspace(4, -1, r)
    out = (ref, mean, np.ascontiguousarray(U), lam)
    for a in out:
        a.setflags(write=False)
    return out


def basis_rows(U, lam):
    """Q [M, 3, r] in float64: the rounding of the upload (one square root and one product per entry)"""
    return (U * np.sqrt(lam)[None, :]).reshape(U.shape[0] // 3, 3, lam.shape[0])


# ------------------------------------------------------------------------------------------------------------------ covariances
def spd_covariances(rng, n):
    """the `well` family: the builder of test_gpu_template_pairs.py (condition about 100)"""
    A = rng.normal(0, 1, (n, 3, 3))
    return A @ np.swapaxes(A, 1, 2) + np.diag([0.2, 1.0, 3.0])[None]


def _orth(rng, n):
    Q, R = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return Q * np.sign(np.einsum("nii->ni", R))[:, None, :]


@functools.lru_cache(maxsize=None)
def covariances(family, n, seed):
    """n symmetric 3 x 3 matrices of `family`, each rotated by a seeded random orthogonal matrix and symmetrised"""
    rng = np.random.default_rng(100 * seed + FAMILIES.index(family))
    if family == "well":
        C = spd_covariances(rng, n)
    else:
        B = _orth(rng, n)
        if family == "iso":
            ev = np.array(ISO_SCALES)[np.arange(n) % len(ISO_SCALES)][:, None] * np.ones((n, 3))   # entry 0: c = 1
        else:
            ev = np.tile(np.array(NOMINAL[family]), (n, 1))
        C = np.einsum("nij,nj,nkj->nik", B, ev, B)
        if family == "iso":
            C = ev[:, :1, None] * np.eye(3)[None]    # a multiple of the identity exactly: the rotation changes nothing
    C = np.ascontiguousarray(0.5 * (C + np.swapaxes(C, 1, 2)))
    C.setflags(write=False)
    return C


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    r: int
    L: int                    # length of the list the kernel sees ([pairs | landmarks] for the concatenated case)
    family: str
    pose: tuple               # (euler, translation, center)
    n_landmarks: int = 0      # the last n entries go through set_landmarks, the others through set_pairs_cov
    override: tuple = ()      # positions of the pair list whose vertex one of the landmarks takes over (rows -1)

    @property
    def rp(self):
        return pc.rp_of(self.r)


def _cases():
    out = []

    def add(r, L, family, pose, **kw):
        tag = "identity" if pose is IDENTITY else "skew"
        out.append(Case(f"r{r}-L{L}-{family}-{tag}" + ("-override" if kw.get("override") else ""), r, L, family, pose, **kw))

    # lists of up to 3 entries are landmarks, longer ones covariance pairs
    add(24, 1, "well", IDENTITY, n_landmarks=1)
    add(24, 3, "well", SKEW, n_landmarks=3)
    for L in (255, 256, 257, 600):
        add(24, L, "well", SKEW)
    for family in ("iso", "pancake", "needle", "graded"):
        add(24, 257, family, SKEW)
    add(264, 257, "well", IDENTITY)
    add(264, 600, "well", SKEW)
    add(264, 256, "well", SKEW)
    for family, L in (("iso", 257), ("pancake", 257), ("needle", 600), ("graded", 257)):
        add(264, L, family, SKEW)
    add(264, 3, "needle", SKEW, n_landmarks=3)
    # [597 pairs | 3 landmarks]: the landmarks' vertices hold pairs in all three chunks, on chunk edges (0, 255, 256) and away from them
    add(264, 600, "well", SKEW, n_landmarks=3, override=(0, 100, 255, 256, 300, 530))
    add(512, 1, "well", SKEW, n_landmarks=1)
    add(512, 257, "well", IDENTITY)
    add(512, 600, "well", SKEW)
    add(512, 257, "needle", SKEW)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SHORT_LANDMARK_CASES = tuple(c.name for c in CASES if c.n_landmarks == c.L)


@dataclasses.dataclass(frozen=True)
class Lists:
    """What the caller hands over (pair_*: gingr_fitter_set_pairs_cov, lm_*: gingr_fitter_set_landmarks) and what the kernel sees:
    rows (-1: skipped), points, covs of the concatenated list."""
    pair_pids: np.ndarray
    pair_points: np.ndarray
    pair_covs: np.ndarray
    lm_pids: np.ndarray
    lm_points: np.ndarray
    lm_covs: np.ndarray
    rows: np.ndarray
    points: np.ndarray
    covs: np.ndarray


def posed_point(parts, pose, pid):
    ref, mean = parts[0], parts[1]
    euler, t, c = pose
    return (ref[pid] + mean[pid] - np.asarray(c)) @ euler_to_rot(euler).T + np.asarray(c) + np.asarray(t)


@functools.lru_cache(maxsize=None)
def lists_of(name):
    case = BY_NAME[name]
    parts = model_parts(case.r)
    rng = np.random.default_rng(7919 * case.r + 31 * case.L + FAMILIES.index(case.family) + 1000 * case.n_landmarks)
    n_pairs = case.L - case.n_landmarks
    covs = covariances(case.family, case.L, 17 + case.r)
    lm_pids = rng.permutation(M_POINTS)[: case.n_landmarks].astype(np.int64)
    if n_pairs:
        # repeated, unordered vertex ids (test_covariance_pairs): two thirds distinct, the rest drawn from them again
        pool = np.setdiff1d(np.arange(M_POINTS), lm_pids)
        base = rng.permutation(pool)[: max(1, min(2 * n_pairs // 3, pool.shape[0] - 1))]
        pids = np.concatenate([base, rng.choice(base, n_pairs - base.shape[0])])[rng.permutation(n_pairs)].astype(np.int64)
        for k, pos in enumerate(case.override):
            pids[pos] = lm_pids[k % case.n_landmarks]
    else:
        pids = np.zeros(0, dtype=np.int64)
    all_pids = np.concatenate([pids, lm_pids])
    # observed points: the posed model point plus noise of a few units (v_l of order one to ten)
    points = posed_point(parts, case.pose, all_pids) + rng.normal(0, 2.0, (case.L, 3))
    rows = all_pids.copy()
    rows[:n_pairs][np.isin(pids, lm_pids)] = -1          # pairs_rebuild_cov_list: a landmark's vertex loses its covariance pairs
    out = Lists(pids, points[:n_pairs], covs[:n_pairs], lm_pids, points[n_pairs:], covs[n_pairs:], rows, points, covs)
    for f in dataclasses.fields(out):
        getattr(out, f.name).setflags(write=False)
    return out


def check_guard(case, lists=None):
    """The edges the case is built for, on its inputs alone; raises AssertionError with the case's name."""
    li = lists or lists_of(case.name)
    assert li.rows.shape == (case.L,) and li.covs.shape == (case.L, 3, 3) and li.points.shape == (case.L, 3), case.name
    assert np.array_equal(li.covs, np.swapaxes(li.covs, 1, 2)), case.name
    ev = np.linalg.eigvalsh(li.covs)[:, ::-1]
    if case.family in NOMINAL:
        nom = np.array(NOMINAL[case.family])
        for a, b in ((0, 1), (1, 2), (0, 2)):          # eigenvalue ratios within 1 % of the nominal ones
            assert np.all(np.abs(ev[:, a] / ev[:, b] / (nom[a] / nom[b]) - 1.0) < 0.01), (case.name, a, b)
    elif case.family == "iso":
        assert all(np.array_equal(C, C[0, 0] * np.eye(3)) for C in li.covs) and li.covs[0, 0, 0] == 1.0, case.name
        assert case.L < len(ISO_SCALES) or len({C[0, 0] for C in li.covs}) == len(ISO_SCALES), case.name
    else:
        assert np.all(ev[:, 2] > 0.19) and np.all(ev[:, 0] / ev[:, 2] < 1e3), case.name
    # chunks
    chunks, last = -(-case.L // K_CHUNK), (case.L - 1) % K_CHUNK + 1
    want = {1: (1, 1), 3: (1, 3), 255: (1, 255), 256: (1, 256), 257: (2, 1), 600: (3, 88)}[case.L]
    assert (chunks, last) == want, (case.name, chunks, last)
    # -1 rows and where they fall
    skipped = tuple(int(i) for i in np.flatnonzero(li.rows < 0))
    assert skipped == tuple(sorted(case.override)), (case.name, skipped)
    if case.override:
        assert {0, 255, 256} <= set(skipped) and {i // K_CHUNK for i in skipped} == {0, 1, 2}, case.name
        assert any(i % K_CHUNK not in (0, K_CHUNK - 1) for i in skipped), case.name
        assert np.isin(li.lm_pids, li.pair_pids).all() and case.L - case.n_landmarks > 2 * K_CHUNK, case.name
    n_pairs = case.L - case.n_landmarks
    if n_pairs > 3:                                    # repeated, unordered vertex ids
        assert np.unique(li.pair_pids).shape[0] < n_pairs and (np.diff(li.pair_pids) < 0).any(), case.name
    assert np.unique(li.lm_pids).shape[0] == case.n_landmarks, case.name
    assert case.L <= 3 or n_pairs > 3, case.name       # short lists are landmarks, long ones pairs
    # column class
    assert column_class(case.rp) == {24: "one", 264: "ragged", 512: "two"}[case.r], case.name
    # pose
    R = euler_to_rot(case.pose[0])
    angle = math.acos(min(1.0, (np.trace(R) - 1.0) / 2.0))
    if case.pose is IDENTITY:
        assert angle == 0.0 and not any(case.pose[1]) and not any(case.pose[2]), case.name
    else:
        axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2 * math.sin(angle))
        assert 0.35 < angle < 0.45 and np.abs(axis).min() > 0.3 and all(case.pose[1]) and all(case.pose[2]), (case.name, angle, axis)


def check_coverage():
    """what the set of cases as a whole must meet"""
    seen = {(c.r, c.L) for c in CASES}
    for r in RANKS:
        assert (r, 257) in seen and (r, 600) in seen, r
        assert any(c.r == r and c.pose is IDENTITY for c in CASES), r
    for fam in FAMILIES:
        for r in (24, 264):
            assert any(c.r == r and c.family == fam for c in CASES), (fam, r)
    assert {c.L for c in CASES} >= {1, 3, 255, 256, 257, 600}
    assert [c.r for c in CASES if c.override] == [264]


# ------------------------------------------------------------------------------------------------------------------ reference
def _ld_of_mpf(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def mp_inverse(C):
    """the inverse of a 3 x 3 float64 matrix by cofactors at 60 digits (the cancellation of the determinant costs at most cond^2), as
    np.longdouble"""
    import mpmath
    with mpmath.workdps(60):
        c = [mpmath.mpf(float(v)) for v in np.asarray(C).reshape(9)]
        cof = [c[4] * c[8] - c[5] * c[7], c[2] * c[7] - c[1] * c[8], c[1] * c[5] - c[2] * c[4],
               c[5] * c[6] - c[3] * c[8], c[0] * c[8] - c[2] * c[6], c[2] * c[3] - c[0] * c[5],
               c[3] * c[7] - c[4] * c[6], c[1] * c[6] - c[0] * c[7], c[0] * c[4] - c[1] * c[3]]
        det = c[0] * cof[0] + c[1] * cof[3] + c[2] * cof[6]
        return np.array([_ld_of_mpf(v / det) for v in cof], dtype=LD).reshape(3, 3)


def cofactor_inverse(C):
    """the formula landmarks_kernel used before the Cholesky inverse, operation by operation in float64 (the host emulation of the revert
    check)"""
    c = [float(v) for v in np.asarray(C, dtype=np.float64).reshape(9)]
    det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])
    return np.array([(c[4] * c[8] - c[5] * c[7]) / det, (c[2] * c[7] - c[1] * c[8]) / det, (c[1] * c[5] - c[2] * c[4]) / det,
                     (c[5] * c[6] - c[3] * c[8]) / det, (c[0] * c[8] - c[2] * c[6]) / det, (c[2] * c[3] - c[0] * c[5]) / det,
                     (c[3] * c[7] - c[4] * c[6]) / det, (c[1] * c[6] - c[0] * c[7]) / det, (c[0] * c[4] - c[1] * c[3]) / det]).reshape(3, 3)


def reference(parts, pose, rows, points, covs, dtype=LD, inverse=None):
    """-> (G [r r], rhs [r], Gabs, rhsabs) in `dtype`: the kernel's definition in the device frame.  dtype np.longdouble with the mpmath
    inverse is the reference, np.float64 with np.linalg.inv the float64 route; `inverse` replaces the 3 x 3 inverse."""
    ref, mean, U, lam = parts
    if inverse is None:
        inverse = mp_inverse if dtype is LD else np.linalg.inv
    euler, t, c = pose
    R = euler_to_rot(euler).astype(dtype)
    t, c = np.asarray(t, dtype=dtype), np.asarray(c, dtype=dtype)
    r = lam.shape[0]
    rows = np.asarray(rows)
    live = np.flatnonzero(rows >= 0)
    p = rows[live]
    Ci = np.array([np.asarray(inverse(covs[l]), dtype=dtype) for l in live], dtype=dtype).reshape(-1, 3, 3)
    W = np.einsum("da,lde,eb->lab", R, Ci, R)                                             # R^T C^-1 R
    v = (points[live].astype(dtype) - c - t) @ R - (ref[p].astype(dtype) - c) - mean[p].astype(dtype)
    Qp = basis_rows(U, lam)[p].astype(dtype)                                              # n x 3 x r
    T = np.einsum("lde,ler->ldr", W, Qp)                                                  # W_l Q_p
    G = Qp.reshape(-1, r).T @ T.reshape(-1, r)
    vec = np.einsum("ldr,ld->lr", T, v)                                                   # per entry: Q_p^T W_l v_l
    rhs, rhsabs = vec.sum(0), np.abs(vec).sum(0)
    # Gabs is a scale only: its per-entry r x r terms are formed in float64, a block of entries at a time
    Gabs = np.zeros((r, r))
    Q64, T64 = np.asarray(Qp, dtype=np.float64), np.asarray(T, dtype=np.float64)
    for b in range(0, live.shape[0], 16):
        Gabs += np.abs(np.swapaxes(Q64[b: b + 16], 1, 2) @ T64[b: b + 16]).sum(0)
    return G, rhs, Gabs.astype(dtype), rhsabs


def deviation(got, ref):
    """(max |G - G_ref| / max Gabs, max |rhs - rhs_ref| / max rhsabs) of a pair (G, rhs, ...) against a reference tuple"""
    G, rhs, Gabs, rhsabs = ref
    dG = np.abs(np.asarray(got[0]).astype(LD) - G).max() / Gabs.max()
    dr = np.abs(np.asarray(got[1]).astype(LD) - rhs).max() / rhsabs.max()
    return float(dG), float(dr)


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """the reference of a case, its float64 route and that route's two figures: computed once per process, never modified"""
    case = BY_NAME[name]
    li = lists_of(name)
    parts = model_parts(case.r)
    ref = reference(parts, case.pose, li.rows, li.points, li.covs)
    f64 = reference(parts, case.pose, li.rows, li.points, li.covs, dtype=np.float64)
    for a in ref + f64:
        a.setflags(write=False)
    return ref, f64, deviation(f64, ref)


def bounds_of(figures, r):
    """1000 x the float64 route's figure of the case ("1 000 x the spread"); floored at r 2^-53 where that figure is zero"""
    return tuple(1000.0 * f if f > 0.0 else r * 2.0 ** -53 for f in figures)
