"""Matrices, reference and judgement for the direct tests of the symmetric eigen-solver (gingr_amd/csrc/sym_eig.hip, eig.hip:
sym_eig / sym_eig_strided and the five kernels behind them).  Plain numpy, importable without a GPU; tests/test_sym_eig_cases_host.py
measures the tolerance with it, tests/test_gpu_sym_eig.py judges the device with it.

  matrices    G = Q diag(lambda) Q^T, Q from the QR of a seeded normal matrix, the product formed in np.longdouble, symmetrised exactly
              ((A + A^T) / 2) and rounded to float64: the kernels read column c as row c, so G is bit-symmetric.  `shifted` is formed
              directly (a centred Gram matrix plus trace / n on the diagonal), `diagonal*` and `identity` need no Q.
  judge       in np.longdouble, relative to lambda_1: max |G V - V diag(e)|, max |V^T V - I|, max |e - reference spectrum|, and whether
              e is non-increasing.  The reference spectrum is LAPACK's of the rounded G, not the lambda that went in.  Single
              eigenvectors are never compared: residual and orthogonality are well posed whatever the gaps.
  tolerance   EIG_ROUTE_SPREAD, the largest figure either of two correct host routes (numpy.linalg.eigh; the cyclic two-sided Jacobi
              below) leaves over every case of this module except `null_many`; the device is held to 1000 x that (DESIGN.md section 4,
              pca_restatement.ROUTE_SPREAD)."""
import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# ---------------------------------------------------------------------------------------------------------------- the cases
KINDS = ("graded", "shifted", "clustered")                    # what every test covers unless it says otherwise
SPECIAL_KINDS = ("identity", "diagonal", "diagonal_perm")
SINGULAR_KINDS = ("null1", "zero_row")

REGISTER_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192)   # the three templates on both sides of their edges
SPECIAL_SIZES = (5, 64, 129)
STRIDED_SIZES = (5, 64, 65, 129, 192)
STRIDED_COUNT = 4
MIXED_BATCHES = ((5, 70, 190), (64, 65, 129))                 # small problems in a large template
BLOCK_SIZES = (193, 224, 225, 256, 257, 321, 449, 512)        # 13 (padded), 14, 15 blocks; E = 4 | 5; E = 6; E = 8; a full last block
BLOCK_BATCHES = ((193, 192, 193), (257, 256, 257))
FALLBACK_ONE_WORKGROUP = (2, 31, 64, 128)                     # jacobi_eig_kernel
FALLBACK_GRID = (129, 192)                                    # jacobi_eig_grid_kernel
TWO_SIDED_DIRECT = (193, 257)                                 # blocks = false
ZERO_ROW_BLOCKS = 200                                         # blocks = true, the block kernel's pivot fails
DEFECT_SIZE = 200
DEFECT_KINDS = ("graded", "zero_row", "shifted")
NULL_MANY_SIZES = (20, 130)


def batch_cases(sizes, kind):
    """the problems of one call: (kind, n, variant), a size that comes twice with two different matrices"""
    seen, out = {}, []
    for n in sizes:
        out.append((kind, n, seen.get(n, 0)))
        seen[n] = seen.get(n, 0) + 1
    return out


def all_cases():
    """every (kind, n, variant) the GPU tests decompose, each once, in a fixed order"""
    cases = []

    def add(c):
        if c not in cases:
            cases.append(c)

    for kind in KINDS:
        for n in REGISTER_SIZES:
            add((kind, n, 0))
        for n in STRIDED_SIZES:
            for v in range(STRIDED_COUNT):
                add((kind, n, v))
        for sizes in MIXED_BATCHES + BLOCK_BATCHES:
            for c in batch_cases(sizes, kind):
                add(c)
        for n in BLOCK_SIZES:
            add((kind, n, 0))
    for kind in SPECIAL_KINDS:
        for n in SPECIAL_SIZES:
            add((kind, n, 0))
    for kind in SINGULAR_KINDS:
        for n in FALLBACK_ONE_WORKGROUP + FALLBACK_GRID:
            add((kind, n, 0))
    for n in TWO_SIDED_DIRECT:
        add(("graded", n, 0))
    add(("zero_row", ZERO_ROW_BLOCKS, 0))
    for kind in DEFECT_KINDS:
        add((kind, DEFECT_SIZE, 0))
    for n in NULL_MANY_SIZES:
        add(("null_many", n, 0))
    return cases


# ---------------------------------------------------------------------------------------------------------------- the matrices
_KIND_IDS = {k: i for i, k in enumerate(KINDS + SPECIAL_KINDS + SINGULAR_KINDS + ("null_many",))}


def _rng(kind, n, variant):
    return np.random.default_rng([_KIND_IDS[kind], n, variant, 20261021])


def graded_spectrum(n):
    """geometric, 1 ... 1e-10: what a Gaussian-kernel Gram matrix looks like"""
    return np.array([1.0]) if n == 1 else 10.0 ** (-10.0 * np.arange(n) / (n - 1))


def clustered_spectrum(n):
    """groups of 1, 2, 3 and 7 exactly equal values, group g at 1 / (1 + g / 4)"""
    lam, g = [], 0
    while len(lam) < n:
        lam += [1.0 / (1.0 + 0.25 * g)] * (1, 2, 3, 7)[g % 4]
        g += 1
    return np.array(lam[:n])


def from_spectrum(lam, rng):
    """Q diag(lam) Q^T in np.longdouble, symmetrised exactly, rounded to float64"""
    n = lam.shape[0]
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    Ql = Q.astype(LD)
    A = (Ql * lam.astype(LD)[None, :]) @ Ql.T
    return np.ascontiguousarray(((A + A.T) / LD(2)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _matrix(kind, n, variant):
    rng = _rng(kind, n, variant)
    if kind == "graded":
        G = from_spectrum(graded_spectrum(n), rng)
    elif kind == "clustered":
        G = from_spectrum(clustered_spectrum(n), rng)
    elif kind == "shifted":
        # n shapes of n + 7 coordinates: a few strong modes and a little noise, centred over the shapes; the Gram matrix of the centred
        # rows is singular (they sum to zero), trace / n on the diagonal makes its condition number at most n + 1 (pca_model.hip).  At
        # n = 1 this is the 1 x 1 zero matrix.
        d = n + 7
        X = rng.normal(size=(n, d)) * (0.7 ** np.arange(d))[None, :] + 0.05 * rng.normal(size=(n, d))
        Xc = X.astype(LD) - X.astype(LD).mean(axis=0)[None, :]
        A = Xc @ Xc.T
        A = A + np.eye(n, dtype=LD) * (np.trace(A) / LD(n))
        G = np.ascontiguousarray(((A + A.T) / LD(2)).astype(np.float64))
    elif kind == "identity":
        G = np.eye(n)
    elif kind in ("diagonal", "diagonal_perm"):
        d = 1.0 / (1.0 + np.arange(n))
        d[min(2, n - 1)] = d[min(1, n - 1)]                    # two equal entries
        if kind == "diagonal_perm":
            d = d[_rng("diagonal", n, variant).permutation(n)]
        G = np.diag(d)
    elif kind == "null1":
        lam = graded_spectrum(n)
        lam[-1] = 0.0
        G = from_spectrum(lam, rng)
    elif kind == "zero_row":
        G = from_spectrum(graded_spectrum(n), rng)
        G[n // 2, :] = 0.0
        G[:, n // 2] = 0.0
    elif kind == "null_many":
        lam = graded_spectrum(n)
        lam[n // 2:] = 0.0
        G = from_spectrum(lam, rng)
    else:
        raise ValueError(kind)
    assert np.array_equal(G, G.T)
    G.setflags(write=False)
    return G


def matrix(kind, n, variant=0):
    """the float64 matrix of a case (bit-symmetric, read-only, computed once)"""
    return _matrix(kind, int(n), int(variant))


@functools.lru_cache(maxsize=None)
def _reference(kind, n, variant):
    e = np.linalg.eigvalsh(matrix(kind, n, variant))[::-1].copy()
    e.setflags(write=False)
    return e


def reference_spectrum(kind, n, variant=0):
    """LAPACK's eigenvalues of the rounded G, descending"""
    return _reference(kind, int(n), int(variant))


# ---------------------------------------------------------------------------------------------------------------- the judgement
def judge(G, evals, V, reference=None):
    """(residual, orthogonality, eigenvalue error, non-increasing) of evals [n] and V [n, n] (eigenvector k in column k) as a
    decomposition of G: max |G V - V diag(e)|, max |V^T V - I|, max |e - reference| -- all in np.longdouble, all relative to lambda_1,
    the largest |reference| (1 for the zero matrix).  A NaN anywhere makes the figure infinite."""
    n = G.shape[0]
    if reference is None:
        reference = np.linalg.eigvalsh(G)[::-1]
    scale = LD(np.abs(reference).max())
    if not scale > 0:
        scale = LD(1)
    Gl, el, Vl = G.astype(LD), np.asarray(evals, dtype=np.float64).astype(LD), np.asarray(V, dtype=np.float64).astype(LD)
    assert el.shape == (n,) and Vl.shape == (n, n)

    def worst(x):
        return float(np.abs(x).max() / scale) if np.isfinite(x).all() else float("inf")

    resid = worst(Gl @ Vl - Vl * el[None, :])
    orth = float(np.abs(Vl.T @ Vl - np.eye(n, dtype=LD)).max()) if np.isfinite(Vl).all() else float("inf")
    err = worst(el - np.asarray(reference).astype(LD))
    monotone = bool(np.all(el[:-1] >= el[1:]))
    return resid, orth, err, monotone


# ---------------------------------------------------------------------------------------------------------------- host route two
def jacobi_eigh(G, max_sweeps=60):
    """(evals descending, V columns, sweeps): cyclic two-sided Jacobi in float64, the round-robin ordering with its n' / 2 disjoint
    rotations of a round applied at once -- tests/cloud_normals_restatement.jacobi_eigh for any n.  A pair rotates while
    |a_pq| > (eps / 2) sqrt(|a_pp a_qq|) and |a_pq| > eps ||G||_F / sqrt(n): with the second the method ends at off(A) <=
    sqrt(n) eps ||G||_F, a backward error of LAPACK's own order -- below it a rotation moves nothing that the figures of judge(), all
    relative to lambda_1, can see, and inside a null space the first alone would go on rotating rounding noise.  A' = J^T A J is
    formed as two row passes with a transposition between them (J^T (J^T A)^T, A symmetric) and V is kept transposed, so that every
    pass reads whole rows.  Nothing here restates the device's kernels."""
    A = np.array(G, dtype=np.float64, copy=True)
    n = A.shape[0]
    Vt = np.eye(n)
    floor = EPS * float(np.linalg.norm(A)) / np.sqrt(n)
    players = n + (n & 1)
    half = players // 2
    t = np.arange(half)
    sweeps = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = False
        for rd in range(players - 1 if n > 1 else 0):
            a = np.where(t == 0, players - 1, (rd + t) % (players - 1))
            b = (rd + players - 1 - t) % (players - 1)
            p, q = np.minimum(a, b), np.maximum(a, b)
            keep = q < n                                                     # the bye of an odd n
            p, q = p[keep], q[keep]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            go = (np.abs(apq) > 0.5 * EPS * np.sqrt(np.abs(app * aqq))) & (np.abs(apq) > floor)
            if not go.any():
                continue
            rotated = True
            p, q, app, aqq, apq = p[go], q[go], app[go], aqq[go], apq[go]
            with np.errstate(over="ignore"):                                 # (a huge theta: t = 0, no rotation)
                theta = (aqq - app) / (2.0 * apq)
                tt = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            cc, ss = c[:, None], s[:, None]
            for _ in range(2):
                Ap, Aq = A[p, :], A[q, :]
                A[p, :], A[q, :] = cc * Ap - ss * Aq, ss * Ap + cc * Aq
                A = np.ascontiguousarray(A.T)
            A[p, q] = A[q, p] = 0.0
            Vp, Vq = Vt[p, :], Vt[q, :]
            Vt[p, :], Vt[q, :] = cc * Vp - ss * Vq, ss * Vp + cc * Vq
        if not rotated:
            break
    lam = np.diag(A).copy()
    order = np.argsort(-lam, kind="stable")
    return lam[order], np.ascontiguousarray(Vt[order, :].T), sweeps


def lapack_eigh(G):
    """(evals descending, V columns): host route one"""
    lam, V = np.linalg.eigh(G)
    return lam[::-1].copy(), V[:, ::-1].copy()


# The largest figure of judge() (residual, orthogonality, eigenvalue error) that either host route leaves over every case of
# all_cases() except the `null_many` ones.  Measured by tests/test_sym_eig_cases_host.py::test_route_spread, which prints every case and
# asserts that this constant covers them.  The GPU bound is 1000 x this for all three figures.
# Measured 2026-10-21:  python -m pytest tests/test_sym_eig_cases_host.py -s   ->  2.97e-13, the orthogonality of the Jacobi route at
# ('graded', 512, 0) after its 24 sweeps (LAPACK's figures stay below 4e-15).  Stored rounded up to the next half: the matrices come
# from LAPACK's QR, whose last bits depend on the BLAS build and its thread count, and the test must not fail over them; it also
# asserts that the constant is less than twice what it measures.
EIG_ROUTE_SPREAD = 3.5e-13
