"""Cases, restatements, extended-precision references and derived bounds for the compact passes of a coordinate-separable model
(fitter_phases.hip: use_compact): gram_tri_kernel<3, true, 1> over the compact basis, the scatter branch of
phase1_finalize_kernel, posterior_solve_lds_kernel<2> and sweep_fit_boxes_kernel<3, 4, true>.  Plain module, imported by
test_separable_cases_host.py (CPU) and test_gpu_separable_edges.py (GPU).

Restated here, asserted against hand-worked values by the host test:
    compact_plan        gram_compact_plan (gp_gram.hip): the slabs of the compact Gram pass
    sep_map / SepMap    gp.h: class, position and class lists of the dense columns
    column_classes      model.hip, model_detect_separable: a column is of class d when only rows 3 i + d hold anything but +-0.0
    kd_leaf_order       kd_order.h: the device's row order.  line_reference gives clouds whose k-d order is the caller's order, so that
                        "row s of slab b" means the same on the device and here (the host test runs the library's own header on them).

Bounds -- derived, never measured.  u = 2^-53.

G and rhs, per entry (gram_bound, rhs_bound).  The device forms  sum_i (w_i q_ia) q_ib  over the nonzero-weight rows i of a plane:
one rounding for w_i q_ia, then a fused multiply-add per row into one of several accumulators (four lane groups, four K groups, two
steps in flight), the accumulators added up per slab and the nslabs slab partials added up by the finalize kernel.  Whatever the
order, each of the n_rows products passes through at most n_rows + nslabs - 1 additions (Higham, Accuracy and Stability, section 4.2:
any-order summation), and carries the two product roundings; in the CPD flavour w_i = 1 / (sigma2 lambda (1 / P1_i)) adds at most
four roundings of its own to the restated weight (none in the pairs flavour, whose weights are read back from the device).  To
first order that is (n_rows + nslabs + 5) u S_abs, S_abs = sum_i |w_i| |q_ia| |q_ib|; the bound is (n_rows + nslabs + 10) u S_abs,
the remaining 5 u covering the second-order terms (n u < 2e-12 at the largest case).  Zero-weight rows add exact zeros and do not
count.  rhs_a = sum_i q_ia e_i is the same sum with e_i in the place of w_i q_ib (the product is fused: fewer roundings, same bound,
S_abs = sum_i |q_ia| |e_i|) plus the rounding of e itself: obs_points_kernel forms, for the identity pose, e_i = w_i ((o - c - t)
- (ref - c) - mean) with c = t = 0 -- two rounded subtractions and one product, at most 3 u w_i (|o| + |ref| + |mean| + |c|);
obs_cpd_kernel first forms o = y + (PX (1 / P1) - y), four more roundings of at most u (|o| + |y|) each with y = ref + mean to
rounding.  The bound takes E_ULPS = 8 ulp of (|o| + |ref| + |mean| + |c|) for both, times w_i |q_ia|, summed.

Fit, per coordinate (fit_bound).  sweep_fit_boxes_kernel forms ref + mean + sum_k q_k alpha_k over the r_d columns of the
coordinate's class: r_d fused multiply-adds and two additions in some order -- every term passes through at most r_d + 2 roundings --
so |delta| <= (r_d + 3) u (|ref| + |mean| + sum_k |q_k| |alpha_k|) with one u to spare for the second order.  A coordinate whose
class is empty is ref + mean, one rounding: the bit pattern of the float64 sum.
"""
import numpy as np

from tests import posterior_solve_cases as pc

LD = np.longdouble
U53 = 2.0 ** -53
COMPACT_COLS = 48   # kCompactCols (gp.h)
E_ULPS = 8

ROWS = [1, 15, 16, 17, 48, 64, 65, 193, 257, 10881]
COUNTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (16, 16, 16), (17, 15, 16), (33, 32, 1), (48, 1, 0), (0, 48, 48),
          (48, 48, 16), (48, 47, 17), (38, 37, 37)]
ORDERS = ("interleaved", "grouped_201", "random")
BLOCK_SIZES = (0, 1, 2, 15, 16, 17, 31, 33, 47, 48)

have_extended = pc.have_extended
rp_of = pc.rp_of


# ------------------------------------------------------------------------------------------------ slab plan
def compact_plan(M):
    """gram_compact_plan -> (nslabs, rows_per_slab)"""
    want = min(170, max(1, -(-M // 64)))
    rps = -(-(-(-M // want)) // 16) * 16
    return -(-M // rps), rps


def slabs(M):
    """[(first row, one past the last row)] of every slab"""
    n, rps = compact_plan(M)
    return [(b * rps, min(M, (b + 1) * rps)) for b in range(n)]


# ------------------------------------------------------------------------------------------------ classes and SepMap
def column_classes(U):
    """class of every column of the [3 M, r] basis, or None when some column has entries on two coordinates"""
    out = []
    for k in range(U.shape[1]):
        nz = [d for d in range(3) if np.any(U[d::3, k] != 0.0)]  # (-0.0 != 0.0 is false: a signed zero holds nothing)
        if len(nz) > 1:
            return None
        out.append(nz[0] if nz else 0)
    return np.array(out, dtype=np.int64)


class SepMap:
    """gp.h: the index functions of gingr_model::sep_map ([2 rp + 3 kCompactCols] int32)"""

    def __init__(self, rp):
        self.rp = rp

    def cls(self, k):
        return k

    def pos(self, k):
        return self.rp + k

    def col(self, d, p):
        return 2 * self.rp + d * COMPACT_COLS + p

    def total(self):
        return 2 * self.rp + 3 * COMPACT_COLS


def sep_map(classes):
    """the map model_detect_separable uploads: class (-1: padding), position within the class, the three class lists (-1 behind)"""
    r = len(classes)
    sm = SepMap(rp_of(r))
    m = np.full(sm.total(), -1, dtype=np.int32)
    count = [0, 0, 0]
    for k, d in enumerate(classes):
        m[sm.cls(k)], m[sm.pos(k)], m[sm.col(d, count[d])] = d, count[d], k
        count[d] += 1
    return m


def class_columns(classes):
    return [np.flatnonzero(classes == d) for d in range(3)]


# ------------------------------------------------------------------------------------------------ row order
def kd_leaf_order(pts):
    """kd_order.h restated for finite coordinates: perm[s] = caller's index of the point at device position s"""
    def split(idx, leaf):
        n = len(idx)
        if n <= leaf:
            return [idx]
        p = pts[idx]
        ext = p.max(axis=0) - p.min(axis=0)
        ax = 0
        for d in (1, 2):
            if ext[d] > ext[ax]:
                ax = d
        half = ((n // leaf + 1) // 2) * leaf
        if half >= n:
            half = n // 2
        o = idx[np.lexsort((idx, pts[idx, ax]))]
        return split(o[:half], leaf) + split(o[half:], leaf)

    out = []
    for leaf in split(np.arange(pts.shape[0]), 256):
        out += [np.sort(q) for q in split(leaf, 64)]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def line_reference(M, seed=0):
    """(ref, mean): x advances by 3 per point, everything else stays within +-0.6 -- in every node of the k-d tree with two points or
    more x is the longest axis, the median cut is the cut of the index order, and the device keeps the caller's row order."""
    rng = np.random.default_rng(50000 + 7 * M + seed)
    ref = rng.uniform(-0.5, 0.5, (M, 3))
    ref[:, 0] += 3.0 * np.arange(M)
    return ref, rng.uniform(-0.1, 0.1, (M, 3))


# ------------------------------------------------------------------------------------------------ bases
def admits(M, counts):
    """orthonormal columns per class are possible"""
    return M >= max(counts)


def basis(M, counts, order="interleaved", seed=0):
    """(U [3 M, r], lam [r], classes [r]): counts[d] columns on coordinate d, orthonormal per class where M >= max(counts) (plain
    normal columns otherwise), in the given column order.  lam are squares of numbers with ten fractional bits in [4.5, 20], so that
    sqrt(lam) -- and with it Q0 = U sqrt(lam), one rounded product -- is the same float64 on the device and here; descending."""
    assert order in ORDERS
    rng = np.random.default_rng(1 + 1000 * M + 31 * (counts[0] + 49 * counts[1] + 2401 * counts[2]) + seed)
    cols = []
    for d, n in enumerate(counts):
        if not n:
            continue
        q = rng.normal(0, 1, (M, n))
        if admits(M, counts):
            q, _ = np.linalg.qr(q)
        for k in range(n):
            u = np.zeros(3 * M)
            u[d::3] = q[:, k]
            cols.append((k, d, u))
    if order == "interleaved":
        cols.sort(key=lambda c: (c[0], c[1]))
    elif order == "grouped_201":
        cols.sort(key=lambda c: ((2, 0, 1).index(c[1]), c[0]))
    else:
        cols = [cols[i] for i in rng.permutation(len(cols))]
    U = np.ascontiguousarray(np.stack([c[2] for c in cols], axis=1))
    s = np.sort(np.round(rng.uniform(4.5, 20.0, U.shape[1]) * 1024.0) / 1024.0)[::-1]
    return U, np.ascontiguousarray(s * s), np.array([c[1] for c in cols], dtype=np.int64)


def scaled_basis(U, lam):
    """Q0 as pack_basis_kernel forms it"""
    return U * np.sqrt(lam)[None, :]


# ------------------------------------------------------------------------------------------------ pairs of the Gram cases
def marker_pairs(M, seed=0):
    """(pid, var) of the isotropic pairs of a Gram case: variances log-uniform in [1e-6, 1e6]; a third of the vertices without a pair
    (weight exactly 0); with two slabs or more one whole slab without a pair (the second, or the first of two); the first and the last row
    of every other slab carry the smallest variance 1e-6, i.e. the largest weight -- the single row of a last slab among them."""
    rng = np.random.default_rng(70000 + M + seed)
    sl = slabs(M)
    empty = None if len(sl) < 2 else (1 if len(sl) > 2 else 0)
    keep = rng.uniform(0, 1, M) > 1.0 / 3.0
    var = 10.0 ** rng.uniform(-6, 6, M)
    for b, (r0, r1) in enumerate(sl):
        if b == empty:
            keep[r0:r1] = False
        else:
            keep[[r0, r1 - 1]] = True
            var[[r0, r1 - 1]] = 1e-6
    pid = np.flatnonzero(keep).astype(np.int32)
    return pid, var[pid], empty


# ------------------------------------------------------------------------------------------------ references and bounds
def observation_e(w, obs, ref, mean):
    """e_i = w_i (o_i - ref_i - mean_i) of the identity pose with centre and translation 0, in extended precision; 0 where w is 0"""
    e = w.astype(LD)[:, None] * (obs.astype(LD) - ref.astype(LD) - mean.astype(LD))
    e[w == 0.0] = 0.0
    return e


def cpd_weight(P1, sigma2, lam):
    """obs_cpd_kernel's weight, operation by operation in float64"""
    p1inv = 1.0 / P1
    return 1.0 / (sigma2 * lam * p1inv)


def cpd_observation(fit, P1, PX):
    """obs_cpd_kernel's observed point in extended precision: y + (PX / P1 - y) = PX / P1"""
    return np.asarray(PX.astype(LD) / P1.astype(LD)[:, None], dtype=np.float64)


def gram_reference(Q, classes, w, e):
    """G = sum_i w_i Q_i^T Q_i, rhs = Q^T e and their sums over absolute values, all in extended precision.  Class by class over the
    rows with a weight (the rest of the products have a zero factor): entries between the classes are exactly 0."""
    r = Q.shape[1]
    G, rhs, Ga, ra = (np.zeros(s, dtype=LD) for s in ((r, r), r, (r, r), r))
    rows = np.flatnonzero(w)
    wl = w[rows].astype(LD)[:, None]
    for d, cols in enumerate(class_columns(classes)):
        if len(cols) == 0:
            continue
        Qd = Q[3 * rows + d][:, cols].astype(LD)
        ed = e[rows, d].astype(LD)
        G[np.ix_(cols, cols)] = Qd.T @ (wl * Qd)
        Ga[np.ix_(cols, cols)] = np.abs(Qd).T @ (np.abs(wl) * np.abs(Qd))
        rhs[cols] = Qd.T @ ed
        ra[cols] = np.abs(Qd).T @ np.abs(ed)
    return G, rhs, Ga, ra


def gram_bounds(Q, classes, w, e, obs, ref, mean, nslabs, centre=0.0):
    """-> (G, rhs, bound of G [r, r], bound of rhs [r]) (module docstring)"""
    G, rhs, Ga, ra = gram_reference(Q, classes, w, e)
    n_rows = int(np.count_nonzero(w))
    c = (n_rows + nslabs + 10) * U53
    mag = (np.abs(obs) + np.abs(ref) + np.abs(mean) + abs(centre)) * np.abs(w)[:, None]
    mag[w == 0.0] = 0.0
    e_round = np.zeros(Q.shape[1])
    for d, cols in enumerate(class_columns(classes)):
        if len(cols):
            e_round[cols] = E_ULPS * U53 * (np.abs(Q[d::3][:, cols]).T @ mag[:, d])
    return G, rhs, np.asarray(c * Ga, dtype=np.float64), np.asarray(c * ra, dtype=np.float64) + e_round


def fit_reference(ref, mean, Q, alpha, classes):
    """(fit, bound) [M, 3]: ref + mean + Q alpha in extended precision and (r_d + 3) u (|ref| + |mean| + sum |q| |alpha|)"""
    M = ref.shape[0]
    fit = ref.astype(LD) + mean.astype(LD) + (Q.astype(LD) @ alpha.astype(LD)).reshape(M, 3)
    mag = np.abs(ref) + np.abs(mean) + (np.abs(Q) @ np.abs(alpha)).reshape(M, 3)
    rd = np.array([np.count_nonzero(classes == d) for d in range(3)], dtype=np.float64)
    return fit, (rd[None, :] + 3.0) * U53 * mag


# ------------------------------------------------------------------------------------------------ block systems
def block_solve(G, rhs, classes):
    """a [r] of the three uncoupled systems (I + G_dd) a_d = rhs_d, extended precision; entries of G between classes are not read"""
    a = np.zeros(len(classes), dtype=LD)
    for cols in class_columns(classes):
        if len(cols):
            N = np.eye(len(cols), dtype=LD) + G[np.ix_(cols, cols)].astype(LD)
            L = pc.cholesky_left(N)
            a[cols] = pc.backward_sub_t(L, pc.forward_sub(L, rhs[cols].astype(LD)))
    return a


def scatter_blocks(classes, blocks):
    """dense (G [r, r], rhs [r]) with blocks[d] = (G_d, rhs_d) at the positions of class d, zeros between the classes"""
    r = len(classes)
    G, rhs = np.zeros((r, r)), np.zeros(r)
    for cols, blk in zip(class_columns(classes), blocks):
        if len(cols):
            G[np.ix_(cols, cols)] = blk[0]
            rhs[cols] = blk[1]
    return G, rhs


# (family, size) per class; None: an empty class.  Every family once at 48 and once at 17, every size of BLOCK_SIZES, the two mixes.
BLOCK_CASES = [
    (("ill", 48), ("zero", 17), ("graded_up", 47)),
    (("diagonal", 48), ("graded_down", 17), ("well", 47)),
    (("zero", 48), ("ill", 17), ("well", 16)),
    (("graded_up", 48), ("diagonal", 17), ("graded_down", 31)),
    (("well", 48), ("graded_up", 17), ("ill", 33)),
    (("graded_down", 48), ("well", 17), ("zero", 15)),
    (("well", 2), None, ("ill", 1)),
    (None, ("graded_down", 33), ("diagonal", 2)),
    (("graded_up", 1), ("zero", 2), None),
    (("ill", 15), ("zero", 16), ("graded_up", 31)),
    (("diagonal", 33), ("graded_down", 47), ("well", 1)),
]


def block_counts(case):
    return tuple(0 if c is None else c[1] for c in case)
