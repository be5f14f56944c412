"""Inputs, guards, reference and restatements for the element-wise tests of the table exponential (gingr_amd/csrc/fastexp.h).  No
tests in here; test_fastexp_host.py checks tables, constants, guards and restatements on the CPU, test_gpu_fastexp.py runs the
same inputs through `Context.gauss_block` (degree 3, round to nearest) and `Context.cpd_stats` (floor form, round toward -inf).

REFERENCE.  The kernels evaluate 2^(u / 2048) with u = d2 * c, d2 and c float64.  `reference` computes that for the EXACT rational
u with the standard library's `decimal` at 70 digits and returns it as an unevaluated pair hi + lo of float64 (hi the correctly
rounded value, gradual underflow included; lo the rest), so that a relative error of 1e-16 can be formed in numpy.  c is restated
bit for bit (`c_gauss`, `c_cpd`).  Nothing in here depends on device output.

EXACT-ARGUMENT INPUTS.  One point sits at the origin (the row-statistics test moves everything by a lattice vector), the others
have coordinates (integer with at most 26 significant bits) * 2^p: differences, squares and the three-term sum are exact in
every rounding mode (`exact_d2` asserts that every square and every partial sum is a float64), so d2 is known exactly.
  * floor form: sigma2 = log2(e) / 4, hence c = -2^12 exactly, coordinates on the 2^-16 lattice: u = -n / 2^20 with n = a^2 + b^2 +
    c^2, so floor(u) = -q and the fraction f = g / 2^20 are chosen freely as n = q 2^20 - g (`three_squares` finds a, b, c; the
    numerators it finds no representation for are skipped, and the guards below count what is left).
  * degree 3: sigma = 1/2, hence c = -log2(e) 2^13 (a 53-bit number), coordinates on the 2^-14 lattice: u = -n log2(e) / 2^15, a
    step of 4.4e-5 in u; n is the integer nearest to the wanted u, and (k, f) = (rint(u), u - k) are computed exactly from it.

GUARDS (`guards_nearest`, `guards_floor`) are evaluated on the inputs alone, and both test modules assert them: every table index,
both ends of the reduced argument, the exponent carry across j = 2047 -> 0, d2 = 0, the normal / subnormal border, the subnormal
range, the flush to +0, the clamp.

RESTATEMENTS.  `restate_nearest` is fastexp2_scaled<3> behind gauss_block_kernel's clamp, `restate_floor` is
fastexp2_floor_scaled with every operation rounded toward -inf, both from fractions.Fraction (float(Fraction) is correctly
rounded; the round-down result is that value, stepped down when it exceeds the exact one) with the tables read from the .inc
files and the constants parsed from the header.

GENERIC CLOUDS (`generic_clouds`, `pair_matrix`, `rows_reference`): coordinates that are no lattice points, for the norm-expansion
form of the CPD passes, scaled to a chosen value of use_expansion's figure; the reference uses the exact squared distance of the
float64 coordinates."""
from __future__ import annotations

import dataclasses
import decimal
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gingr_amd", "csrc")

LOG2E = 1.4426950408889634074          # the literal of fastexp_scale_for_variance: the same float64
TAB = 2048
TWO = Fraction(2)

# ------------------------------------------------------------------------------------------------------------------ bounds
# Derived from the header's constants and IEEE rounding, never from what the kernels return.
ULPS_NEAREST = 1.0                      # fastexp.h: degree 3, "<= 1 ulp of the correctly rounded result of its argument"
POLY3_BOUND = 3.5e-17                   # largest relative error of 1 + f (C1 + f (C2 + f C3)) on |f| <= 1/2 (3.42e-17)
POLY2_BOUND = 2.02e-13                  # ... of the economised degree-2 form on |f| <= 1/2 (2.0194e-13)
POLYF_BOUND = 2.03e-13                  # ... of S (1 + f (Q0 + Q1 f)) on [0, 1) (2.0203e-13)
# one K of the floor form from an exact argument: the polynomial (2.0203e-13), the table entry (fl(T[j] S) against T[j] S with T[j]
# correctly rounded: 2 * 2^-53 = 2.2e-16) and the two roundings toward -inf that matter (the final FMA and the sum into a zero
# accumulator: 2^-52 each; those of q and f q are scaled by f q <= 3.4e-4): 2.0203e-13 + 2.2e-16 + 4.4e-16 < 2.03e-13
REL_FLOOR = 2.03e-13
ARG_ROUNDINGS = 1.6e-15                 # generic coordinates: seven roundings at 2^-52 of the argument, times |ln K|
EXPAND_TOL = 1e-12                      # cpd_pairs.hip: kExpandTol, the budget use_expansion exists to enforce
TINY = 2.0 ** -1074


# ------------------------------------------------------------------------------------------------- the header and the tables
_HEX = r"-?0x[0-9a-fA-F]+\.?[0-9a-fA-F]*p[+-]?\d+"


def parse_table(name):
    """the float64 entries of an .inc file; comment lines are skipped (the floor table's header comment holds a hex literal)"""
    vals = []
    with open(os.path.join(CSRC, name)) as fh:
        for line in fh:
            if line.lstrip().startswith("//"):
                continue
            vals.extend(float.fromhex(h) for h in re.findall(_HEX, line))
    return vals


@functools.lru_cache(maxsize=None)
def header():
    """name -> float64: the polynomial constants, S and the two magic numbers of fastexp.h"""
    with open(os.path.join(CSRC, "fastexp.h")) as fh:
        text = fh.read()
    out = {}
    for name in ("C1", "C2", "C3", "C1_D2", "Q0", "Q1"):
        m = re.findall(r"static constexpr double %s = ([0-9.eE+-]+);" % name, text)
        assert len(m) == 1, name
        out[name] = float(m[0])
    m = re.findall(r"static constexpr double S = (%s);" % _HEX, text)
    assert len(m) == 1
    out["S"] = float.fromhex(m[0])
    for name in ("GINGR_EXP_MAGIC", "GINGR_EXP_MAGIC8"):
        m = re.findall(r"#define %s ([0-9.]+)" % name, text)
        assert len(m) == 1, name
        out[name] = float(m[0])
    return out


@functools.lru_cache(maxsize=None)
def tables():
    return tuple(parse_table("exp_table.inc")), tuple(parse_table("exp_floor_table.inc"))


# ------------------------------------------------------------------------------------------------------------- the scale c
def c_gauss(sigma):
    """gauss_block_kernel: fastexp_scale_for_variance(sigma * sigma) = -(2048 log2 e) / (sigma sigma)"""
    return (-2048.0 * LOG2E) / (sigma * sigma)


def c_cpd(sigma2):
    """cpd_colsum_kernel / cpd_rowstats_kernel: fastexp_scale_for_variance(2 sigma2)"""
    return (-2048.0 * LOG2E) / (2.0 * sigma2)


def d2_limit(c):
    """fastexp_d2_limit"""
    return (-1100.0 * 2048.0) / c


SIGMA_GAUSS = 0.5
P_GAUSS = -14                                   # lattice of the degree-3 sweep
SIGMA2_CPD = LOG2E * 0.5 / 2.0                  # m = 1: c = -2^12
P_CPD = -16                                     # lattice of the floor sweep: u = -n / 2^20
G = 1 << 20


# ----------------------------------------------------------------------------------------------------- three-square search
def _isqrt(n):
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r -= (r * r > n)
    r += ((r + 1) * (r + 1) <= n)
    return r


def three_squares(n, tries_a=40, tries_b=80):
    """n: non-negative int64.  (a, b, c, found) with a^2 + b^2 + c^2 = n where found: factors of 4 are stripped first, then a runs
    down from isqrt(n), b down from isqrt(n - a^2), and the rest has to be a square."""
    n = np.asarray(n, dtype=np.int64)
    m, shift = n.copy(), np.zeros(n.shape, dtype=np.int64)
    for _ in range(32):
        strip = (m > 0) & (m % 4 == 0)
        m = np.where(strip, m // 4, m)
        shift += strip
    a0 = _isqrt(m)
    out = np.zeros((3,) + n.shape, dtype=np.int64)
    found = np.zeros(n.shape, dtype=bool)
    for s in range(tries_a):
        todo = np.nonzero(~found & (a0 - s >= 0))[0]
        if todo.size == 0:
            break
        a = a0[todo] - s
        r1 = m[todo] - a * a
        b0 = _isqrt(r1)
        for t in range(tries_b):
            b = b0 - t
            r2 = r1 - b * b
            c = _isqrt(np.maximum(r2, 0))
            hit = (b >= 0) & (c * c == r2) & ~found[todo]
            if hit.any():
                idx = todo[hit]
                out[0, idx], out[1, idx], out[2, idx] = a[hit], b[hit], c[hit]
                found[idx] = True
    out = out << shift[None]
    assert np.all((out[0] ** 2 + out[1] ** 2 + out[2] ** 2 == n) | ~found)
    return out[0], out[1], out[2], found


def representable(n):
    """Legendre: n is a sum of three squares unless it is 4^k (8 l + 7)"""
    while n > 0 and n % 4 == 0:
        n //= 4
    return n % 8 != 7


def _odd_not_1_mod_8(g):
    """g made odd and != 1 mod 8: q 2^20 - g is then odd and != 7 mod 8, a sum of three squares whatever q is"""
    g |= 1
    return g + 2 if g % 8 == 1 else g


def _lattice_points(n, p, rng):
    """points (a, b, c) 2^p with a^2 + b^2 + c^2 = n, coordinates in a random order with random signs (the cloud's centroid stays
    near the origin); the numerators without a representation are dropped"""
    a, b, c, found = three_squares(np.array(n, dtype=np.int64))
    abc = np.stack([a, b, c], axis=1)[found]
    abc = np.take_along_axis(abc, np.argsort(rng.random(abc.shape), axis=1), axis=1) * rng.choice([-1, 1], abc.shape)
    assert np.abs(abc).max() < (1 << 26)
    return np.ascontiguousarray(abc.astype(np.float64) * 2.0 ** p)


def exact_d2(points, origin=(0.0, 0.0, 0.0)):
    """the squared distances of the points from `origin` as Fractions; asserts that gauss_block_kernel's and the pair passes'
    float64 evaluation fma(dz, dz, fma(dy, dy, dx dx)) is exact at every step (then it is in every rounding mode)"""
    out = []
    for row in np.asarray(points, dtype=np.float64):
        d = [Fraction(float(v)) - Fraction(float(o)) for v, o in zip(row, origin)]
        s1, s2 = d[0] * d[0], d[0] * d[0] + d[1] * d[1]
        s3 = s2 + d[2] * d[2]
        for v in d + [s1, s2, s3]:
            assert Fraction(float(v)) == v, "not a float64"
        out.append(s3)
    return out


# ------------------------------------------------------------------------------------------------------------- the reference
_CTX = decimal.Context(prec=70, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_LN2 = _CTX.ln(decimal.Decimal(2))


def exp2_exact(U):
    """2^(U / 2048) for a Fraction U as a Fraction good to 1e-68 relative (None below 2^-1200: beyond every float64)"""
    e = math.floor(U / TAB)
    if e < -1200:
        return None
    r = U - TAB * e                                                   # in [0, 2048)
    x = _CTX.divide(decimal.Decimal(r.numerator), decimal.Decimal(r.denominator))
    y = _CTX.exp(_CTX.multiply(_CTX.divide(x, decimal.Decimal(TAB)), _LN2))
    return Fraction(y) * TWO ** e


LO_BELOW, LO_SHIFT = 2.0 ** -600, 400       # lo is stored times 2^400 where hi < 2^-600: it would underflow otherwise


def reference(d2, c):
    """d2: Fractions, c: float64.  (U, hi, lo, below): U = d2 c exactly, hi + lo = 2^(U / 2048) with hi correctly rounded (lo scaled
    by 2^LO_SHIFT where hi < LO_BELOW), below: the exact value is under 2^-1075 (a correctly rounded or rounded-down result is +0)"""
    cf = Fraction(c)
    U, hi, lo, below = [], np.zeros(len(d2)), np.zeros(len(d2)), np.zeros(len(d2), dtype=bool)
    for i, d in enumerate(d2):
        u = d * cf
        U.append(u)
        v = exp2_exact(u)
        if v is None:
            below[i] = True
            continue
        hi[i] = float(v)
        lo[i] = float((v - Fraction(hi[i])) * TWO ** (LO_SHIFT if hi[i] < LO_BELOW else 0))
        below[i] = v < TWO ** -1075
    for a in (hi, lo, below):
        a.setflags(write=False)
    return U, hi, lo, below


def rel_error(got, hi, lo, units=1.0, everywhere=False):
    """|got - (hi + lo)| / hi, after `units` of 2^-1074 have been taken off the difference where hi is below 2^-1022 (the
    result's own rounding in the subnormal range), or `everywhere` (a sum of terms K / den with tiny den: what a K loses at the
    underflow is no longer tiny in the quotient).  got - hi is exact for neighbours, and small results are compared times
    2^LO_SHIFT.  Where hi = 0 the figure is in units of 2^-1074."""
    got = np.asarray(got, dtype=np.float64)
    k = np.where(hi < LO_BELOW, LO_SHIFT, 0)
    diff = np.abs(np.ldexp(got - hi, k) - lo) - np.where((hi < 2.0 ** -1022) | everywhere, np.ldexp(units, k - 1074), 0.0)
    return np.maximum(diff, 0.0) / np.ldexp(np.maximum(hi, TINY), k)


def ulp_error(got, hi):
    """|got - hi| in units of the last place of hi (2^-1074 in the subnormal range and at 0)"""
    got = np.asarray(got, dtype=np.float64)
    return np.abs(got - hi) / np.maximum(np.spacing(np.abs(hi)), TINY)


# ----------------------------------------------------------------------------------------------------------------- the sweeps
@dataclasses.dataclass(frozen=True)
class Sweep:
    """points[i] at squared distance d2[i] (exact) from the origin; U = d2 c; hi + lo the exact 2^(U / 2048)"""
    points: np.ndarray
    c: float
    d2: tuple
    U: tuple
    hi: np.ndarray
    lo: np.ndarray
    below: np.ndarray

    def __len__(self):
        return self.points.shape[0]


def _make_sweep(points, c, extra=()):
    points = np.ascontiguousarray(np.concatenate([points] + [np.atleast_2d(e) for e in extra])) if len(extra) else points
    points.setflags(write=False)
    d2 = exact_d2(points)
    U, hi, lo, below = reference(d2, c)
    return Sweep(points, c, tuple(d2), tuple(U), hi, lo, below)


def _floor_targets(rng):
    """(q, g): u = -q + g / 2^20, i.e. floor(u) = -q, f = g / 2^20, n = q 2^20 - g"""
    T = [(0, 0)]                                                           # d2 = 0
    for j in range(TAB):                                                   # every table index, twice, anywhere down to 2^-1074
        for _ in range(2):
            e = int(rng.integers(-1074, 0))
            T.append((-(e * TAB + j), _odd_not_1_mod_8(int(rng.integers(1, G - 8)))))
    for _ in range(96):                                                    # both ends of [0, 1)
        T.append((int(rng.integers(1, 1074 * TAB)), 0))
        T.append((int(rng.integers(1, 1074 * TAB)), G - 1))
    for E in (1, 2, 3, 100, 1021, 1022, 1023, 1050, 1074):                 # exact powers of two
        T.append((E * TAB, 0))
    for E in (1, 2, 7, 512, 1021, 1022, 1023, 1073):                       # the carry: j = 2047 of exponent -(E + 1), j = 0 of -E
        for q in (E * TAB + 1, E * TAB):
            for g in (0, 1, G // 2, G // 2 + 1, G - 1, G - 2):
                T.append((q, g))
    for dq in range(-2, 4):                                                # 2^-1022 (1 +- 2^-10): |u + 1022 * 2048| <= 2.884
        for g in (0, 1, G - 1) + tuple(int(v) for v in rng.integers(1, G, 6)):
            T.append((1022 * TAB + dq, g))
    for _ in range(128):                                                   # the subnormal range
        T.append((int(rng.integers(1022 * TAB + 1, 1074 * TAB)), int(rng.integers(0, G))))
    for _ in range(64):                                                    # within a factor 2 of 2^-1074
        T.append((int(rng.integers(1073 * TAB + 1, 1075 * TAB)), int(rng.integers(0, G))))
    for g in (0, 1, G - 1):                                                # 2^-1075 itself (a tie: to even, and down, is +0) and next to it
        T.append((1075 * TAB, g))
        T.append((1075 * TAB + 1, g))
    for _ in range(64):                                                    # (2^-1100, 2^-1075): +0
        T.append((int(rng.integers(1075 * TAB + 1, 1100 * TAB)), int(rng.integers(0, G))))
    T.append((1100 * TAB, 0))                                              # fastexp_d2_limit exactly ...
    for k in range(1, 9):                                                  # ... the next lattice values above it ...
        T.append((1100 * TAB + 1, G - k))
    for _ in range(16):                                                    # ... and beyond
        T.append((int(rng.integers(1100 * TAB + 1, 1110 * TAB)), int(rng.integers(0, G))))
    return T


def _big26(v):
    """the float64 with 26 significant bits next above v"""
    m, e = math.frexp(v)
    return math.ldexp(math.ceil(m * (1 << 26)), e - 26)


FAR_CLAMPED = ((65536.0, 0.0, 0.0), (0.0, -65536.0, 32768.0), (0.0, 0.0, _big26(1e150)))   # d2 |c| > 2^42; d2 >= 1e300


@functools.lru_cache(maxsize=None)
def floor_sweep(clamped=False):
    """The sweep of the floor form (about 4 800 points).  clamped: three far points are appended, which put the CPD passes into
    their clamped regime (3 am^2 |c| >= 2^41) and whose own arguments lie past 2^42 and at d2 >= 1e300."""
    rng = np.random.default_rng(2048)
    n = [q * G - g for q, g in _floor_targets(rng)]
    pts = _lattice_points(n, P_CPD, rng)
    c = c_cpd(SIGMA2_CPD)
    assert c == -4096.0
    return _make_sweep(pts, c, FAR_CLAMPED if clamped else ())


def _nearest_targets(rng):
    """(K, t, copies): u near K + t"""
    T = [(0, 0.0, 1)]
    for j in range(TAB):
        for _ in range(2):
            e = int(rng.integers(-1074, 0))
            T.append((e * TAB + j, float(rng.uniform(-0.45, 0.45)), 1))
    for _ in range(96):                                                    # |f| >= 0.499, both signs, and |f| <= 1e-3
        for t in (0.4995, -0.4995, float(rng.uniform(-5e-4, 5e-4))):
            T.append((-int(rng.integers(1, 1074 * TAB)), t, 2))
    for E in (1, 2, 7, 512, 1021, 1022, 1023, 1073):                       # the carry, approached from both sides of the tie
        for K in (-E * TAB - 1, -E * TAB):
            for t in (-0.4995, -0.3, 0.0, 0.3, 0.4995):
                T.append((K, t, 2))
    for dK in range(-2, 3):                                                # 2^-1022 (1 +- 2^-10)
        for t in (-0.4995, 0.4995) + tuple(float(v) for v in rng.uniform(-0.45, 0.45, 6)):
            T.append((-1022 * TAB + dK, t, 1))
    for _ in range(128):
        T.append((-int(rng.integers(1022 * TAB + 1, 1074 * TAB)), float(rng.uniform(-0.5, 0.5)), 1))
    for _ in range(64):
        T.append((-int(rng.integers(1073 * TAB + 1, 1075 * TAB)), float(rng.uniform(-0.5, 0.5)), 1))
    for t in (-0.01, -1e-4, 1e-4, 0.01):                                   # either side of 2^-1075
        T.append((-1075 * TAB, t, 2))
    for _ in range(64):
        T.append((-int(rng.integers(1075 * TAB + 1, 1100 * TAB)), float(rng.uniform(-0.5, 0.5)), 1))
    for t in (-0.4, -0.01, -1e-4):                                         # just under the clamp (above it: `clamp_points`)
        T.append((-1100 * TAB + 1, t, 2))
    return T


def clamp_points(c):
    """Points whose float64 d2 is fastexp_d2_limit(c) EXACTLY (x and y found so that fl(fma(y, y, fl(x x))) hits it: generic
    coordinates, evaluated as the kernel does in round to nearest), one with d2 the next float64 above it, and points far beyond:
    d2 |c| > 2^42, d2 >= 1e300.  Returns (points, d2 as the kernel forms it)."""
    lim = d2_limit(c)
    pts, d2 = [], []

    def kernel_d2(x, y):
        return float(Fraction(y) * Fraction(y) + Fraction(x * x))          # one FMA on top of the rounded square

    for want in (lim, math.nextafter(lim, math.inf)):
        x = math.sqrt(want) * 0.8
        for _ in range(4096):
            rest = Fraction(want) - Fraction(x * x)
            y = math.sqrt(float(rest))
            hit = [yy for yy in (math.nextafter(y, 0.0), y, math.nextafter(y, math.inf)) if kernel_d2(x, yy) == want]
            if hit:
                pts.append((x, hit[0], 0.0))
                d2.append(want)
                break
            x = math.nextafter(x, math.inf)
    big = _big26(1e150)
    far = math.ldexp(1.0, 22)
    assert far * far * -c > 2.0 ** 42
    for p in ((far, 0.0, 0.0), (0.0, 0.0, -big)):
        pts.append(p)
        d2.append(p[0] * p[0] + p[2] * p[2])
    return np.array(pts), d2


@functools.lru_cache(maxsize=None)
def nearest_sweep():
    """The sweep of the degree-3 form (about 3 500 points), the points of `clamp_points` at its end"""
    rng = np.random.default_rng(11)
    c = c_gauss(SIGMA_GAUSS)
    assert Fraction(c) == -Fraction(LOG2E) * 2 ** 13
    step = -Fraction(c) * TWO ** (2 * P_GAUSS)                             # u = -n step
    n = []
    for K, t, copies in _nearest_targets(rng):
        n0 = round((-(Fraction(K) + Fraction(t))) / step)
        n.extend([v for v in (n0, n0 + 1, n0 - 1, n0 + 2, n0 - 2) if v >= 0 and representable(v)][:copies])
    pts = _lattice_points(sorted(set(n)), P_GAUSS, rng)
    cp, cd2 = clamp_points(c)
    d2 = exact_d2(pts) + [Fraction(v) for v in cd2]
    points = np.ascontiguousarray(np.concatenate([pts, cp]))
    points.setflags(write=False)
    U, hi, lo, below = reference(d2, c)
    return Sweep(points, c, tuple(d2), tuple(U), hi, lo, below), len(cd2)


# ------------------------------------------------------------------------------------------------------------------- guards
def _range_counts(U):
    """how many arguments put the exact result into each of the ranges the tests are about"""
    x = [u / TAB for u in U]                                               # log2 of the result
    edge = Fraction(math.log2(1.0 + 2.0 ** -10))
    return {
        "one": sum(u == 0 for u in U),
        "normal_border": sum(abs(v + 1022) <= edge for v in x),
        "border_above": sum(0 <= v + 1022 <= edge for v in x),
        "border_below": sum(-edge <= v + 1022 < 0 for v in x),
        "subnormal": sum(-1074 <= v < -1022 for v in x),
        "near_tiny": sum(-1075 < v < -1073 for v in x),
        "flushed": sum(-1100 < v < -1075 for v in x),
        "at_limit": sum(v == -1100 for v in x),
        "past_limit": sum(v < -1100 for v in x),
    }


def guards_floor(sweep):
    """name -> bool, from the inputs of a floor sweep alone"""
    kf = [(math.floor(u), u - math.floor(u)) for u in sweep.U if u > -(2 ** 42)]
    js = {k % TAB for k, _ in kf}
    ks = {k for k, _ in kf}
    r = _range_counts(sweep.U)
    lim = Fraction(d2_limit(sweep.c))
    above = sorted(d for d in sweep.d2 if d > lim)
    return {
        "every table index": js == set(range(TAB)),
        "f = 0": sum(f == 0 for _, f in kf) >= 64,
        "f >= 1 - 2^-20": sum(f >= 1 - Fraction(1, G) for _, f in kf) >= 64,
        "carry 2047 -> 0": sum((k % TAB == TAB - 1) and (k + 1 in ks) for k in ks) >= 8,
        "d2 = 0": r["one"] == 1,
        "2^-1022 (1 +- 2^-10)": r["border_above"] >= 8 and r["border_below"] >= 8,
        "subnormal": r["subnormal"] >= 128,
        "within 2 of 2^-1074": r["near_tiny"] >= 32,
        "(2^-1100, 2^-1075)": r["flushed"] >= 32,
        "at fastexp_d2_limit": r["at_limit"] == 1 and lim in sweep.d2,
        "one step above it": bool(above) and above[0] - lim == TWO ** (2 * P_CPD),
        "past it": r["past_limit"] >= 16,
    }


def guards_floor_clamped(sweep):
    """what the three far points add"""
    big = [d for d in sweep.d2 if d * -Fraction(sweep.c) > 2 ** 42]
    return {"d2 |c| > 2^42": len(big) == 3, "d2 >= 1e300": any(d >= Fraction(1e300) for d in big)}


def guards_nearest(sweep, n_clamp):
    kf = [(round(u), u - round(u)) for u in sweep.U[:len(sweep) - n_clamp]]
    js = {k % TAB for k, _ in kf}
    ks = {k for k, _ in kf}
    r = _range_counts(sweep.U)
    lim = Fraction(d2_limit(sweep.c))
    tail = sweep.d2[len(sweep) - n_clamp:]
    return {
        "every table index": js == set(range(TAB)),
        "f >= 0.499": sum(f >= Fraction(499, 1000) for _, f in kf) >= 64,
        "f <= -0.499": sum(f <= -Fraction(499, 1000) for _, f in kf) >= 64,
        "|f| <= 1e-3": sum(abs(f) <= Fraction(1, 1000) for _, f in kf) >= 64,
        "carry 2047 -> 0": sum((k % TAB == TAB - 1) and (k + 1 in ks) for k in ks) >= 8,
        "d2 = 0": r["one"] == 1,
        "2^-1022 (1 +- 2^-10)": r["border_above"] >= 8 and r["border_below"] >= 8,
        "subnormal": r["subnormal"] >= 128,
        "within 2 of 2^-1074": r["near_tiny"] >= 32,
        "(2^-1100, 2^-1075)": r["flushed"] >= 32,
        "at fastexp_d2_limit": tail[0] == lim,
        "one step above it": tail[1] == Fraction(math.nextafter(float(lim), math.inf)),
        "d2 |c| > 2^42": tail[2] * -Fraction(sweep.c) > 2 ** 42,
        "d2 >= 1e300": tail[3] >= Fraction(1e300),
    }


# ------------------------------------------------------------------------------------------------------------- restatements
def _rn(v):
    return float(v)


def _rd(v):
    x = float(v)
    return math.nextafter(x, -math.inf) if Fraction(x) > v else x


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def restate_nearest(d2, c):
    """gauss_block_kernel's clamp and fastexp2_scaled<3>, every operation rounded to nearest"""
    h, (T, _) = header(), tables()
    lim = d2_limit(c)
    d2 = lim if d2 > lim else d2
    u = Fraction(d2) * Fraction(c)
    magic = h["GINGR_EXP_MAGIC"]
    tm = _rn(u + Fraction(magic))
    kf = tm - magic
    f = _rn(u - Fraction(kf))
    b = _bits(tm)
    e, j = _int32(b >> 11), b & (TAB - 1)
    q = _rn(Fraction(f) * Fraction(h["C3"]) + Fraction(h["C2"]))
    q = _rn(Fraction(f) * Fraction(q) + Fraction(h["C1"]))
    fq = f * q
    r = _rn(Fraction(T[j]) * Fraction(fq) + Fraction(T[j]))
    return _rn(Fraction(r) * TWO ** e)


def restate_floor(d2, c, clamp=False):
    """fastexp2_floor_scaled (behind fastexp_clamp_d2 in the CLAMP instances), every operation rounded toward -inf"""
    h, (_, T) = header(), tables()
    lim = d2_limit(c)
    if clamp and d2 > lim:
        d2 = lim
    magic = h["GINGR_EXP_MAGIC8"]
    u = _rd(Fraction(d2) * Fraction(c))
    tm = _rd(Fraction(u) + Fraction(magic))
    f = min(_rd(Fraction(u) - math.floor(Fraction(u))), 1.0 - 2.0 ** -53)      # v_fract_f64
    b = _bits(tm)
    e, j = _int32(b >> 14), (b & 0x3FF8) >> 3
    q = _rd(Fraction(f) * Fraction(h["Q1"]) + Fraction(h["Q0"]))
    fq = _rd(Fraction(f) * Fraction(q))
    r = _rd(Fraction(T[j]) * Fraction(fq) + Fraction(T[j]))
    return _rd(Fraction(r) * TWO ** e)


# --------------------------------------------------------------------------------------- polynomials with exact coefficients
def poly_errors(samples=4096):
    """largest relative error of the three polynomials of fastexp.h against 2^(f / 2048), coefficients taken as the exact rationals
    the header's float64 constants are, evaluated in 70-digit decimal on a grid with both ends of the interval"""
    h = header()
    worst = {"deg3": decimal.Decimal(0), "deg2": decimal.Decimal(0), "floor": decimal.Decimal(0)}
    with decimal.localcontext(_CTX):
        D = {k: decimal.Decimal(Fraction(v).numerator) / decimal.Decimal(Fraction(v).denominator) for k, v in h.items()}
        a = _LN2 / TAB
        for i in range(samples + 1):
            f = decimal.Decimal(i) / samples - decimal.Decimal("0.5")
            exact = (a * f).exp()
            worst["deg3"] = max(worst["deg3"], abs((1 + f * (D["C1"] + f * (D["C2"] + f * D["C3"]))) / exact - 1))
            worst["deg2"] = max(worst["deg2"], abs((1 + f * (D["C1_D2"] + f * D["C2"])) / exact - 1))
            g = decimal.Decimal(i) / samples
            worst["floor"] = max(worst["floor"], abs(D["S"] * (1 + g * (D["Q0"] + g * D["Q1"])) / (a * g).exp() - 1))
    return {k: float(v) for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------- generic clouds (expansion)
def expansion_figure(fit, target, sigma2):
    """use_expansion's ratio 3 rmax^2 |c| ln2 / 2048 times its constant 7.7e-16 (expansion form while that is below 1e-12); rmax is
    the largest |coordinate - target centroid| of either cloud"""
    ctr = target.mean(axis=0)
    rmax = max(float(np.abs(target - ctr).max()), float(np.abs(fit - ctr).max()))
    return 3.0 * rmax * rmax * -c_cpd(sigma2) * (0.69314718055994530942 / 2048.0) * 7.7e-16


@functools.lru_cache(maxsize=None)
def generic_clouds(figure, rows):
    """(fit, target, sigma2 = 1) with generic coordinates, scaled so that `expansion_figure` is `figure`.  The cloud: 1 500 points
    uniform in a cube, a quarter of them within a fifth of its half-width of the corner P (there the norm expansion cancels most:
    both norms are of the order of 3 rmax^2 while K is of order 1).  rows = False (column sums): fit = {P}, target = the cloud.
    rows = True (row statistics): fit = the cloud, target = {P, -P}, whose centroid is the cube's centre.  The same cloud for every
    figure, up to the scale."""
    rng = np.random.default_rng(77)
    half = 27.0
    cloud = rng.uniform(-half, half, (1500, 3))
    corner = np.array([half, -half, half]) * 0.985
    cloud[:375] = corner + rng.uniform(-6.0, 6.0, (375, 3))
    cloud = np.clip(cloud, -half, half)
    fit, target = (cloud, np.stack([corner, -corner])) if rows else (corner[None], cloud)
    scale = math.sqrt(figure / expansion_figure(fit, target, 1.0))
    fit, target = np.ascontiguousarray(fit * scale), np.ascontiguousarray(target * scale)
    fit.setflags(write=False)
    target.setflags(write=False)
    return fit, target, 1.0


def exp2_decimal(U):
    """2^(U / 2048) for a Fraction U as a 70-digit Decimal (0 below 2^-1200)"""
    e = math.floor(U / TAB)
    if e < -1200:
        return decimal.Decimal(0)
    r = U - TAB * e
    x = _CTX.divide(decimal.Decimal(r.numerator), decimal.Decimal(r.denominator))
    y = _CTX.exp(_CTX.multiply(_CTX.divide(x, decimal.Decimal(TAB)), _LN2))
    return _CTX.multiply(y, _CTX.power(decimal.Decimal(2), decimal.Decimal(e)))


def split(values):
    """Decimals -> (hi, lo) float64 arrays in the convention of `reference`"""
    hi, lo = np.zeros(len(values)), np.zeros(len(values))
    two_shift = decimal.Decimal(2) ** LO_SHIFT
    for i, v in enumerate(values):
        hi[i] = float(v)
        rest = _CTX.subtract(v, decimal.Decimal(hi[i]))
        lo[i] = float(_CTX.multiply(rest, two_shift) if hi[i] < LO_BELOW else rest)
    return hi, lo


def join(hi, lo):
    """the inverse of `split`"""
    two_shift = decimal.Decimal(2) ** LO_SHIFT
    return [_CTX.add(decimal.Decimal(float(h)), _CTX.divide(decimal.Decimal(float(l)), two_shift) if h < LO_BELOW else decimal.Decimal(float(l)))
            for h, l in zip(hi, lo)]


def pair_matrix(fit, target, sigma2):
    """K[i][j] = exp(-|fit_i - target_j|^2 / (2 sigma2)) as Decimals, from the EXACT squared distance of the float64 coordinates and c
    as the kernels form it; and |ln K| as a float64 array"""
    cf = Fraction(c_cpd(sigma2))
    F = [[Fraction(float(v)) for v in row] for row in fit]
    X = [[Fraction(float(v)) for v in row] for row in target]
    K, lnk = [], np.zeros((len(F), len(X)))
    for i, a in enumerate(F):
        row = []
        for j, b in enumerate(X):
            u = sum((p - q) ** 2 for p, q in zip(a, b)) * cf
            lnk[i, j] = float(-u) * (math.log(2.0) / TAB)
            row.append(exp2_decimal(u))
        K.append(row)
    return K, lnk


def rows_reference(K, elem_bound):
    """K: [M][N] Decimals; elem_bound: [M, N] relative bounds of the single K_ij.  Returns den [N] Decimals (the column sums),
    (hi, lo) of P1_i = sum_j K_ij / den_j, and the bound of P1_i that follows: every den_j inherits the K-weighted mean of its
    elements' bounds plus M 2^-52 for its M additions (toward -inf), every term of P1_i its element's bound plus den_j's."""
    M, N = len(K), len(K[0])
    with decimal.localcontext(_CTX):
        den = [sum((K[i][j] for i in range(M)), decimal.Decimal(0)) for j in range(N)]
        terms = [[K[i][j] / den[j] for j in range(N)] for i in range(M)]
        P1 = [sum(t, decimal.Decimal(0)) for t in terms]
    Kf = np.array([[float(v) for v in row] for row in K])
    denf = np.array([float(v) for v in den])
    den_bound = (Kf * elem_bound).sum(axis=0) / denf + M * 2.0 ** -52
    tf = np.array([[float(v) for v in row] for row in terms])
    each = elem_bound + den_bound[None]
    with np.errstate(divide="ignore", invalid="ignore"):                     # the weights of rows near the underflow are not formed
        p1_bound = np.where(tf.sum(axis=1) > 1e-290, (tf / tf.sum(axis=1, keepdims=True) * each).sum(axis=1), each.max(axis=1))
    hi, lo = split(P1)
    return den, hi, lo, p1_bound
