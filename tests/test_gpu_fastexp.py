"""The table exponential (gingr_amd/csrc/fastexp.h) element by element on the device, against a 70-digit reference of 2^(d2 c / 2048)
for the exact float64 operands the kernels form (tests/fastexp_cases.py: inputs, guards, reference, bounds; test_fastexp_host.py
checks all of that, and Python restatements of the arithmetic, on the CPU).

  * degree 3, round to nearest: `Context.gauss_block(origin, points, 1/2, 1)`, one row, every element a single exponential;
  * floor form (round toward -inf): `Context.cpd_stats` with ONE fit point and w = 0, so that den[j] = 0 + K_j, and with the
    roles swapped (one target, the sweep as fit points), so that P1[i] = K_i / den;
  * norm-expansion form of both CPD passes: generic clouds at 0.84 of use_expansion's limit, and the same clouds just past it.

Every bound is derived in fastexp_cases.py from the header's constants and IEEE rounding; which arithmetic form a call runs is
asserted from the inputs with `regime_of` (tests/test_gpu_cpd_pair_pass_variants.py).  Sizes: the sweeps have 4 500 to 5 100
points (two points per thread in the pair passes), the generic clouds 1 500 (one per thread); the arithmetic of one pair is the
same template code at every size, and test_gpu_cpd_pair_pass_variants.py runs every instance.

Measured on an MI355X (largest deviation | bound):
  degree 3 (gauss_block), 5 115 elements                 1.000 ulp | 1 ulp; 491 subnormal results within 1.000 unit of 2^-1074; 77 flushed: +0
  degree 3 next to inf / NaN coordinates                 1.000 ulp | 1 ulp; inf - finite: +0; NaN: NaN (it was +0 before fastexp_clamp_d2)
  floor form, column sums, plain and clamped (4 504/7)   2.0230e-13 | 2.03e-13 (the CPU restatement's figure to the digit); 398 subnormal
                                                         results within one unit; 75 / 78 flushed: +0
  floor form, row statistics, plain and clamped          den 1.79e-14 | 1.203e-12; P1 2.2039e-13 | 1.4061e-12; PX against P1 x 3.55e-16 | 4.44e-16
  generic cloud, column sums, expansion (0.84 of limit)  3.84e-13; closest to its bound 2.72e-13 | 1.21e-12: use_expansion's 7.7e-16 holds
  generic cloud, column sums, just past the limit        3.57e-13; closest to its bound 2.0149e-13 | 2.0328e-13 (at |ln K| = 0.2)
  generic cloud, row statistics, expansion               den 1.5e-13, 2.4e-14; P1 4.46e-13 | 2.76e-12
  generic cloud, row statistics, just past the limit     den 9.0e-14, 1.6e-13; P1 6.45e-13, closest to its bound 2.91e-13 | 7.41e-13
  NaN coordinate in the fit / target cloud               den, P1, Pt1 NaN where the C restatement has them NaN, in all three regimes (in the
                                                         clamped one the NaN fit point used to contribute K = 0 to every column)
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import gingr_oracle as go
from tests import fastexp_cases as fc
from tests.test_gpu_cpd_pair_pass_variants import regime_of

pytestmark = pytest.mark.gpu

ORIGIN = np.zeros((1, 3))


def assert_guards(g):
    assert all(g.values()), [k for k, v in g.items() if not v]


def assert_plus_zero(values, where):
    v = np.asarray(values)[where]
    assert np.all(v == 0.0) and not np.any(np.signbit(v)), v[(v != 0.0) | np.signbit(v)][:8]


# ---------------------------------------------------------------------------------------------------- degree 3, round to nearest
def test_degree3_every_element_within_one_ulp(ctx):
    s, n_clamp = fc.nearest_sweep()
    assert len(s) <= 16384
    assert_guards(fc.guards_nearest(s, n_clamp))
    got = ctx.gauss_block(ORIGIN, s.points, fc.SIGMA_GAUSS, 1.0)[0]
    ulps = fc.ulp_error(got, s.hi)
    sub = (s.hi < 2.0 ** -1022) & ~s.below
    print(f"\ndegree 3: {len(s)} elements, largest deviation {ulps.max():.3f} ulp | {fc.ULPS_NEAREST} ulp; subnormal results "
          f"{int(sub.sum())}: {ulps[sub].max():.3f} units of 2^-1074; flushed to +0: {int(s.below.sum())}")
    assert ulps.max() <= fc.ULPS_NEAREST
    assert got[[u == 0 for u in s.U].index(True)] == 1.0                   # d2 = 0
    assert_plus_zero(got, s.below)                                         # every reference under 2^-1075 ...
    assert np.all(s.below[-n_clamp:])                                      # ... the clamp and what lies beyond it included
    assert s.below.sum() >= 32 + n_clamp


def test_degree3_non_finite_coordinates(ctx):
    """inf - finite is d2 = +inf, clamped: +0, as exp(-inf).  A NaN coordinate is a NaN squared distance and must come out as NaN,
    as it does from the formula exp(-|a - b|^2 / sigma^2): the clamp in front of the exponential must not swallow it (fmin did).  The
    finite elements around them keep their bound."""
    s, _ = fc.nearest_sweep()
    keep = np.arange(0, len(s), 7)
    inf, nan = math.inf, math.nan
    odd = np.array([[inf, 0.0, 0.0], [1.0, -inf, 2.0], [0.0, 0.0, inf], [-inf, inf, 3.0],
                    [nan, 0.0, 0.0], [0.5, nan, 0.25], [0.0, 0.0, nan], [inf, nan, 0.0], [nan, nan, nan]])
    pts = np.concatenate([s.points[keep][:300], odd[:4], s.points[keep][300:], odd[4:]])
    at_inf = np.arange(300, 304)
    at_nan = np.arange(len(pts) - 5, len(pts))
    finite = np.setdiff1d(np.arange(len(pts)), np.concatenate([at_inf, at_nan]))
    with np.errstate(invalid="ignore"):
        want = go.gauss_block(ORIGIN, pts, fc.SIGMA_GAUSS, 1.0)[0]
    assert np.all(want[at_inf] == 0.0) and np.all(np.isnan(want[at_nan]))
    got = ctx.gauss_block(ORIGIN, pts, fc.SIGMA_GAUSS, 1.0)[0]
    ulps = fc.ulp_error(got[finite], s.hi[keep])
    print(f"\ndegree 3 next to non-finite inputs: {ulps.max():.3f} ulp | {fc.ULPS_NEAREST} ulp; inf -> {got[at_inf]}, NaN -> {got[at_nan]}")
    assert_plus_zero(got, at_inf)
    assert np.all(np.isnan(got[at_nan])), got[at_nan]
    assert ulps.max() <= fc.ULPS_NEAREST
    # a NaN in the other cloud poisons its whole row and nothing else
    two = ctx.gauss_block(np.array([[0.0, 0.0, 0.0], [0.0, nan, 0.0]]), s.points[keep], fc.SIGMA_GAUSS, 1.0)
    assert np.all(np.isnan(two[1])) and fc.ulp_error(two[0], s.hi[keep]).max() <= fc.ULPS_NEAREST


# --------------------------------------------------------------------------------------------------------- floor form, column sums
@pytest.mark.parametrize("clamped", [False, True], ids=["plain", "clamped"])
def test_floor_form_column_sums(ctx, clamped):
    """den[j] = 0 + K_j: one fit point at the origin, w = 0.  Relative error <= 2.03e-13 (fastexp_cases.REL_FLOOR), one more unit of
    2^-1074 below 2^-1022, exactly +0 where the reference is under 2^-1075 -- past the clamp, past 2^42 and at d2 >= 1e300 as well."""
    s = fc.floor_sweep(clamped)
    assert len(s) <= 16384
    assert_guards(fc.guards_floor(s))
    if clamped:
        assert_guards(fc.guards_floor_clamped(s))
    reg = regime_of(ORIGIN, s.points, fc.SIGMA2_CPD)
    assert not reg["expand"] and reg["clamp"] == clamped, reg
    got = ctx.cpd_stats(ORIGIN, s.points, fc.SIGMA2_CPD, 0.0)["den"]
    err = fc.rel_error(got, s.hi, s.lo)
    sub = (s.hi < 2.0 ** -1022) & ~s.below
    print(f"\nfloor form, column sums, {'clamped' if clamped else 'plain'}: {len(s)} elements, largest relative deviation "
          f"{err[~sub].max():.4e} | {fc.REL_FLOOR:.2e}; subnormal results {int(sub.sum())}: beyond one unit of 2^-1074 by "
          f"{err[sub].max():.2e}; flushed to +0: {int(s.below.sum())}")
    assert err.max() <= fc.REL_FLOOR
    assert got[[u == 0 for u in s.U].index(True)] == float.fromhex("0x1.000000000038dp+0")   # d2 = 0: T'[0] = S, exactly
    assert_plus_zero(got, s.below)
    assert s.below.sum() >= 32 + (3 if clamped else 0)


# ------------------------------------------------------------------------------------------------------ floor form, row statistics
OFFSET = np.array([3.0, -5.0, 7.0]) / 64.0          # on the sweep's lattice: the single target, and the shift of the fit points


@pytest.mark.parametrize("clamped", [False, True], ids=["plain", "clamped"])
def test_floor_form_row_statistics(ctx, clamped):
    """One target at OFFSET, the sweep (moved by OFFSET: the differences stay exact) as fit points, w = 0: P1[i] = K_i / den with
    den = sum_i K_i, both from the 70-digit reference.  Bound: the element's 2.03e-13 plus the denominator's 2.03e-13 + M 2^-52 (M
    additions toward -inf), and (1 / den + 1) units of 2^-1074 below 2^-1022.  PX[i] = P1[i] x to 2^-51: K (x / den) against
    (K / den) x, three roundings toward -inf of which two cancel at best."""
    s = fc.floor_sweep(clamped)
    n = len(s) - 1 if clamped else len(s)           # without the point at 1e150: moved by OFFSET it would not be exact any more
    fit = s.points[:n] + OFFSET
    assert np.array_equal(fit - OFFSET, s.points[:n])
    assert tuple(fc.exact_d2(fit, OFFSET)) == s.d2[:n]
    target = OFFSET[None].copy()
    reg = regime_of(fit, target, fc.SIGMA2_CPD)
    assert not reg["expand"] and reg["clamp"] == clamped, reg
    den, hi, lo, bound = fc.rows_reference([[v] for v in fc.join(s.hi[:n], s.lo[:n])], np.full((n, 1), fc.REL_FLOOR))
    assert np.allclose(bound, 2.0 * fc.REL_FLOOR + n * 2.0 ** -52, rtol=1e-12, atol=0.0)
    assert den[0] >= 1
    got = ctx.cpd_stats(fit, target, fc.SIGMA2_CPD, 0.0)
    units = _units(False, [1.0 / float(den[0])])
    err = fc.rel_error(got["P1"], hi, lo, units=units)
    derr = abs(Fraction(float(got["den"][0])) / Fraction(den[0]) - 1)
    print(f"\nfloor form, row statistics, {'clamped' if clamped else 'plain'}: {n} rows, den {float(derr):.3e} | "
          f"{fc.REL_FLOOR + n * 2.0 ** -52:.3e}; P1 largest relative deviation {err.max():.4e} | {bound.max():.4e}")
    assert derr <= fc.REL_FLOOR + n * 2.0 ** -52
    assert np.all(err <= bound)
    assert_plus_zero(got["P1"], s.below[:n])
    # exactly, in Fractions; (|x| + 1) units of 2^-1074 are set aside: P1 or PX in the subnormal range has lost that much already
    worst = Fraction(0)
    for i in range(n):
        p1 = Fraction(float(got["P1"][i]))
        for d in range(3):
            x = Fraction(float(OFFSET[d]))
            slack = abs(Fraction(float(got["PX"][i, d])) - p1 * x) - (abs(x) + 1) * Fraction(fc.TINY)
            if p1 != 0 and slack > 0:
                worst = max(worst, slack / abs(p1 * x))
    print(f"    PX against P1 x: {float(worst):.3e} | {2.0 ** -51:.3e}")
    assert worst <= Fraction(2.0 ** -51)


# ------------------------------------------------------------------------------------------------------ norm-expansion form
def _element_bound(lnk, expand):
    return fc.REL_FLOOR + fc.ARG_ROUNDINGS * lnk + (fc.EXPAND_TOL if expand else 0.0)


def _units(expand, inv_den=(), terms=1):
    """Units of 2^-1074 a result below 2^-1022 may be off besides its relative bound.  Column sums: one, the ldexp toward -inf.  Row
    statistics: that unit divided by den_j for every target, and one per FMA that accumulates a term.  The expansion form multiplies
    the finished sum by the owned point's factor 2^(frac / 2048) <= 2^(1/4096) in round to nearest: half a unit more."""
    u = (sum(inv_den) + terms) if inv_den else 1.0
    return u * 2.0 ** (1.0 / 4096.0) + 0.5 if expand else u


@pytest.mark.parametrize("figure,expand", [(0.84e-12, True), (1.01e-12, False)], ids=["expansion", "just-past-the-limit"])
def test_generic_cloud_column_sums(ctx, figure, expand):
    """Generic coordinates, one fit point in a corner of the cloud, w = 0: den[j] = K_j.  Expansion form: 2.03e-13 + 1.6e-15 |ln K|
    (seven roundings of the argument at 2^-52) + kExpandTol, the budget use_expansion exists to enforce; the same cloud scaled just
    past the limit runs plain differences and owes 2.03e-13 + 1.6e-15 |ln K|."""
    fit, target, sigma2 = fc.generic_clouds(figure, False)
    fig = fc.expansion_figure(fit, target, sigma2)
    assert (0.5e-12 <= fig < 1e-12) if expand else (1e-12 <= fig < 1.05e-12), fig
    reg = regime_of(fit, target, sigma2)
    assert reg["expand"] == expand and not reg["clamp"], reg
    K, lnk = fc.pair_matrix(fit, target, sigma2)
    hi, lo = fc.split(K[0])
    bound = _element_bound(lnk[0], expand)
    got = ctx.cpd_stats(fit, target, sigma2, 0.0)["den"]
    err = fc.rel_error(got, hi, lo, units=_units(expand))
    live = hi >= 2.0 ** -1022
    assert live.sum() >= 500 and (hi > 1e-3).sum() >= 100
    k = int(np.argmax(err / bound))
    print(f"\ngeneric cloud, column sums, {'expansion' if expand else 'plain'} (figure {fig:.3e}): {int(live.sum())} normal results, "
          f"largest relative deviation {err[live].max():.4e}; closest to its bound: {err[k]:.4e} | {bound[k]:.4e} at |ln K| {lnk[0][k]:.1f}")
    assert np.all(err <= bound)
    assert_plus_zero(got, lnk[0] > 1100.0 * math.log(2.0))


@pytest.mark.parametrize("figure,expand", [(0.84e-12, True), (1.01e-12, False)], ids=["expansion", "just-past-the-limit"])
def test_generic_cloud_row_statistics(ctx, figure, expand):
    """The same cloud as fit points, two targets (the corner P and -P, centroid at the cube's centre), w = 0:
    P1[i] = K_iP / den_P + K_iQ / den_Q, reference and bound from fastexp_cases.rows_reference with the element bounds above."""
    fit, target, sigma2 = fc.generic_clouds(figure, True)
    fig = fc.expansion_figure(fit, target, sigma2)
    assert (0.5e-12 <= fig < 1e-12) if expand else (1e-12 <= fig < 1.05e-12), fig
    reg = regime_of(fit, target, sigma2)
    assert reg["expand"] == expand and not reg["clamp"], reg
    K, lnk = fc.pair_matrix(fit, target, sigma2)
    den, hi, lo, bound = fc.rows_reference(K, _element_bound(lnk, expand))
    got = ctx.cpd_stats(fit, target, sigma2, 0.0)
    units = _units(expand, [1.0 / float(d) for d in den], terms=2)
    err = fc.rel_error(got["P1"], hi, lo, units=units, everywhere=True)  # every K_ij within a unit of 2^-1074, divided by den_j
    derr = [float(abs(Fraction(float(g)) / Fraction(d) - 1)) for g, d in zip(got["den"], den)]
    live = hi >= 2.0 ** -1022
    assert live.sum() >= 500
    k = int(np.argmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f"\ngeneric cloud, row statistics, {'expansion' if expand else 'plain'} (figure {fig:.3e}): den {derr[0]:.3e}, {derr[1]:.3e}; "
          f"{int(live.sum())} normal rows, P1 largest relative deviation {err[live].max():.4e}; closest to its bound: {err[k]:.4e} | {bound[k]:.4e}")
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------ NaN in a CPD cloud
def _nan_clouds(regime):
    rng = np.random.default_rng(5)
    spread = {"expansion": 3.0, "plain": 12.0, "clamped": 12.0}[regime]
    x = rng.normal(0.0, spread, (400, 3))
    y = x[rng.permutation(400)[:300]] + rng.normal(0.0, 0.3, (300, 3))
    if regime == "clamped":
        x[17] = (1e5, -2e5, 5e4)
    return np.ascontiguousarray(y), np.ascontiguousarray(x), 1.0, 0.1


@pytest.mark.parametrize("where", ["fit", "target"])
@pytest.mark.parametrize("regime", ["expansion", "plain", "clamped"])
def test_nan_coordinate_in_a_cpd_cloud(ctx, regime, where):
    """One NaN coordinate in the fit cloud, or in the target cloud: den, P1 and Pt1 are NaN exactly where the C restatement of the
    reference's loops has them NaN (a NaN fit point poisons every column sum, a NaN target its own column and every row), and the
    other elements keep the suite's 1e-10.  In the clamped regime the clamp in front of the exponential must let the NaN through."""
    y, x, sigma2, w = _nan_clouds(regime)
    reg = regime_of(y, x, sigma2)           # of the finite clouds: the extent kernels skip a NaN coordinate (fmax), and every
    assert reg["expand"] == (regime == "expansion") and reg["clamp"] == (regime == "clamped"), reg   # predicate has a factor 2 to spare
    (y if where == "fit" else x)[123, 1] = math.nan
    want = co.cpd_stats(y, x, sigma2, w)
    got = ctx.cpd_stats(y, x, sigma2, w)
    for name, ref in (("den", want.den), ("P1", want.P1), ("Pt1", want.Pt1)):
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref)), (name, int(np.isnan(got[name]).sum()), int(np.isnan(ref).sum()))
        ok = ~np.isnan(ref)
        assert np.all(np.abs(got[name][ok] - ref[ok]) <= 1e-10 * np.abs(ref[ok])), name
    nans = {k: int(np.isnan(got[k]).sum()) for k in ("den", "P1", "Pt1")}
    print(f"\nNaN in the {where} cloud, {regime}: NaN elements {nans}")
    assert nans["P1"] == len(y) and nans["den"] == (len(x) if where == "fit" else 1)
