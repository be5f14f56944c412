"""The table exponential of gingr_amd/csrc/fastexp.h on the CPU: its two tables, its constants, the inputs of the device tests and the
stated arithmetic itself.

  * exp_table.inc holds the 2048 correctly rounded 2^(j/2048), exp_floor_table.inc the 2048 products fl(T[j] S) -- what
    tools/gen_exp_table.py writes and nothing else reads back.
  * With the header's constants taken as exact rationals, the three polynomials stay within the figures the header states:
    degree 3 on |f| <= 1/2: 3.42e-17, economised degree 2 on |f| <= 1/2 (no caller today): 2.0194e-13, floor form S (1 + f (Q0 + Q1 f))
    on [0, 1): 2.0203e-13.
  * The guards of tests/fastexp_cases.py hold on the inputs that test_gpu_fastexp.py sends to the device.
  * The Python restatements of fastexp2_scaled<3> (round to nearest) and fastexp2_floor_scaled (every operation toward -inf) meet,
    on every case, the bounds the device test asserts: the stated arithmetic is good enough, so a device failure is the kernel's.
    Measured: degree 3 at most 1.0 ulp (the header's claim holds as it stands); floor form 2.0230e-13 relative above 2^-1022, one
    unit of 2^-1074 below; every reference under 2^-1075 comes out as +0 in both."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import fastexp_cases as fc


def test_exp_table_is_the_correctly_rounded_power():
    T, _ = fc.tables()
    assert len(T) == 2048
    ctx = decimal.Context(prec=100)
    for j, v in enumerate(T):
        exact = Fraction(ctx.power(decimal.Decimal(2), ctx.divide(decimal.Decimal(j), decimal.Decimal(2048))))
        assert v == float(exact), (j, v.hex(), float(exact).hex())
        assert abs(exact - Fraction(v)) <= Fraction(math.ulp(v)) / 2


def test_floor_table_is_the_rounded_product():
    T, TF = fc.tables()
    S = fc.header()["S"]
    assert len(TF) == 2048
    for j in range(2048):
        assert TF[j] == T[j] * S == float(Fraction(T[j]) * Fraction(S)), j      # fl(T[j] S), round to nearest


def test_table_parser_skips_the_comment_with_a_hex_literal():
    import os
    with open(os.path.join(fc.CSRC, "exp_floor_table.inc")) as fh:
        head = fh.readline()
    assert head.startswith("//") and "0x1.000000000038dp+0" in head
    assert fc.tables()[1][0] == fc.header()["S"] and len(fc.tables()[1]) == 2048


def test_header_constants():
    h = fc.header()
    assert h["GINGR_EXP_MAGIC"] == 1.5 * 2.0 ** 52 and h["GINGR_EXP_MAGIC8"] == 1.5 * 2.0 ** 49
    a = Fraction(decimal.Context(prec=60).ln(decimal.Decimal(2))) / 2048
    # C1 is the correctly rounded ln2 / 2048; C2 and C3 are one unit of their last place off it (1.2e-16 and 1.3e-16 relative, times
    # f^2 C2 <= 1.4e-8 resp. f^3 C3 <= 8.1e-13 in the result: far below everything test_polynomials_meet_their_stated_errors measures)
    assert h["C1"] == float(a)
    for name, exact in (("C2", a * a / 2), ("C3", a ** 3 / 6)):
        assert abs(Fraction(h[name]) - exact) <= Fraction(math.ulp(h[name])), name
    assert abs(Fraction(h["C1_D2"]) - (a + a ** 3 / 6 * Fraction(3, 16))) < Fraction(1, 10 ** 18)
    assert h["S"] == float.fromhex("0x1.000000000038dp+0")


def test_polynomials_meet_their_stated_errors():
    got = fc.poly_errors()
    print(f"\npolynomials: degree 3 {got['deg3']:.4e} (bound {fc.POLY3_BOUND:.2e}), degree 2 {got['deg2']:.4e} (bound "
          f"{fc.POLY2_BOUND:.2e}), floor form {got['floor']:.4e} (bound {fc.POLYF_BOUND:.2e})")
    assert got["deg3"] <= fc.POLY3_BOUND
    assert got["deg2"] <= fc.POLY2_BOUND
    assert got["floor"] <= fc.POLYF_BOUND
    assert got["deg3"] > 3e-17 and got["deg2"] > 2e-13 and got["floor"] > 2e-13     # the grid reaches the extrema


def test_scales_are_what_the_inputs_assume():
    assert fc.c_cpd(fc.SIGMA2_CPD) == -4096.0
    assert Fraction(fc.c_gauss(fc.SIGMA_GAUSS)) == -Fraction(fc.LOG2E) * 8192
    assert fc.d2_limit(-4096.0) == 550.0


def test_guards_of_the_floor_sweep():
    for clamped in (False, True):
        s = fc.floor_sweep(clamped)
        assert len(s) <= 16384
        g = fc.guards_floor(s)
        assert all(g.values()), [k for k, v in g.items() if not v]
    g = fc.guards_floor_clamped(fc.floor_sweep(True))
    assert all(g.values()), g
    assert not any(fc.guards_floor_clamped(fc.floor_sweep(False)).values())


def test_guards_of_the_nearest_sweep():
    s, n_clamp = fc.nearest_sweep()
    assert len(s) <= 16384
    g = fc.guards_nearest(s, n_clamp)
    assert all(g.values()), [k for k, v in g.items() if not v]


def test_three_squares_and_exact_distances():
    n = np.array([0, 1, 2, 3, 6, 7, 15, 28, 2200 << 30, (1 << 41) + 5], dtype=np.int64)
    a, b, c, found = fc.three_squares(n)
    assert list(found) == [fc.representable(int(v)) for v in n] == [True, True, True, True, True, False, False, False, True, True]
    assert np.all((a * a + b * b + c * c == n)[found])
    with pytest.raises(AssertionError):
        fc.exact_d2(np.array([[0.1, 0.2, 0.3]]))


def test_nearest_restatement_meets_the_device_bound():
    s, _ = fc.nearest_sweep()
    got = np.array([fc.restate_nearest(float(d), s.c) for d in s.d2])
    ulps = fc.ulp_error(got, s.hi)
    print(f"\ndegree 3 restatement: {len(s)} cases, largest deviation {ulps.max():.3f} ulp (bound {fc.ULPS_NEAREST})")
    assert ulps.max() <= fc.ULPS_NEAREST
    assert np.all(got[s.below] == 0.0) and s.below.sum() >= 32
    assert got[[u == 0 for u in s.U].index(True)] == 1.0


@pytest.mark.parametrize("clamped", [False, True])
def test_floor_restatement_meets_the_device_bound(clamped):
    s = fc.floor_sweep(clamped)
    got = np.array([fc.restate_floor(float(d), s.c, clamp=clamped) for d in s.d2])
    err = fc.rel_error(got, s.hi, s.lo)
    sub = s.hi < 2.0 ** -1022
    print(f"\nfloor restatement ({'clamped' if clamped else 'plain'}): {len(s)} cases, largest relative deviation "
          f"{err[~sub].max():.4e} (bound {fc.REL_FLOOR:.2e}), {int(sub.sum())} results below 2^-1022 within one unit of 2^-1074")
    assert err.max() <= fc.REL_FLOOR
    assert np.all(got[s.below] == 0.0) and s.below.sum() >= 32


def test_decimal_reference_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    s = fc.floor_sweep(False)
    n, _ = fc.nearest_sweep()
    with mpmath.workprec(400):
        for sweep in (s, n):
            step = max(1, len(sweep) // 128)
            for u in sweep.U[::step][:128]:
                mine = fc.exp2_exact(u)
                if mine is None:
                    continue
                theirs = mpmath.power(2, mpmath.mpf(u.numerator) / u.denominator / 2048)
                ratio = mpmath.mpf(mine.numerator) / mine.denominator / theirs
                assert abs(ratio - 1) < mpmath.mpf(10) ** -60
