"""The numpy restatement of gingr_model_localize (tests/localize_restatement.py) against exact properties of a tapered covariance, its
route (pivoted Cholesky, Gram matrix, eigh) against the eigen-decomposition of the dense K, the shared cases' fitness for the
comparisons the GPU test makes (pivot stability, stop margins, distance from the cutoff), and the entry in the header, the loader and
the Python layer.  CPU only.

The localization keeps no decision in a plan header -- the column ceiling, the stop rule and the info are gpmm_factor::Factor's and
three lines of the entry point -- so there is no stand-alone sanitizer driver here; tests/test_gpmm_plan_host.py has the one of the
bookkeeping the tail shares with the GPMM build."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import localize_restatement as lr
from tests.localize_restatement import CASES, FULL_CASES, PIVOT_STABLE, ROUTE_SPREAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("M,r,sigma", [(5, 3, 40.0), (37, 16, 25.0), (86, 20, 30.0)])
def test_the_taper_keeps_every_variance(M, r, sigma):
    src, K = lr.source(M, r), lr.case_K(M, r, sigma)
    full = src.Q0 @ src.Q0.T
    np.testing.assert_array_equal(np.diag(K), np.diag(full))                      # g(x, x) = exp(0) = 1 exactly
    # ... and the whole 3 x 3 block of every vertex
    for i in (0, M // 2, M - 1):
        np.testing.assert_array_equal(K[3 * i:3 * i + 3, 3 * i:3 * i + 3], full[3 * i:3 * i + 3, 3 * i:3 * i + 3])
    assert abs(np.trace(K) - src.variance.sum()) <= 1e-13 * src.variance.sum()    # orthonormal basis: trace Q Q^T = sum lambda
    np.testing.assert_array_equal(K, K.T)
    assert np.linalg.eigvalsh(K).min() >= -1e-13 * src.variance[0]                # Schur product of two PSD matrices


def test_a_wide_taper_gives_the_source_back():
    src = lr.source(150, 100)
    x = lr.localize(src, 1e12, tol=0.0)
    # exp(-d^2 / 1e24) rounds to 1 for every pair (d^2 < 1e5): K = Q Q^T to the bit, rank 100 of 450 entries, the factor stops by exhaustion
    assert np.array_equal(lr.dense_K(src, 1e12), src.Q0 @ src.Q0.T)
    assert x.model.rank == 100 and x.tolerance_reached
    np.testing.assert_allclose(x.model.variance, src.variance, rtol=0, atol=1e-13 * src.variance[0])
    P = lr.probes(450)
    np.testing.assert_allclose(x.model.operator(P), src.operator(P), rtol=0, atol=1e-12 * np.abs(src.operator(P)).max())
    np.testing.assert_array_equal(x.model.mean, src.mean)
    np.testing.assert_array_equal(x.model.reference, src.reference)


def test_a_narrow_taper_gives_a_block_diagonal_covariance():
    src = lr.source(37, 16)
    K = lr.dense_K(src, 1e-3)                                                     # exp(-d^2 / 1e-6) underflows to 0 between any two vertices
    full = src.Q0 @ src.Q0.T
    want = np.zeros_like(full)
    for i in range(37):
        want[3 * i:3 * i + 3, 3 * i:3 * i + 3] = full[3 * i:3 * i + 3, 3 * i:3 * i + 3]
    np.testing.assert_array_equal(K, want)
    x = lr.localize(src, 1e-3, tol=0.0)
    # the spectrum is the union of the 37 blocks' spectra
    blocks = np.sort(np.concatenate([np.linalg.eigvalsh(full[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(37)]))[::-1]
    assert x.columns == 111
    np.testing.assert_allclose(x.model.all_variance, np.maximum(blocks, 0.0), rtol=0, atol=1e-13 * blocks[0])


@pytest.mark.parametrize("case", [(700, 8, 400.0, 1e-2), (700, 8, 400.0, 1e-8), (171, 8, 60.0, 0.0), (300, 512, 400.0, 1e-8)])
def test_the_residual_is_positive_semidefinite_with_the_reported_trace(case):
    M, r, sigma, tol = case
    x, K = lr.expected(*case), lr.case_K(M, r, sigma)
    assert x.model.rank == x.columns                                              # nothing cut: Q' Q'^T = L L^T
    R = K - x.model.Q0 @ x.model.Q0.T
    lam1 = x.model.variance[0]
    low = np.linalg.eigvalsh(R).min()
    print(f"{case}: {x.columns} columns, residual trace {np.trace(R):.6e} = {np.trace(R) / np.trace(K):.3e} of the trace "
          f"(reported {x.residual_fraction:.3e}), smallest eigenvalue {low / lam1:.1e} lambda_1")
    assert low >= -1e-12 * lam1
    assert abs(np.trace(R) - x.residual_fraction * x.total_variance) <= 1e-12 * lam1
    assert abs(x.total_variance - lr.source(M, r).variance.sum()) <= 1e-12 * lam1
    assert abs(x.total_variance - x.model.all_variance.sum() - x.residual_fraction * x.total_variance) <= 1e-12 * lam1


def test_max_rank_cuts_the_leading_components():
    full = lr.expected(86, 20, 30.0, 0.0)
    cut = lr.expected(86, 20, 30.0, 0.0, 9)
    assert cut.model.rank == 9 and cut.columns == full.columns == 258
    np.testing.assert_array_equal(cut.model.variance, full.model.variance[:9])
    assert lr.expected(86, 20, 30.0, 0.0, 4000).model.rank == 258


# ------------------------------------------------------------------------------------------------------ two routes
def test_route_spread():
    worst = 0.0
    for c in FULL_CASES:
        M, r, sigma, _ = c
        x = lr.expected(*c)
        y = lr.dense_eigh(lr.source(M, r), lr.case_K(M, r, sigma))
        assert x.model.rank == y.rank
        d_lam = float(np.abs(x.model.variance - y.variance).max() / y.variance[0])
        P = lr.probes(3 * M)
        want = lr.case_K(M, r, sigma) @ P
        d_op = float((np.linalg.norm(x.model.operator(P) - want, axis=0) / np.linalg.norm(want, axis=0)).max())
        print(f"{c}: {x.columns} columns, rank {x.model.rank}, eigenvalues {d_lam:.2e} of lambda_1, operator {d_op:.2e} of the result")
        worst = max(worst, d_lam, d_op)
    print(f"largest: {worst:.2e}; ROUTE_SPREAD = {ROUTE_SPREAD:.2e}")
    assert worst <= ROUTE_SPREAD


@pytest.mark.parametrize("case", FULL_CASES)
def test_full_factorisations_take_every_column(case):
    M, r, sigma, tol = case
    x = lr.expected(*case)
    want_cols = 37 if case == (37, 1, 25.0, 0.0) else 3 * M
    assert x.columns == want_cols and x.model.rank == want_cols and x.tolerance_reached


# ------------------------------------------------------------------------------------------------------ fitness of the cases
@pytest.mark.parametrize("case", PIVOT_STABLE)
def test_pivot_sequence_and_stop_step_do_not_hang_on_rounding(case):
    """The GPU test asks for the restatement's column count in these cases: the float64 pivot sequence is the longdouble one, and the
    stop step clears the tolerance by more than 1 % on both sides (the last trace that continues, the first that stops)."""
    M, r, sigma, tol = case
    K = lr.case_K(M, r, sigma)
    x = lr.expected(*case)
    _, piv_ld, tr_ld = lr.pivoted_cholesky(K, tol, dtype=np.longdouble)
    assert np.array_equal(x.pivots, piv_ld)
    k = x.columns
    above, below = float(x.traces[k - 1] / x.traces[0]) / tol - 1.0, 1.0 - float(x.traces[k] / x.traces[0]) / tol
    print(f"{case}: {k} columns; the trace before the last column is {100 * above:.1f} % above the tolerance, after it {100 * below:.1f} % below")
    assert above > 0.01 and below > 0.01
    assert abs(float(tr_ld[k] / tr_ld[0]) - x.residual_fraction) <= 1e-3 * tol


@pytest.mark.parametrize("case", CASES)
def test_no_eigenvalue_near_the_cutoff(case):
    x = lr.expected(*case)
    rel = x.model.all_variance / x.model.all_variance[0]
    print(f"{case}: rank {x.model.rank} of {x.columns} columns, smallest kept {rel[x.model.rank - 1]:.2e}")
    assert not np.any((rel > 0.1 * lr.CUTOFF) & (rel < 10.0 * lr.CUTOFF))


def test_the_shared_table():
    got = {c: (lr.expected(*c).columns, lr.expected(*c).tolerance_reached) for c in lr.STOPPED_CASES}
    assert got[(171, 8, 60.0, 0.0)] == (512, False)
    assert got[(700, 8, 400.0, 1e-8)] == (214, True)
    assert got[(2500, 3, 500.0, 1e-8)] == (68, True)
    assert got[(700, 40, 900.0, 1e-8)] == (512, False)
    assert got[(300, 512, 400.0, 1e-8)] == (512, False)
    assert got[(700, 8, 400.0, 1e-2)] == (12, True)
    assert all(lr.TOLERANCE_REACHED[c] == lr.expected(*c).tolerance_reached for c in CASES)
    for c in lr.STOPPED_CASES:
        x = lr.expected(*c)
        assert (x.residual_fraction < c[3]) == x.tolerance_reached


# ------------------------------------------------------------------------------------------------------ the surface
def test_entry_is_declared_bound_and_exported():
    from gingr_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert re.search(r"\bint gingr_model_localize\s*\(", header)
    assert "gingr_model_localize" in _native.SIGNATURES and hasattr(lib, "gingr_model_localize")
    assert len(_native.SIGNATURES["gingr_model_localize"][1]) == 7
    # typedef struct { int32 columns, rank, tolerance_reached; double residual_fraction, total_variance, kept_variance; }: 3 x 4 bytes,
    # 4 of padding, 3 x 8
    body = re.search(r"typedef struct gingr_localize_info \{(.*?)\} gingr_localize_info;", header, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|double)\s+(\w+);", body)
    assert [(n, {"int32_t": ctypes.c_int32, "double": ctypes.c_double}[t]) for t, n in fields] == list(_native.LocalizeInfo._fields_)
    assert ctypes.sizeof(_native.LocalizeInfo) == 40 and _native.LocalizeInfo.residual_fraction.offset == 16


def test_python_layer_names():
    import gingr_amd as ga
    from gingr_amd import api, models
    assert api.LocalizedDevicePointDistributionModel is models.LocalizedDevicePointDistributionModel is ga.LocalizedDevicePointDistributionModel
    assert api.LocalizeInfo is models.LocalizeInfo is ga.LocalizeInfo
    assert issubclass(ga.LocalizedDevicePointDistributionModel, ga.DevicePointDistributionModel)
    assert callable(ga.DeviceModel.localize) and callable(ga.PointDistributionModel.localizeModel)
    assert [f.name for f in dataclasses.fields(ga.LocalizeInfo)] == [n for n, _ in __import__("gingr_amd")._native.LocalizeInfo._fields_]


def test_the_timing_hook_is_listed():
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    assert re.search(r"21 = the pivot step of gingr_model_localize", header)
    common = open(os.path.join(ROOT, "gingr_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define GINGR_TIMERS (\d+)", common).group(1)) >= 22
