"""Host side of the landmark-system tests (the device side is test_gpu_landmark_system.py):

1. every case of tests/landmark_system_cases.py has the edges it is built for (its guard), and the cases together cover what they must;
2. the extended-precision reference agrees with the oracle's own assembly (go.PDM._regression on the posed model) on the `well` family,
   to the float64 route's figure -- the reference restates the kernel's device-frame definition, the oracle works in the posed frame;
3. the float64 route's figures (np.linalg.inv, float64 products and sums: what the oracle does), per case and printed; the GPU bounds are
   1 000 x these, computed per case in the GPU test.  Largest per covariance family and rank class, measured here:

       family    rp <= 256 (r 24)      256 < rp < 512 (r 264)   rp = 512 (r 512)
                 G         rhs         G         rhs            G         rhs
       iso       6.76e-16  2.42e-16    4.56e-16  3.02e-16       -         -
       well      1.74e-15  5.33e-16    6.81e-16  3.56e-16       4.13e-16  4.37e-15
       pancake   1.13e-10  3.31e-10    3.27e-10  2.84e-10       -         -
       needle    1.09e-12  1.88e-12    7.40e-12  1.01e-11       3.46e-12  2.56e-12
       graded    1.03e-10  1.90e-10    1.32e-10  1.35e-10       -         -

   (Relative to the largest entry of Gabs the float64 route loses far less on `needle` than the 4e-11 of its worst single inverse: the
   large entries of C^-1, along the two tight directions, are the accurate ones.)  The same figures of the cofactor formula the kernel
   used before (lc.cofactor_inverse in place of np.linalg.inv): needle 1.66e-07 / 1.73e-07 at r 24, graded 5.16e-07 / 1.19e-07 --
   past 1 000 x the table for needle in G and rhs, for graded in G alone, which is what test_the_cofactor_formula_misses_the_bounds
   holds on to; the parent commit's kernel gave the same numbers on an MI355X (test_gpu_landmark_system.py);
4. spd3_inverse of gingr_amd/csrc/svd3.h compiled for the host (tests/c/spd3_driver.cpp) against the 60-digit inverse over all families:
   within 10 x the figure of np.linalg.inv on the same matrices, the identity inverted exactly, NaNs for what is no covariance; and the
   same program once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import landmark_system_cases as lc
from tests import posterior_solve_cases as pc

pytestmark = pytest.mark.skipif(not pc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------ 1. guards
@pytest.mark.parametrize("name", [c.name for c in lc.CASES])
def test_case_guards(name):
    lc.check_guard(lc.BY_NAME[name])


def test_cases_cover_the_edges():
    lc.check_coverage()
    assert len({c.name for c in lc.CASES}) == len(lc.CASES)
    assert lc.K_CHUNK == 256 and [pc.rp_of(r) for r in lc.RANKS] == [32, 272, 512]
    with open(os.path.join(ROOT, "gingr_amd", "csrc", "gp_obs.hip")) as f:
        src = f.read()
    assert "constexpr int kLmChunk = 256;" in src and "constexpr int kCols = 2;" in src   # the constants the cases are built around


# ------------------------------------------------------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize("name", ["r24-L3-well-skew", "r24-L257-well-skew", "r264-L600-well-skew-override"])
def test_reference_agrees_with_the_oracles_assembly(name):
    """G = QtL Q and rhs = QtL (y - m) of genericRegressionComputations on the model posed by (R, t, center): the same numbers as the
    device-frame sums, since the posed basis is R Q_p and the posed displacement R v_l"""
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    ref, mean, U, lam = lc.model_parts(case.r)
    euler, t, c = case.pose
    posed = go.PDM(np.array(ref), np.array(mean), np.array(U), np.array(lam)).transform(go.euler_to_rot(*euler), np.asarray(t), np.asarray(c))
    keep = li.rows >= 0
    pids = li.rows[keep]
    _, QtL, yVec, mVec = posed._regression(pids, li.points[keep] - posed.ref[pids], li.covs[keep])
    rows = (3 * pids[:, None] + np.arange(3)[None, :]).reshape(-1)
    Q = posed.U[rows, :] * np.sqrt(posed.lam)[None, :]
    want, _, figures = lc.reference_of(name)
    dG, dr = lc.deviation((QtL @ Q, QtL @ (yVec - mVec)), want)
    # the oracle rounds the posed reference and the posed basis once more than the float64 route does: ten times its figure
    print(f"{name}: oracle assembly against the reference: G {dG:.2e} rhs {dr:.2e}; float64 route {figures[0]:.2e} {figures[1]:.2e}")
    assert dG <= 10.0 * figures[0] and dr <= 10.0 * figures[1], (dG, dr, figures)


# ------------------------------------------------------------------------------------------------------------------ 3. the float64 route
def test_float64_route_figures():
    rows = {}
    for case in lc.CASES:
        _, _, fig = lc.reference_of(case.name)
        print("    %-34s G %.2e  rhs %.2e" % (case.name, *fig))
        assert 0.0 < fig[0] < 1e-9 and 0.0 < fig[1] < 1e-9, (case.name, fig)    # no family is beyond what 1 000 x can still tell apart
        key = (case.family, lc.column_class(case.rp))
        rows[key] = tuple(max(a, b) for a, b in zip(rows.get(key, (0.0, 0.0)), fig))
    print("  largest per family and column class:")
    for (fam, cls), fig in sorted(rows.items()):
        print("    %-8s %-7s G %.2e  rhs %.2e" % (fam, cls, *fig))
    # conditioning shows where it must: the ill-conditioned families lose digits, the others none
    for (fam, cls), fig in rows.items():
        assert (max(fig) > 1e-13) == (fam in lc.NOMINAL), (fam, cls, fig)


@pytest.mark.parametrize("name", ["r24-L257-needle-skew", "r24-L257-graded-skew", "r264-L600-needle-skew"])
def test_the_cofactor_formula_misses_the_bounds(name):
    """The revert check on the host: the system assembled with the cofactor inverse, operation by operation as landmarks_kernel had it,
    is outside 1 000 x the float64 route's figure -- the bound of the GPU test -- for the two families with a small middle eigenvalue:
    `needle` by two orders in G and rhs, `graded` (whose float64 route loses seven digits itself) by a factor 5 in G alone."""
    case, li = lc.BY_NAME[name], lc.lists_of(name)
    want, _, fig = lc.reference_of(name)
    got = lc.reference(lc.model_parts(case.r), case.pose, li.rows, li.points, li.covs, dtype=np.float64, inverse=lc.cofactor_inverse)
    dG, dr = lc.deviation(got, want)
    bG, br = lc.bounds_of(fig, case.r)
    print(f"{name}: cofactor formula G {dG:.2e} (bound {bG:.2e})  rhs {dr:.2e} (bound {br:.2e})")
    assert dG > bG, (dG, bG, dr, br)
    assert case.family != "needle" or (dG > 100.0 * bG and dr > br), (dG, bG, dr, br)


# ------------------------------------------------------------------------------------------------------------------ 4. spd3_inverse
def _build(tmp, name, extra):
    exe = tmp / name
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gingr_amd", "csrc"), *extra,
                           os.path.join(ROOT, "tests", "c", "spd3_driver.cpp"), "-o", str(exe)])
    return exe


def _run(exe, C):
    raw = subprocess.run([str(exe)], input=np.ascontiguousarray(C, dtype=np.float64).tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(raw, dtype=np.float64).reshape(-1, 3, 3)


def _rel_error(X, ref):
    return float((np.abs(X.astype(lc.LD) - ref).reshape(-1, 9).max(1) / np.abs(ref).reshape(-1, 9).max(1)).max())


NOT_A_COVARIANCE = {
    "rank 2": [[1.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 1.0]],           # (1,1,0)(1,1,0)^T + (0,1,1)(0,1,1)^T: the last pivot is exactly 0
    "rank 1": [[4.0, 2.0, -2.0], [2.0, 1.0, -1.0], [-2.0, -1.0, 1.0]],
    "indefinite": [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]],       # eigenvalues 3, -1, 1
    "negative": [[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]],
    "zero": [[0.0] * 3] * 3,
    "nan": [[1.0, 0.0, 0.0], [0.0, float("nan"), 0.0], [0.0, 0.0, 1.0]],
    "nan off the diagonal": [[1.0, 0.0, float("nan")], [0.0, 1.0, 0.0], [float("nan"), 0.0, 1.0]],
    "inf": [[float("inf"), 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
}


def _check_inverse(exe, n):
    for fam in lc.FAMILIES:
        C = lc.covariances(fam, n, 3)
        ref = np.array([lc.mp_inverse(c) for c in C])
        got = _run(exe, C)
        e_new, e_inv = _rel_error(got, ref), _rel_error(np.linalg.inv(C), ref)
        print(f"spd3_inverse {fam}: {e_new:.2e}, np.linalg.inv {e_inv:.2e}, "
              f"cofactor formula {_rel_error(np.array([lc.cofactor_inverse(c) for c in C]), ref):.2e}")
        assert e_new <= 10.0 * e_inv, (fam, e_new, e_inv)
        assert np.array_equal(got, np.swapaxes(got, 1, 2)), fam
    eye = _run(exe, np.eye(3)[None])[0]
    assert np.array_equal(eye, np.eye(3)) and not np.signbit(eye).any()             # exactly I: the goldens' identity covariances keep their bits
    for scale in (0.25, 4.0, 2.0 ** 40):
        assert np.array_equal(_run(exe, scale * np.eye(3)[None])[0], np.eye(3) / scale), scale
    bad = _run(exe, np.array(list(NOT_A_COVARIANCE.values())))
    for name, out in zip(NOT_A_COVARIANCE, bad):
        assert np.isnan(out).all(), (name, out)
    # the two triangles are averaged: a covariance that is symmetric to rounding only is inverted as its symmetric part
    C = lc.covariances("well", 4, 5).copy()
    skew = C.copy()
    skew[:, 0, 1] *= 1.0 + 2.0 ** -50
    sym = 0.5 * (skew + np.swapaxes(skew, 1, 2))
    assert np.array_equal(_run(exe, skew), _run(exe, sym))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no HIP compiler")
def test_spd3_inverse_against_mpmath(tmp_path):
    _check_inverse(_build(tmp_path, "spd3_driver", ["-O2"]), 200)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no HIP compiler")
def test_spd3_inverse_under_sanitizers(tmp_path):
    """the same stand-alone program with the address and undefined-behaviour sanitizers compiled in (host code only)"""
    exe = _build(tmp_path, "spd3_driver_san", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    _check_inverse(exe, 40)
