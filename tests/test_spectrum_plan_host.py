"""CPU side of the spectrum cut of the derived-model builders (gingr_amd/csrc/spectrum_plan.h): the header compiled for the host with
the address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/spectrum_plan_driver.cpp), run as a child process on
hand-worked spectra, and against the numpy restatements that state the same rule (tests/pca_restatement.py: _keep,
tests/localize_restatement.py: keep_count).  Doubles travel as hex floats in both directions: every comparison is of bits."""
import os
import shutil
import subprocess
from typing import NamedTuple

import numpy as np
import pytest

from tests import localize_restatement as lz
from tests import pca_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


class Cut(NamedTuple):
    k: int
    first_nonfinite: int
    kept: float
    total: float
    lam: list


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("spectrum_plan") / "spectrum_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "spectrum_plan_driver.cpp"),
                           "-o", str(exe)])

    def run(*case):
        words = [float(c).hex() if isinstance(c, (float, np.floating)) else str(c) for c in case]
        return subprocess.run([str(exe)] + words, capture_output=True, check=True, text=True).stdout.split("\n")
    return run


def cut(driver, ev, shift=0.0, available=None, max_rank=0, tol=1e-10) -> Cut:
    ev = [float(v) for v in ev]
    out = driver("cut", float(shift), len(ev) if available is None else available, max_rank, float(tol), *ev)
    k, bad = (int(v) for v in out[0].split())
    kept, total = (float.fromhex(v) for v in out[1].split())
    return Cut(k, bad, kept, total, [float.fromhex(v) for v in out[2].split()])


def ascending_sum(values) -> float:
    acc = 0.0
    for v in values:
        acc += float(v)
    return acc


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- by hand
def test_one_eigenvalue(driver):
    assert cut(driver, [2.5]) == Cut(1, -1, 2.5, 2.5, [2.5])
    assert cut(driver, [2.5], shift=1.0) == Cut(1, -1, 1.5, 1.5, [1.5])
    assert cut(driver, [2.5], available=0) == Cut(0, -1, 0.0, 2.5, [2.5])        # (a single centred shape spans nothing)
    assert cut(driver, [0.0]) == Cut(0, -1, 0.0, 0.0, [0.0])


def test_all_zeros_have_rank_zero(driver):
    for tol in (0.0, 1e-10):
        assert cut(driver, [0.0] * 7, tol=tol) == Cut(0, -1, 0.0, 0.0, [0.0] * 7)
    assert cut(driver, [3.0] * 7, shift=3.0).k == 0                                # the shift alone: a null space of every dimension


def test_threshold_is_strict(driver):
    lam = [1.0, 0.5, 0.25, 0.125]                                                  # 0.25 * 1.0 is exact
    assert cut(driver, lam, tol=0.25).k == 2
    assert cut(driver, lam, tol=np.nextafter(0.25, 0.0)).k == 3
    assert cut(driver, lam, tol=0.125).k == 3
    assert driver("leading", 4, 0.25, *lam)[0] == "2"
    assert driver("leading", 1, 0.0, *lam)[0] == "1" and driver("leading", 0, 0.0, *lam)[0] == "0"


def test_zero_tolerance_keeps_the_positive_entries(driver):
    c = cut(driver, [3.0, 2.0, 5e-324, 0.0, 0.0], tol=0.0)
    assert (c.k, c.kept, c.total) == (3, 5.0, 5.0)
    assert cut(driver, [3.0, 0.0, 0.0], tol=0.0).k == 1


def test_an_eigenvalue_below_the_shift_clamps_and_ends_the_run(driver):
    c = cut(driver, [5.0, 4.0, 2.9, 2.5], shift=3.0, tol=0.0)
    assert c == Cut(2, -1, 3.0, 3.0, [2.0, 1.0, 0.0, 0.0])
    assert float.fromhex(driver("unshift", 2.5, 3.0)[0]) == 0.0 and float.fromhex(driver("unshift", 3.0, 1.0)[0]) == 2.0
    # nothing behind a clamped entry comes back, whatever it holds
    assert cut(driver, [5.0, 2.0, 4.0], shift=3.0, tol=0.0).k == 1


def test_rank_ceiling_from_each_source(driver):
    ones = [1.0] * 600
    assert cut(driver, ones[:10], available=4).k == 4                              # what the data can span
    assert cut(driver, ones[:10], max_rank=3).k == 3                               # the caller's limit
    assert cut(driver, ones[:10], available=4, max_rank=6).k == 4 and cut(driver, ones[:10], available=9, max_rank=6).k == 6
    assert cut(driver, ones, max_rank=0).k == 512                                  # the width of a model, no limit given
    assert cut(driver, ones, max_rank=600).k == 512                                # ... and a limit above it
    assert cut(driver, ones, max_rank=512).k == 512 and cut(driver, ones, max_rank=511).k == 511
    assert cut(driver, ones[:10], available=20).k == 10                            # never past the spectrum
    for available, max_rank, want in [(4, 0, 4), (600, 0, 512), (600, 600, 512), (600, 3, 3), (2, 3, 2), (513, 512, 512), (0, 5, 0)]:
        assert int(driver("ceiling", available, max_rank)[0]) == want


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_the_first_value_that_is_not_finite_is_reported(driver, bad):
    base = [9.0, 7.0, 5.0, 3.0, 1.0]
    for at in (0, 2, 4):
        ev = list(base)
        ev[at] = bad
        assert cut(driver, ev, shift=0.5).first_nonfinite == at
    ev = list(base)
    ev[1] = ev[3] = bad
    assert cut(driver, ev).first_nonfinite == 1
    assert cut(driver, base).first_nonfinite == -1


def geometric(n=512, first=7.3, ratio=0.97):
    return first * ratio ** np.arange(n)


@pytest.mark.parametrize("shift", [0.0, 0.8125])
def test_sums_are_plain_ascending_loops(driver, shift):
    ev = geometric() + shift
    lam = [max(float(v) - shift, 0.0) for v in ev]
    for tol, max_rank in [(1e-10, 0), (1e-3, 0), (0.0, 100)]:
        c = cut(driver, ev, shift=shift, max_rank=max_rank, tol=tol)
        k = 0
        while k < (max_rank or 512) and lam[k] > tol * lam[0] and lam[k] > 0.0:
            k += 1
        assert c.k == k and 0 < k and same_bits(c.lam, lam)
        assert same_bits(c.total, ascending_sum(lam)) and same_bits(c.kept, ascending_sum(lam[:k]))
        assert same_bits(c.kept, c.total) == (k == 512)


# -------------------------------------------------------------------------------------------- the restatements state the same rule
def spectra():
    rng = np.random.default_rng(20261021)
    out = [geometric(), geometric(40, 3.0, 0.5), geometric(600, 1.0, 0.999), np.array([4.0, 1.0, 1e-10 * 4.0, 1e-12 * 4.0, 0.0]),
           np.array([1.0]), np.zeros(6), np.array([2.0, 2.0, 2.0, 0.0])]
    for n in (2, 17, 193, 513):
        lam = np.sort(rng.random(n) ** 8)[::-1].copy()
        lam[int(0.7 * n):] = 0.0                                                   # a null space, as a centred Gram matrix has
        out.append(lam)
    return out


@pytest.mark.parametrize("tol,max_rank", [(1e-10, 0), (0.0, 0), (1e-3, 5), (0.5, 600)])
def test_pca_restatement_keeps_the_same_count(driver, tol, max_rank):
    for lam in spectra():
        n = lam.shape[0]
        assert cut(driver, lam, available=n - 1, max_rank=max_rank, tol=tol).k == pr._keep(lam, n, tol, max_rank), (n, tol, max_rank)


@pytest.mark.parametrize("max_rank", [0, 5, 600])
def test_localize_restatement_keeps_the_same_count(driver, max_rank):
    for lam in spectra():
        assert cut(driver, lam, max_rank=max_rank, tol=lz.CUTOFF).k == lz.keep_count(lam, max_rank), (lam.shape[0], max_rank)
