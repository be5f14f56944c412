"""CPU pin of gingr_amd/csrc/gpmm_plan.h, the host-side bookkeeping of the GPMM construction (what decides a model's rank and the values
of gingr_gpmm_info): the header compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone driver
(tests/c/gpmm_plan_driver.cpp).  Its column count, eigen blocks, merged spectrum and verdicts are those of the numpy restatement
(tests/gpmm_plan_restatement.py), bit for bit, and the column count it derives from the oracle's scalar traces is the column count of the
oracle's generic factorisation over the 3M (point, coordinate) entries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import gpmm_plan_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler: the only guard of the rank bookkeeping cannot run"
    exe = tmp_path_factory.mktemp("gpmm_plan") / "gpmm_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "gpmm_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def call(driver, *parts):
    raw = np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in parts]).tobytes()
    return np.frombuffer(subprocess.run([driver], input=raw, capture_output=True, check=True).stdout, dtype=np.float64)


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- column count
def columns(driver, htr, limit, rel_tol, M):
    htr = np.asarray(htr, dtype=np.float64)
    ks = htr.shape[0] - 1
    out = call(driver, [1, ks, limit, M, rel_tol], htr)
    assert out.shape[0] == 6
    n, cnt, reached, fraction = pr.count_columns(htr, ks, limit, rel_tol, M)
    assert [int(v) for v in out[:5]] == [n, *cnt, int(reached)] and same_bits(out[5], fraction)
    return n, cnt, bool(reached), fraction


TRACES = [100.0, 50.0, 20.0, 5.0, 1.0, 0.1]      # scalar traces of ks = 5 columns; generic: 300, 250, 200, 150, 120, 90, 60, 45, 30, 15, ...


@pytest.mark.parametrize("rel_tol,n", [(0.55, 3), (0.45, 4), (0.35, 5), (0.25, 6)])
def test_stop_at_every_remainder(driver, rel_tol, n):
    """the first generic trace below rel_tol * 300 sits at n % 3 == 0, 1, 2 and 0 again"""
    got = columns(driver, TRACES, 3 * 40, rel_tol, 40)
    assert got[0] == n and got[1] == [n // 3 + (d < n % 3) for d in range(3)] and got[2]
    assert got[3] == pr.generic_trace(TRACES, n) / 300.0 < rel_tol


def test_limit_before_tolerance(driver):
    n, cnt, reached, fraction = columns(driver, TRACES, 7, 0.01, 40)
    assert n == 7 and cnt == [3, 2, 2] and not reached and fraction == 45.0 / 300.0
    assert columns(driver, TRACES, 15, 1e-6, 40)[::2] == (15, False)          # the scalar columns run out: n = 3 ks, 3 tr_s(ks) left


def test_exhaustion_counts_as_reached(driver):
    htr = [4.0, 2.0, 1.0, 0.5, 0.25]                                           # M = ks = 4: every point pivoted, n = 3 M
    n, cnt, reached, fraction = columns(driver, htr, 12, 1e-3, 4)
    assert n == 12 and cnt == [4, 4, 4] and reached and fraction == 0.25 / 4.0
    assert not columns(driver, htr, 12, 1e-3, 5)[2]                            # the same traces of a larger cloud: not exhausted


def test_tolerance_zero(driver):
    n, cnt, reached, _ = columns(driver, TRACES, 3 * 40, 0.0, 40)               # nothing is below 0: the columns run out
    assert n == 15 and not reached
    assert columns(driver, [3.0, 1.0, 0.0], 3 * 40, 0.0, 40)[0] == 6            # an exact zero trace is not below 0 either


def test_nan_trace_stops(driver):
    htr = [100.0, 50.0, float("nan"), 5.0, 1.0]
    n, cnt, reached, fraction = columns(driver, htr, 3 * 40, 0.01, 40)          # trace(4) = 2 * 50 + NaN: not >= the threshold
    assert n == 4 and cnt == [2, 1, 1] and reached and np.isnan(fraction)


def test_one_scalar_column(driver):
    assert columns(driver, [10.0, 1.0], 3 * 40, 0.5, 40)[:3] == (2, [1, 1, 0], True)      # 30, 21, 12 against 15
    assert columns(driver, [10.0, 1.0], 3 * 40, 0.05, 40)[:3] == (3, [1, 1, 1], False)    # 3 against 1.5: out of columns
    assert columns(driver, [10.0, 1.0], 1, 0.05, 40)[:3] == (1, [1, 0, 0], False)


# ------------------------------------------------------------------------------------------------------ agreement with the oracle
@pytest.mark.parametrize("M,seed,sigma,rel_tol", [(12, 1, 30.0, 0.05), (25, 2, 45.0, 0.01), (40, 3, 60.0, 1e-4)])
def test_column_count_is_the_generic_factorisation_s(driver, M, seed, sigma, rel_tol):
    """The scalar traces of the oracle's scalar factorisation give the column count of its generic factorisation over the 3M entries."""
    pts = np.random.default_rng(seed).normal(0.0, 30.0, (M, 3))
    scaling = 20.0
    Ls = go.pivoted_cholesky_scalar(pts, sigma, scaling, rel_tol)
    ks = Ls.shape[1]
    diag, htr = np.full(M, scaling), []
    for k in range(ks + 1):                                                     # residual trace after k scalar pivots
        htr.append(float(diag.sum()))
        if k < ks:
            diag = diag - Ls[:, k] * Ls[:, k]
    tol = rel_tol * 3.0 * htr[0]
    margins = [abs(pr.generic_trace(htr, n) - tol) / tol for n in range(3 * ks + 1)]
    assert min(margins) > 1e-9, "a trace within 1e-9 of the threshold: the comparison would hang on rounding; choose another input"
    n, cnt, reached, _ = columns(driver, htr, 3 * M, rel_tol, M)
    Lg = go.pivoted_cholesky_matrix_valued(pts, [sigma], [scaling], rel_tol)
    assert Lg.shape == (3 * M, n) and reached and 0 < n < 3 * M
    assert cnt == [int(np.count_nonzero(np.abs(Lg[d::3]).sum(axis=0) > 0.0)) for d in range(3)]      # columns per coordinate


# -------------------------------------------------------------------------------------------------------------------- the merge
def merge(driver, cnt, ev_blocks, keep_rank, ex=1):
    out = call(driver, [2, *cnt, ex, keep_rank], *ev_blocks)
    nblocks, block_of, block_n = pr.group_blocks(cnt)
    assert int(out[0]) == nblocks == len(ev_blocks) and [int(v) for v in out[1:7]] == block_of + block_n
    n = int(out[7])
    assert n == sum(cnt) and out.shape[0] == 8 + 4 * n + 5
    variance, qdim, qblock, qidx = out[8:8 + 4 * n].reshape(4, n)
    keep, need, kept = int(out[8 + 4 * n]), [int(v) for v in out[9 + 4 * n:12 + 4 * n]], out[12 + 4 * n]
    ev = [np.asarray(e, dtype=np.float64) for e in ev_blocks]
    w = pr.merge_spectra(ev, cnt, block_of)
    assert same_bits(variance, w[0]) and all(np.array_equal(g, x) for g, x in zip((qdim, qblock, qidx), w[1:]))
    refusal, wkeep, info = pr.conclude(ex, False, keep_rank, n, True, 0.0, w[0])
    assert keep == wkeep and need == pr.eigvecs_needed(w[2], w[3], keep) and same_bits(kept, info[4])
    return variance, qdim.astype(int), qblock.astype(int), qidx.astype(int), keep, need


def test_merge_three_unequal_blocks_with_ties(driver):
    # cnt = (4, 4, 3): x and y share the 4-column block, z the 3-column block.  9.0 ties across all three coordinates at index 0
    # (order x, y, z); 5.0 ties inside a coordinate (indices 1 and 2, by index, the coordinates alternating within each index);
    # block 1 repeats 5.0 at index 1; the negative eigenvalue comes last with variance 0.
    ev = [[9.0, 5.0, 5.0, -1e-18], [9.0, 5.0, 2.0]]
    variance, qdim, qblock, qidx, keep, need = merge(driver, [4, 4, 3], ev, 0)
    assert list(variance) == [9.0, 9.0, 9.0, 5.0, 5.0, 5.0, 5.0, 5.0, 2.0, 0.0, 0.0]
    assert list(qdim) == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1] and list(qidx) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3]
    assert list(qblock) == [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0] and keep == 11 and need == [4, 3, 0]
    # keep_rank cuts inside the 9.0 tie, inside the 5.0 tie, at the column count and above it
    assert merge(driver, [4, 4, 3], ev, 2)[4:] == (2, [1, 0, 0])
    assert merge(driver, [4, 4, 3], ev, 3)[4:] == (3, [1, 1, 0])
    assert merge(driver, [4, 4, 3], ev, 7)[4:] == (7, [3, 2, 0])
    assert merge(driver, [4, 4, 3], ev, 11)[4:] == (11, [4, 3, 0])
    assert merge(driver, [4, 4, 3], ev, 12)[4:] == (11, [4, 3, 0])
    assert merge(driver, [4, 4, 3], ev, 5, ex=0)[4:] == (11, [4, 3, 0])         # the plain entry never truncates


def test_merge_block_shapes(driver):
    variance, qdim, qblock, qidx, keep, need = merge(driver, [3, 3, 3], [[4.0, 2.0, 1.0]], 4)
    assert list(qdim) == [0, 1, 2, 0, 1, 2, 0, 1, 2] and set(qblock) == {0} and (keep, need) == (4, [2, 0, 0])
    variance, qdim, qblock, qidx, keep, need = merge(driver, [1, 0, 0], [[7.0]], 0)         # one generic column: y and z have none
    assert list(variance) == [7.0] and list(qdim) == [0] and (keep, need) == (1, [1, 0, 0])
    variance, qdim, qblock, qidx, keep, need = merge(driver, [2, 2, 1], [[3.0, -2.0], [3.0]], 0)
    assert list(variance) == [3.0, 3.0, 3.0, 0.0, 0.0] and list(qdim) == [0, 1, 2, 0, 1] and list(qblock) == [0, 0, 1, 0, 0]


def test_merge_three_distinct_blocks(driver):
    # cnt = (3, 2, 1): every coordinate its own block (the build never produces it; the header takes it).  4.0 ties across x and y at
    # index 0 and again, in y's own block, at index 1 against x's index 1: by index first, then by coordinate.
    ev = [[6.0, 4.0, 1.0], [6.0, 4.0], [4.0]]
    variance, qdim, qblock, qidx, keep, need = merge(driver, [3, 2, 1], ev, 0)
    assert list(variance) == [6.0, 6.0, 4.0, 4.0, 4.0, 1.0]
    assert list(qdim) == [0, 1, 2, 0, 1, 0] and list(qidx) == [0, 0, 0, 1, 1, 2] and list(qblock) == [0, 1, 2, 0, 1, 0]
    assert (keep, need) == (6, [3, 2, 1])
    assert merge(driver, [3, 2, 1], ev, 3)[4:] == (3, [1, 1, 1])             # cuts inside the 4.0 tie: z's index 0 is in, the index 1 pair out
    assert merge(driver, [3, 2, 1], ev, 4)[4:] == (4, [2, 1, 1])


def test_group_kernels(driver):
    for ids, want in [([5, 5, 5], (1, [0, 0, 0], [0, -1, -1])), ([5, 6, 6], (2, [0, 1, 1], [0, 1, -1])),
                      ([5, 6, 5], (2, [0, 1, 0], [0, 1, -1])), ([5, 6, 7], (3, [0, 1, 2], [0, 1, 2]))]:
        out = [int(v) for v in call(driver, [4, *ids])]
        assert (out[0], out[1:4], out[4:7]) == want


# --------------------------------------------------------------------------------------------------------------------- conclude
def conclude(driver, ex, to_tolerance, keep_rank, reached, fraction, lam):
    lam = np.asarray(lam, dtype=np.float64)
    out = call(driver, [3, ex, to_tolerance, keep_rank, lam.shape[0], reached, fraction], lam)
    refusal, keep, info = pr.conclude(ex, to_tolerance, keep_rank, lam.shape[0], reached, fraction, lam)
    assert int(out[0]) == refusal and [int(v) for v in out[2:5]] == list(info[:3]) and same_bits(out[5:7], info[3:])
    assert keep is None or int(out[1]) == keep
    return refusal, keep, info


def test_conclude_kept_variance(driver):
    lam = np.sort(np.random.default_rng(5).uniform(0.1, 10.0, 300) ** 3)[::-1]
    for keep_rank in (1, 2, 150, 299):
        refusal, keep, info = conclude(driver, 1, 0, keep_rank, 1, 0.004, lam)
        assert refusal == pr.NONE and keep == keep_rank and info[:4] == (300, keep_rank, 1, 0.004)
        assert info[4] == np.cumsum(lam)[keep_rank - 1] / np.cumsum(lam)[-1] < 1.0
    for keep_rank in (0, 300, 301, -3):
        assert conclude(driver, 1, 0, keep_rank, 0, 0.3, lam)[1:] == (300, (300, 300, 0, 0.3, 1.0))
    assert conclude(driver, 0, 0, 7, 1, 0.004, lam)[1] == 300                   # keep_rank is the ex entry's
    assert conclude(driver, 1, 0, 2, 1, 0.0, [0.0, 0.0, 0.0])[2] == (3, 2, 1, 0.0, 1.0)      # an all-zero spectrum keeps "everything"


def test_conclude_refusals(driver):
    lam = np.linspace(2.0, 1.0, 600)
    # run to tolerance, the ceiling came first: refused before the spectrum is looked at
    assert conclude(driver, 1, 1, 100, 0, 0.02, lam) == (pr.CEILING_BEFORE_TOLERANCE, None, (600, 0, 0, 0.02, 1.0))
    assert conclude(driver, 1, 1, 100, 1, 0.009, lam)[0] == pr.NONE
    # more than 512 kept columns: refused with the info filled; 512 and the plain entry pass
    refusal, keep, info = conclude(driver, 1, 0, 0, 1, 0.009, lam)
    assert refusal == pr.ABOVE_RANK_LIMIT and keep == 600 and info == (600, 600, 1, 0.009, 1.0)
    assert conclude(driver, 1, 0, 513, 1, 0.009, lam)[0] == pr.ABOVE_RANK_LIMIT
    assert conclude(driver, 1, 0, 512, 1, 0.009, lam)[:2] == (pr.NONE, 512)
    assert conclude(driver, 0, 0, 0, 1, 0.009, lam)[:2] == (pr.NONE, 600)
