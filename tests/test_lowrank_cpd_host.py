"""CPU tests of the low-rank non-rigid CPD step: the numpy restatement of its Woodbury form (tests/lowrank_cpd_restatement.py)
against the oracle's dense step with G := L L^T, and the planner of its two passes (gingr_amd/csrc/classic_cpd_lowrank_plan.h),
compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/lowrank_plan_driver.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import lowrank_cpd_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

CASES = [("pair", 130, 150, 6.0, 2.0, 1e-2), ("pair", 500, 420, 10.0, 3.0, 1e-4), ("hull", 1500, 1125, 25.0, 2.0, 1e-8)]


@pytest.mark.parametrize("shape,M,N,beta,lam,tol", CASES)
def test_woodbury_step_is_the_dense_step_with_the_factor_in_place_of_g(shape, M, N, beta, lam, tol):
    """Three iterations, each from the oracle's state: TY, W and sigma2 of the restatement equal
    go.classic_cpd_maximization_nonrigid(X, TY, P, sigma2, L L^T, lambda) to 1e-12 relative (the two differ by rounding alone), and
    L^T W = z."""
    Y, X = lr.pair(M, N, 7 + M, noise=0.3) if shape == "pair" else lr.hull(M, N)
    L = lr.factor(Y, beta, tol)
    assert 1 < L.shape[1] < M
    G = L @ L.T
    TY, s2 = Y, go.classic_cpd_initial_sigma2(Y, X)
    for it in range(3):
        P = go.classic_cpd_expectation(X, TY, s2, 0.05)
        oTY, os2, oW = go.classic_cpd_maximization_nonrigid(X, TY, P, s2, G, lam)
        rTY, rs2, rW, z = lr.woodbury_step(X, TY, P, s2, L, lam)
        figures = (lr.rel(rTY, oTY), lr.rel(rW, oW), abs(rs2 - os2) / abs(os2), lr.rel(L.T @ rW, z))
        print(f"{shape} {M} iteration {it}: TY {figures[0]:.1e} W {figures[1]:.1e} sigma2 {figures[2]:.1e} L^T W - z {figures[3]:.1e}")
        assert max(figures) < 1e-12, (it, figures)
        TY, s2 = oTY, os2


# ---------------------------------------------------------------------------------------------------------------- the planner
SIZES = [1, 15, 16, 31, 32, 33, 130, 500, 700, 1500, 4999, 20000, 48000, 50000, 100003]
COLUMNS = [1, 31, 63, 64, 65, 98, 128, 200, 364, 511, 512]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("lowrank_plan") / "lowrank_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "lowrank_plan_driver.cpp"),
                           "-o", str(exe)])
    cases = [(M, k) for M in SIZES for k in COLUMNS if k <= M]

    def run():
        rows = np.ascontiguousarray(cases, dtype=np.int64)
        return np.frombuffer(subprocess.run([str(exe)], input=rows.tobytes(), capture_output=True, check=True).stdout, dtype=np.int64)

    flat = run()
    assert np.array_equal(flat, run())                                   # a plan depends on (M, k) alone
    out, at = {}, 0
    for case in cases:
        head = [int(v) for v in flat[at:at + 10]]
        npairs = head[3]
        out[case] = (head, flat[at + 10:at + 10 + 2 * npairs].reshape(npairs, 2), [int(v) for v in flat[at + 10 + 2 * npairs:at + 14 + 2 * npairs]])
        at += 14 + 2 * npairs
    assert at == flat.size
    return out


def test_padding_and_block_pairs(plans):
    for (M, k), (head, pairs, _) in plans.items():
        Mpad, kp, nb, npairs = head[:4]
        assert Mpad % 32 == 0 and M <= Mpad < M + 32, (M, k)
        assert kp % 64 == 0 and k <= kp < k + 64 and nb == kp // 64, (M, k)
        want = [(i, j) for i in range(nb) for j in range(i, nb)]         # every pair bi <= bj once, in this order
        assert npairs == len(want) and [tuple(int(v) for v in p) for p in pairs] == want, (M, k)


def test_slabs_tile_the_padded_rows_in_whole_chunks(plans):
    for (M, k), (head, _, _) in plans.items():
        Mpad, _, _, npairs, nslabs, rps, groups = head[:7]
        assert rps % 32 == 0 and rps >= 32, (M, k)
        assert 1 <= nslabs <= 256 and (nslabs - 1) * rps < Mpad <= nslabs * rps, (M, k)      # no slab is empty
        assert nslabs * npairs <= 1024 or nslabs == 1, (M, k)
        assert 1 <= groups <= 1024 and groups <= -(-M // 16), (M, k)


def test_workspace_sizes_and_layout(plans):
    for (M, k), (head, _, corners) in plans.items():
        Mpad, kp, nb, npairs, nslabs = head[:5]
        assert head[7] == Mpad * kp and head[8] == nslabs * npairs * 4096 and head[9] == nslabs * nb * 192, (M, k)
        # block b holds the columns 64 b .. 64 b + 63 of all padded rows, row-major
        first, last_row, last_col, end = corners
        assert first == 0 and last_row == (M - 1) * 64 and end == head[7] - 1, (M, k)
        assert last_col == ((k - 1) // 64) * Mpad * 64 + (k - 1) % 64, (M, k)

