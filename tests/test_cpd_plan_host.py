"""CPU pins of the all-pairs planners (gingr_amd/csrc/cpd_plan.h), compiled for the host with the address and undefined-behaviour
sanitizers into a stand-alone driver (tests/c/cpd_plan_driver.cpp).  Properties the kernels and launchers rely on, checked from the
plans themselves; the planner is not restated:

1. the chunks of a plan tile the streamed side exactly, start on 64-point quarters, are as many as `ChunkPlan::chunks` says and are
   balanced to a quarter;
2. the workspace sizes are the chunk counts of the very plans the launchers launch by;
3. the instance selection (points per thread) hits its documented thresholds, and `fair` is set exactly in one-round launches;
4. the nearest-neighbour plans cover the targets, the pruned plan never has more chunks than the unpruned one (nn_ws_bytes sizes by the
   latter), and the small scan's slice count stays inside the two bounds its planner states."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_cpd_pair_pass_variants import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1500, 1700, 2047, 2048, 2049, 5500, 6000, 6250, 16383, 16384, 16385, 24576, 50000,
           100003, 400000]
RESIDENT = [0, 768, 1024]
PTS = [1, 2, 4]
FORCED = [0, 1, 3, 7]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("cpd_plan") / "cpd_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "cpd_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def run(driver, mode, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = subprocess.run([driver, mode], input=rows.tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(out, dtype=np.int64)


@pytest.fixture(scope="module")
def chunk_plans(driver):
    """Every plan of the grid, once: (owned, streamed, resident, pt, forced) -> (head[6], ranges[nch, 2])."""
    cases = list(itertools.product(LENGTHS, LENGTHS, RESIDENT, PTS, FORCED))
    assert len(cases) == 19044
    flat = run(driver, "chunks", cases)
    plans, at = {}, 0
    for case in cases:
        head = flat[at:at + 6]
        nch = int(head[0])
        assert nch >= 1
        plans[case] = (head, flat[at + 6:at + 6 + 2 * nch].reshape(nch, 2))
        at += 6 + 2 * nch
    assert at == flat.size
    return plans


def test_chunks_tile_the_streamed_side(chunk_plans):
    for (owned, n, resident, pt, forced), (head, rng) in chunk_plans.items():
        case = (owned, n, resident, pt, forced)
        b, e = rng[:, 0], rng[:, 1]
        assert b[0] == 0 and e[-1] == n, case
        assert np.array_equal(b[1:], e[:-1]), case                       # ascending and contiguous
        assert np.all(e > b), case                                       # none empty
        assert np.all(b % 64 == 0), case                                 # every chunk starts on a 64-point quarter


def test_chunk_count_and_balance(chunk_plans):
    for case, (head, rng) in chunk_plans.items():
        nch, chunks, len_big, len_tail, n_big, _ = (int(v) for v in head)
        assert nch == chunks == rng.shape[0], case
        assert len_big % 64 == 0 and len_tail % 64 == 0 and len_tail > 0, case
        assert 0 <= len_big - len_tail <= 64, case


def test_fair_exactly_in_one_round_launches(chunk_plans):
    for (owned, n, resident, pt, forced), (head, _) in chunk_plans.items():
        blocks = -(-owned // (64 * pt))
        assert bool(head[5]) == (resident > 0 and int(head[0]) * blocks <= resident), (owned, n, resident, pt, forced)


def test_workspaces_are_sized_by_the_launchers_plans(driver):
    sizes = list(itertools.product(LENGTHS, LENGTHS))
    for resident in RESIDENT:
        col = run(driver, "colsum", [(m, n, 0, resident) for m, n in sizes]).reshape(-1, 5)
        row = run(driver, "rowstats", [(m, n, resident) for m, n in sizes]).reshape(-1, 5)
        for (m, n), c, r in zip(sizes, col, row):
            assert c[1] == c[2] and r[1] == r[2], (m, n, resident)       # nch == plan.chunks(streamed)
            assert c[4] == c[1] * n, (m, n, resident)                    # cpd_colsum_ws_doubles == nch N
            assert r[4] == 4 * r[1] * m, (m, n, resident)                # cpd_rowstats_ws_doubles == 4 nch M
    # a forced count is the count (wherever the streamed side has that many quarters)
    forced = run(driver, "colsum", [(m, 5500, f, 1024) for m in LENGTHS for f in (1, 3, 7)]).reshape(-1, 5)
    for (m, f), c in zip(((m, f) for m in LENGTHS for f in (1, 3, 7)), forced):
        if -(-m // 64) >= f:
            assert c[1] == f, (m, f)


def test_instance_selection(driver):
    cols = np.arange(1, 40000)
    pt = run(driver, "colsum", np.stack([np.full_like(cols, 5000), cols, 0 * cols, 0 * cols + 1024], 1)).reshape(-1, 5)[:, 0]
    assert np.all(pt[cols <= 2048] == 1) and np.all(pt[(cols > 2048) & (cols <= 16384)] == 2) and np.all(pt[cols > 16384] == 4)
    # the table in the header of tests/test_gpu_cpd_pair_pass_variants.py: SHAPES and its instance comments
    instances = {(1500, 1700): (1, 1), (6000, 5500): (2, 2), (2341, 16584): (4, 4), (16584, 2341): (2, 4)}
    assert list(instances) == SHAPES
    got_c = run(driver, "colsum", [(m, n, 0, 1024) for m, n in SHAPES]).reshape(-1, 5)[:, 0]
    got_r = run(driver, "rowstats", [(m, n, 1024) for m, n in SHAPES]).reshape(-1, 5)[:, 0]
    assert [(int(a), int(b)) for a, b in zip(got_c, got_r)] == list(instances.values())
    # row statistics: 1 where both sides are at most 2 048; 2 up to 2 048 rows, or with both sides at most 16 384; else 4 -- and
    # monotone: more rows or more targets never take fewer points per thread
    sizes = list(itertools.product(LENGTHS, LENGTHS))
    rpt = run(driver, "rowstats", [(m, n, 1024) for m, n in sizes]).reshape(-1, 5)[:, 0].reshape(len(LENGTHS), len(LENGTHS))
    for i, m in enumerate(LENGTHS):
        for j, n in enumerate(LENGTHS):
            want = 1 if (m <= 2048 and n <= 2048) else (2 if (m <= 2048 or (m <= 16384 and n <= 16384)) else 4)
            assert rpt[i, j] == want, (m, n)
    assert np.all(np.diff(rpt, axis=0) >= 0) and np.all(np.diff(rpt, axis=1) >= 0)


def test_nn_plans(driver):
    sizes = list(itertools.product(LENGTHS, LENGTHS))
    out = run(driver, "nn", sizes).reshape(-1, 4)
    for (m, n), (nc_p, len_p, nc_u, len_u) in zip(sizes, out):
        for nc, ln in ((nc_p, len_p), (nc_u, len_u)):
            assert ln > 0 and ln % 256 == 0 and nc >= 1 and nc * ln >= n, (m, n)
        assert nc_p <= nc_u, (m, n)                                      # nn_ws_bytes sizes by the unpruned plan


def test_nn_small_slices_stay_inside_their_bounds(driver):
    """The planner states two bounds on the slice count s: s <= ceil(N / 32) ("at least 32 targets per slice") and
    s >= ceil(N / 2048) ("at most 2 048 targets per slice": 48 KB of LDS).  ceil(N / 2048) <= ceil(N / 32), so both always hold.
    The launcher cuts slices of ceil(N / s) targets: never more than 2 048.  The lower bound is on the COUNT: ceil(N / s) itself can
    come out below 32 (N = 65: three slices of 22; N = 257: nine of 29 -- the only two target counts of this grid where it does),
    which the kernel handles; what holds is that s - 1 slices of 32 fit into N."""
    sizes = list(itertools.product(LENGTHS, LENGTHS))
    s = run(driver, "small", sizes)
    for (m, n), k in zip(sizes, s):
        k = int(k)
        assert -(-n // 2048) <= k <= max(1, -(-n // 32)), (m, n)
        assert -(-n // k) <= 2048, (m, n)
        assert (k - 1) * 32 < n, (m, n)
