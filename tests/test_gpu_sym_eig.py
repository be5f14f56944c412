"""sym_eig / sym_eig_strided (gingr_amd/csrc/sym_eig.hip) on matrices chosen for their kernels: the register kernel at its three
templates and their edges, alone, strided and in mixed batches; the block kernel at every block count and row padding; the two two-sided
kernels through the fallback; a failed pivot beside problems that factor; a null space of several dimensions.

The entries are called by tests/c/sym_eig_driver.cpp, a g++ program linked against libgingr_hip.so (no Python in the process, one fresh
child per test: the device is initialised once per test).  Matrices, reference and judgement are tests/sym_eig_cases.py; every figure
is relative to lambda_1 and held to 1000 x EIG_ROUTE_SPREAD, the spread of two correct host routes that
tests/test_sym_eig_cases_host.py measures.  Every sym_eig problem has row stride n + 3 with NaN outside its
leading n x n block, and the outputs are NaN before the call: a read past the block or an entry left unwritten poisons the figures."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import sym_eig_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1000.0 * sc.EIG_ROUTE_SPREAD
GINGR_OK, GINGR_ERR_NONFINITE = 0, 3
SYM_EIG, SYM_EIG_STRIDED = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sym_eig") / "sym_eig_driver")
    libdir = os.path.join(ROOT, "gingr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "sym_eig_driver.cpp"), "-o", exe, "-L", libdir,
                           "-lgingr_hip", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def padded(G, ldg):
    P = np.full((ldg, ldg), np.nan)
    P[:G.shape[0], :G.shape[0]] = G
    return P


def by_pointer(cases, blocks=False):
    """one sym_eig call of the problems `cases` [(kind, n, variant)], row stride n + 3"""
    return (SYM_EIG, blocks, list(cases), 3)


def strided(cases):
    """one sym_eig_strided call (the entry has no row stride: ldg = n)"""
    return (SYM_EIG_STRIDED, False, list(cases), 0)


def run(driver, tmp_path, calls):
    """the calls in one fresh process -> per call (return code, error text, [(evals, V)] per problem)"""
    inp, outp = str(tmp_path / "calls.bin"), str(tmp_path / "results.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<q", len(calls)))
        for entry, blocks, cases, pad in calls:
            f.write(struct.pack("<qqq", entry, int(blocks), len(cases)))
            for kind, n, variant in cases:
                f.write(struct.pack("<qq", n, n + pad))
                padded(sc.matrix(kind, n, variant), n + pad).tofile(f)
    done = subprocess.run([driver, inp, outp], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    results = []
    with open(outp, "rb") as f:
        for entry, blocks, cases, pad in calls:
            rc, length = struct.unpack("<qq", f.read(16))
            text = f.read(length).decode()
            problems = []
            for kind, n, variant in cases:
                evals = np.fromfile(f, dtype=np.float64, count=n)
                V = np.fromfile(f, dtype=np.float64, count=n * n).reshape(n, n)
                problems.append((evals, V))
            results.append((rc, text, problems))
        assert f.read() == b""
    return results


class Worst:
    """the largest figures of a group of problems, for the printout"""

    def __init__(self):
        self.by_group = {}

    def add(self, group, figures):
        old = self.by_group.get(group, (0.0, 0.0, 0.0))
        self.by_group[group] = tuple(max(a, b) for a, b in zip(old, figures[:3]))

    def report(self):
        for group, (resid, orth, err) in self.by_group.items():
            print(f"largest  {group:42s} resid {resid:.2e} orth {orth:.2e} evals {err:.2e}   (bound {TOL:.2e})")


def check(case, result, worst=None, group=None):
    kind, n, variant = case
    evals, V = result
    figures = sc.judge(sc.matrix(kind, n, variant), evals, V, sc.reference_spectrum(kind, n, variant))
    print(f"{kind:13s} n={n:3d} v={variant}  resid {figures[0]:.2e} orth {figures[1]:.2e} evals {figures[2]:.2e} "
          f"{'non-increasing' if figures[3] else 'NOT non-increasing'}")
    if worst is not None:
        worst.add(group, figures)
    assert figures[0] <= TOL and figures[1] <= TOL and figures[2] <= TOL and figures[3], (case, figures, TOL)
    return figures


def check_calls(calls, results, worst, group_of):
    """every call GINGR_OK, every problem within the bound"""
    for (entry, blocks, cases, pad), (rc, text, problems) in zip(calls, results):
        assert rc == GINGR_OK, (cases, rc, text)
        for case, result in zip(cases, problems):
            check(case, result, worst, group_of(case, cases))


def register_class(n):
    return "<1,2> n <= 64" if n <= 64 else ("<2,4> n <= 128" if n <= 128 else "<3,6> n <= 192")


def block_class(n):
    return f"E = {(n + 63) // 64}"


def test_register_kernel_alone(driver, tmp_path):
    """one problem a call: ring slots padded and not, odd and even n, fewer waves than 16, the three templates on both sides of their
    edges; identity and diagonal matrices (no rotation at all; a permuted diagonal: the rank sort alone).  (`shifted` at n = 1 is the
    1 x 1 zero matrix: its pivot fails and the one-workgroup two-sided kernel answers.)"""
    calls = [by_pointer([(kind, n, 0)]) for kind in sc.KINDS for n in sc.REGISTER_SIZES]
    calls += [by_pointer([(kind, n, 0)]) for kind in sc.SPECIAL_KINDS for n in sc.SPECIAL_SIZES]
    results = run(driver, tmp_path, calls)
    worst = Worst()
    try:
        check_calls(calls, results, worst, lambda case, cases: f"register {register_class(case[1])}")
    finally:
        worst.report()


def test_strided_equals_by_pointer(driver, tmp_path):
    """sym_eig_strided, four problems a launch, against four single sym_eig calls: "the same arithmetic in the same order" (eig.hip),
    so the same bits -- although one reads row stride n and the other n + 3"""
    calls = []
    for kind in sc.KINDS:
        for n in sc.STRIDED_SIZES:
            cases = [(kind, n, v) for v in range(sc.STRIDED_COUNT)]
            calls.append(strided(cases))
            calls += [by_pointer([c]) for c in cases]
    results = run(driver, tmp_path, calls)
    worst = Worst()
    try:
        check_calls(calls, results, worst, lambda case, cases: f"strided / single {register_class(case[1])}")
    finally:
        worst.report()
    step = 1 + sc.STRIDED_COUNT
    for at in range(0, len(calls), step):
        batch = results[at][2]
        for v in range(sc.STRIDED_COUNT):
            single = results[at + 1 + v][2][0]
            assert np.array_equal(batch[v][0], single[0]), calls[at][2][v]
            assert np.array_equal(batch[v][1], single[1]), calls[at][2][v]


def test_mixed_register_batches(driver, tmp_path):
    """three sizes in one launch: the template is chosen by the largest, so the small problems run in a large template with another
    ring -- compared with the bound, not bit for bit"""
    calls = [by_pointer(sc.batch_cases(sizes, kind)) for kind in sc.KINDS for sizes in sc.MIXED_BATCHES]
    results = run(driver, tmp_path, calls)
    worst = Worst()
    try:
        check_calls(calls, results, worst,
                    lambda case, cases: f"mixed: n = {case[1]} in {register_class(max(c[1] for c in cases))}")
    finally:
        worst.report()


@pytest.mark.parametrize("kind", sc.KINDS)
def test_block_kernel(driver, tmp_path, kind):
    """blocks = true: 13 blocks (odd: a padding block), 14, 15; rows padded to 256 | 320 (E = 4 | 5), E = 6, E = 8 with a full last
    block; batches of two sizes, one of them with a problem for the register kernel; the same matrix twice, the same bits"""
    calls = [by_pointer([(kind, n, 0)], blocks=True) for n in sc.BLOCK_SIZES]
    calls += [by_pointer(sc.batch_cases(sizes, kind), blocks=True) for sizes in sc.BLOCK_BATCHES]
    again = len(calls)
    calls.append(by_pointer([(kind, 225, 0)], blocks=True))
    results = run(driver, tmp_path, calls)
    worst = Worst()

    def group(case, cases):
        n = case[1]
        if n <= 192:
            return f"register {register_class(n)} beside blocks"
        return f"blocks {block_class(max(c[1] for c in cases))}" + (" (batch)" if len(cases) > 1 else "")

    try:
        check_calls(calls, results, worst, group)
    finally:
        worst.report()
    first = results[sc.BLOCK_SIZES.index(225)][2][0]
    assert np.array_equal(first[0], results[again][2][0][0]) and np.array_equal(first[1], results[again][2][0][1])


def test_two_sided_kernels_through_the_fallback(driver, tmp_path):
    """a zero eigenvalue (`null1`: the Cholesky kernels report the matrix as singular) and a zero row (`zero_row`: pivot n // 2 is
    exactly 0) send a problem on to the two-sided kernel: one workgroup up to 128 columns, the grid kernel above; blocks = false sends
    everything above 192 columns there directly; blocks = true with a failed pivot goes through the block kernel first"""
    calls = [by_pointer([(kind, n, 0)]) for kind in sc.SINGULAR_KINDS for n in sc.FALLBACK_ONE_WORKGROUP + sc.FALLBACK_GRID]
    calls += [by_pointer([("graded", n, 0)], blocks=False) for n in sc.TWO_SIDED_DIRECT]
    calls.append(by_pointer([("zero_row", sc.ZERO_ROW_BLOCKS, 0)], blocks=True))
    results = run(driver, tmp_path, calls)
    worst = Worst()
    try:
        check_calls(calls, results, worst,
                    lambda case, cases: "two-sided, one workgroup n <= 128" if case[1] <= 128 else "two-sided, grid n > 128")
    finally:
        worst.report()


def test_failed_pivot_beside_problems_that_factor(driver, tmp_path):
    """three problems of 200 columns in one blocks = true call, one of them with a pivot that fails: the other two must still be
    rotated (eig.hip sym_eig_blocks once skipped the sweeps of the whole call and reported the un-rotated Cholesky factors of the two
    as converged: residuals of order 1e-2 ... 1 with GINGR_OK)"""
    n = sc.DEFECT_SIZE
    order = [(kind, n, 0) for kind in sc.DEFECT_KINDS]
    first = [c for c in order if c[0] == "zero_row"] + [c for c in order if c[0] != "zero_row"]
    calls = [by_pointer(order, blocks=True), by_pointer(first, blocks=True)]
    results = run(driver, tmp_path, calls)
    worst = Worst()
    try:
        check_calls(calls, results, worst,
                    lambda case, cases: "failed pivot (two-sided, grid)" if case[0] == "zero_row" else "beside a failed pivot (blocks)")
    finally:
        worst.report()


def test_null_space_of_several_dimensions(driver, tmp_path):
    """rank n // 2.  The two-sided kernel is documented (pca_model.hip, step 5) as not always converging inside a null
    space of several dimensions, so the contract is: GINGR_OK means a decomposition within the bound; otherwise the code is
    GINGR_ERR_NONFINITE with the "did not converge" text, and the next call on the same context succeeds.  The only test that accepts
    a code other than GINGR_OK."""
    calls = []
    for n in sc.NULL_MANY_SIZES:
        calls += [by_pointer([("null_many", n, 0)]), by_pointer([("graded", 5, 0)])]
    results = run(driver, tmp_path, calls)
    for at in range(0, len(calls), 2):
        case = calls[at][2][0]
        rc, text, problems = results[at]
        if rc == GINGR_OK:
            print(f"null_many n = {case[1]}: GINGR_OK")
            check(case, problems[0])
        else:
            print(f"null_many n = {case[1]}: code {rc}, \"{text}\"")
            assert rc == GINGR_ERR_NONFINITE and "did not converge" in text, (case, rc, text)
        rc, text, problems = results[at + 1]
        assert rc == GINGR_OK, (rc, text)
        check(calls[at + 1][2][0], problems[0])
