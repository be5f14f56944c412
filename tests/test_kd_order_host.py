"""CPU pins of the k-d leaf order (gingr_amd/csrc/kd_order.h), the spatial order every cloud takes on the device, compiled for the
host with the address and undefined-behaviour sanitizers (and once with the thread sanitizer) into a stand-alone driver
(tests/c/kd_order_driver.cpp): a permutation, ascending inside every 64-point quarter, the same with and without threads, ties to the
lower index, NaN coordinates last, and -- for power-of-two leaf counts -- every aligned sibling pair cut along the longest axis."""
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 1024, 16384, 20000]


def compile_driver(exe, sanitize):
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                           "-pthread", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "kd_order_driver.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    return compile_driver(tmp_path_factory.mktemp("kd_order") / "kd_order_driver", "address,undefined")


def order(driver, xyz, mode="default"):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    raw = np.array([xyz.shape[0]], dtype=np.int64).tobytes() + xyz.tobytes()
    out = subprocess.run([driver, mode], input=raw, capture_output=True, check=True).stdout
    return np.frombuffer(out, dtype=np.int32)


def cloud(n, seed=0):
    return np.random.default_rng(seed).normal(0.0, [30.0, 20.0, 10.0], (n, 3))


@pytest.mark.parametrize("n", SIZES)
def test_permutation_quarters_ascending_threads_invisible(driver, n):
    xyz = cloud(n, n)
    perm = order(driver, xyz)
    assert np.array_equal(np.sort(perm), np.arange(n))
    for b in range(0, n, 64):                       # every 64-run inside a 256-leaf: original order
        assert np.all(np.diff(perm[b:b + 64]) > 0), b
    assert np.array_equal(order(driver, xyz, "serial"), perm)
    assert np.array_equal(order(driver, xyz, "parallel"), perm)


@pytest.mark.parametrize("n", [257, 1000, 20000])
def test_equal_points_keep_their_order(driver, n):
    # every split is the unique cut of the (coordinate, index) order: ties go to the lower index
    assert np.array_equal(order(driver, np.full((n, 3), 0.25)), np.arange(n))


def test_nan_coordinates_sort_last(driver):
    n = 2048
    xyz = cloud(n, 3)
    xyz[:, 0] *= 10.0                               # the top split is along x
    bad = np.random.default_rng(4).choice(n, 100, replace=False)
    xyz[bad, 0] = np.nan
    xyz[bad[:10], 1] = np.nan
    perm = order(driver, xyz)
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.all(np.isin(bad, perm[n // 2:]))      # on the top split's axis the NaN points are in the right half
    assert np.array_equal(order(driver, xyz, "serial"), perm)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_sibling_blocks_are_cut_along_the_longest_axis(driver, k):
    """Power-of-two leaf counts only: every aligned run of 64 * 2^j points is then one tree node.  (With five leaves the top cut is at
    768: nothing of this kind holds for other n.)"""
    n = 256 * 2 ** k
    xyz = cloud(n, 100 + k)
    xyz[np.random.default_rng(k).choice(n, 7, replace=False), k % 3] = np.nan
    perm = order(driver, xyz).astype(np.int64)
    pts = xyz[perm]
    size = 64
    while 2 * size <= n:
        for b in range(0, n, 2 * size):
            both = pts[b:b + 2 * size]
            ax = int(np.argmax(np.nanmax(both, 0) - np.nanmin(both, 0)))        # first of equal extents, as the split
            key = np.where(np.isnan(both[:, ax]), 1e300, both[:, ax])           # NaN sorts last
            idx = perm[b:b + 2 * size]
            lk, li, rk, ri = key[:size], idx[:size], key[size:], idx[size:]
            # every point of the left block precedes every point of the right one in the (coordinate, index) order
            top = lk.max()
            low = rk.min()
            assert top <= low, (size, b)
            if top == low:
                assert li[lk == top].max() < ri[rk == low].min(), (size, b)
        size *= 2


def test_threads_are_race_free(tmp_path):
    """The same driver under the thread sanitizer, with the library's thread setting at a size that uses it.  The sanitizer's runtime
    refuses to start under more address-space randomisation than it was built for ("unexpected memory mapping", before main): the
    driver runs with randomisation off for itself where setarch can do that, and a host where it still cannot start has no verdict."""
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = compile_driver(tmp_path / "kd_order_driver_tsan", "thread")
    xyz = cloud(20000, 20000)
    setarch = shutil.which("setarch")
    prefix = [setarch, platform.machine(), "-R"] if setarch else []
    p = subprocess.run(prefix + [exe, "default"], input=np.array([20000], dtype=np.int64).tobytes() + xyz.tobytes(), capture_output=True)
    if p.returncode != 0 and (b"FATAL: ThreadSanitizer" in p.stderr or b"setarch:" in p.stderr):   # (a race is a WARNING and fails below)
        pytest.skip("the thread sanitizer's runtime cannot start on this host: " + p.stderr.decode(errors="replace").strip()[:200])
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    assert np.array_equal(np.sort(np.frombuffer(p.stdout, dtype=np.int32)), np.arange(20000))
