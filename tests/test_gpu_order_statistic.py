"""GPU tests of the exact order statistic (gingr_order_statistic / Context.order_statistic, gingr_amd/csrc/robust_select.hip): the radix
selection over the bit patterns of non-negative doubles, at the sizes where the grid changes (one workgroup up to 2 048 keys, 33 at
65 537), at the first, the lower-median and the last rank, on inputs that put all the work into one digit or one bin.  Expected: the
element np.partition puts at position k, bit for bit, twice."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_BAD_ARGUMENT, ERR_NONFINITE = 1, 3
SIZES = [1, 2, 255, 256, 257, 1000, 65537]


def inputs(n):
    """name -> (n,) non-negative doubles"""
    rng = np.random.default_rng(n)
    low = (np.uint64(0x3FF0000000000000) | rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)            # the last digit only
    high = ((rng.integers(0, 0x80, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0000123456789ABC)).view(np.float64)  # the first only
    denormal = np.where(rng.random(n) < 0.5, 0.0, rng.integers(1, 1000, n).astype(np.uint64).view(np.float64))
    with_inf = rng.exponential(3.0, n)
    with_inf[n // 2] = np.inf
    return {"random": rng.exponential(10.0, n) ** 3, "equal": np.full(n, 2.75), "ties": rng.integers(0, 4, n).astype(np.float64),
            "zeros and denormals": denormal, "inf among finite": with_inf, "lowest digit": low, "highest digit": high}


@pytest.mark.parametrize("n", SIZES)
def test_every_rank_equals_partition_bit_for_bit(ctx, n):
    for name, v in inputs(n).items():
        assert np.isfinite(v).sum() >= n - 1 and (v >= 0).all(), name
        for k in sorted({0, (n - 1) // 2, n - 1}):
            want = np.partition(v, k)[k]
            got, again = ctx.order_statistic(v, k), ctx.order_statistic(v, k)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (name, n, k, got, want)
            assert np.float64(again).view(np.uint64) == np.float64(got).view(np.uint64), (name, n, k)


def test_more_keys_than_the_widest_grid_has_threads_for(ctx):
    n = 64 * 2048 + 1                                                                     # 64 workgroups, each striding over the keys
    rng = np.random.default_rng(9)
    for name, v in (("random", rng.exponential(10.0, n) ** 3), ("ties", rng.integers(0, 4, n).astype(np.float64))):
        for k in (0, (n - 1) // 2, n - 1):
            want = np.partition(v, k)[k]
            got = ctx.order_statistic(v, k)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (name, k, got, want)


def test_inf_is_a_value_and_the_last_rank_finds_it(ctx):
    v = np.array([3.0, np.inf, 0.0, 5e-324, 1.0])
    assert [ctx.order_statistic(v, k) for k in range(5)] == [0.0, 5e-324, 1.0, 3.0, np.inf]
    assert ctx.order_statistic(np.array([np.inf, np.inf]), 0) == np.inf


def test_refusals(ctx):
    from gingr_amd._native import dptr
    lib, h = ctx._lib, ctx.handle
    v = np.array([1.0, 2.0, 3.0])
    out = ctypes.c_double(-7.0)

    def call(values, n, k):
        return lib.gingr_order_statistic(h, n, dptr(values), k, ctypes.byref(out))

    assert call(v, 3, 1) == 0 and out.value == 2.0
    out.value = -7.0
    for bad in (np.array([1.0, -1e-300, 3.0]), np.array([1.0, np.nan, 3.0]), np.array([-np.inf, 1.0, 2.0])):
        assert call(bad, 3, 1) == ERR_NONFINITE and out.value == -7.0
    for n, k in ((3, -1), (3, 3), (3, 100), (0, 0), (-2, 0)):
        assert call(v, n, k) == ERR_BAD_ARGUMENT and out.value == -7.0, (n, k)
    assert lib.gingr_order_statistic(h, 3, None, 1, ctypes.byref(out)) == ERR_BAD_ARGUMENT
    assert lib.gingr_order_statistic(h, 3, dptr(v), 1, None) == ERR_BAD_ARGUMENT
    assert lib.gingr_order_statistic(None, 3, dptr(v), 1, ctypes.byref(out)) == ERR_BAD_ARGUMENT
    with pytest.raises(Exception):
        ctx.order_statistic(np.array([1.0, np.nan]), 0)
    assert ctx.order_statistic(v, 2) == 3.0                                               # and the context still works
