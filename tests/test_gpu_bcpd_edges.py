"""GPU tests of the BCPD kernels (gingr_amd/csrc/bcpd.hip) at their size, chunk, clamp and parameter edges.  Every test is ONE
Iteration() from an injected state, set against bcpd_restatement.Problem.iterate of the same state, through test_gpu_bcpd.compare.
Inputs, references and guards are in tests/bcpd_edge_cases.py; each test asserts its guard first, from the restatement alone
(tests/test_bcpd_host.py asserts the same guards without a device).

Guards (all from the restatement; br = bcpd_restatement, ec = bcpd_edge_cases)
  a  size edges      ec.SIZE_EDGES lists for each (M, N) the padded length Mp = round_up(M, 64), its padded rows (0, 1, 47, 59, 63), the
                     number of 64-row blocks nb (1 .. 17) and the chunk counts of the column and the row pass (1 .. 5, all of one tile);
                     size_guard holds br.padded and br.plan_chunks to that list.  (576, 700): 3 and 3 chunks; (1025, 300): 5 column chunks.
  b  two-tile chunks br.plan_chunks(64, 65537) = (129, 512) for the row pass; (513, 130817): (2, 512) for the column pass and (256, 512)
                     for the row pass -- the last chunk holds one point in all three.  One point fewer and every chunk is one tile.
  c  same bits       more than two chunks in at least one pass
  d  clamp           br.clamp_figure = 3 am^2 . 2048 log2(e) / (2 sigma2), am from the data, >= 2^41 (far point: 2.1e3 x 2^41) or
                     < 2^41 (unmoved: 9e-8 x 2^41); the restatement finite; the far point's nu' / the far row's nu exactly 0 there
  e  parameters      the restatement finite; kappa = 1e-3: some <alpha_m> of the restatement exactly 0 (155 of 216 rows are below 1e-300
                     after 10 iterations: a small kappa prunes the mixture)

Tolerances.  a, b, c, d and e but for lambda = 0.1: those of test_gpu_bcpd.compare, unchanged (1e-9 for vectors, sigma_m^2 / max K_mm, s and
R; 1e-8 for the variances).  b adds nu_m and nu'_n element by element at the same 1e-9: they are sums of positive terms, each good to
the 1.5e-13 the exponential's argument (up to 700) loses in its last bit, so the norm-wise bound holds entry by entry.  <alpha_m> element
by element (e): 1e-9 relative, the bound of the norm, wherever the restatement's value is >= 1e-300; at most 1e-300 wherever it is not.
lambda = 0.1 (K = 10 G: v^ is the small difference of two large vectors) and f (xPx - 2 PX . y^ + nu |y^|^2 at |x| = 1e4 cancels eight
digits in the restatement too): rot3_cases.bound(usual, spread, ill=True), i.e. the usual bound or 10 x the restatement's own spread
over 8 perturbations of 2^-52 of (yhat, x) where that is larger.  The spread comes from the restatement, never from the device.

Measured on the MI355X (largest deviation over the cases of a group; spread and bound where the bound is not the fixed one):

  group                          yhat     vhat     alpha    nu       nu'      sig_m^2  s        R        t        sigma2   sbar2
  a  from initial (22 cases)     2.4e-15  7.4e-16  2.2e-15  5.6e-16  1.1e-15  6.9e-16  1.8e-15  1.9e-15  2.4e-15  1.7e-15  4.5e-16
  a  from crafted (22 cases)     1.3e-15  4.6e-14  1.5e-15  2.8e-16  3.3e-16  4.4e-15  8.6e-16  2.0e-15  1.6e-15  1.1e-13  8.6e-15
  b  64 x 65537, w = 0.1         1.1e-14  2.3e-12  6.5e-16  3.4e-16  1.3e-16  2.2e-15  2.4e-15  3.1e-15  5.7e-15  6.1e-14  1.9e-13
  b  64 x 65537, w = 0           9.2e-15  1.9e-12  6.0e-16  3.3e-16  1.0e-16  2.2e-15  5.1e-15  4.4e-15  4.2e-15  1.0e-13  4.7e-15
  b  513 x 130817, w = 0.1       4.6e-14  4.9e-12  8.1e-16  4.7e-16  2.4e-16  6.8e-15  3.9e-15  1.4e-14  1.9e-14  3.3e-13  9.3e-14
  d  far target point (clamp)    7.9e-16  2.7e-15  8.7e-16  4.0e-16  5.7e-16  8.3e-16  6.5e-16  1.1e-15  2.5e-15  1.4e-15  2.2e-16
  d  far template row (clamp)    7.8e-16  3.5e-15  1.5e-15  3.8e-16  6.1e-16  5.6e-16  1.3e-16  1.9e-15  3.6e-15  2.0e-15  0
  d  unmoved (no clamp)          5.3e-16  3.2e-15  6.9e-16  3.9e-16  6.6e-16  6.3e-16  4.0e-16  8.9e-16  1.2e-15  1.8e-15  2.1e-16
  e  kappa 1e-3, 0.5, 7, 1e6     1.4e-15  6.7e-15  1.6e-15  4.9e-16  6.5e-16  6.3e-16  1.6e-15  1.6e-15  1.1e-14  6.5e-15  3.7e-16
  e  beta 0.3, 6                 1.2e-15  1.5e-14  8.3e-16  4.2e-16  6.2e-16  1.7e-15  9.9e-16  1.2e-15  7.0e-15  3.7e-15  4.3e-16
  e  lambda 1e4, w 0.9, gamma 10 1.4e-15  1.7e-13  1.5e-15  4.4e-16  6.4e-16  1.4e-16  2.0e-15  2.4e-15  9.6e-15  2.8e-15  2.8e-16
  e  lambda 0.1 (from 10)        4.6e-16  2.7e-11  5.1e-16  3.6e-16  5.2e-16  0        8.4e-13  8.7e-13  4.6e-16  5.4e-16  0
       the restatement's spread  4.4e-16  5.6e-11  1.8e-15  4.7e-16  1.2e-15  0        1.8e-12  2.6e-12  2.9e-16  6.7e-16  1.8e-16
  f  offset 1e4, from 0          7.4e-16  2.4e-12  8.7e-16  4.1e-16  5.4e-16  8.3e-16  1.1e-13  1.5e-13  1.2e-12  3.3e-08  1.9e-16
       the restatement's spread  2.0e-15  4.9e-12  8.6e-13  1.7e-12  1.5e-12  1.3e-13  1.1e-13  1.2e-13  1.1e-12  4.4e-08  1.0e-13
  f  offset 1e4, from 10         5.4e-16  8.9e-12  7.1e-16  4.3e-16  6.1e-16  6.9e-16  1.0e-13  8.8e-14  6.4e-13  1.0e-14  2.1e-16
       the restatement's spread  1.8e-15  1.7e-11  1.4e-12  2.6e-12  2.4e-12  1.6e-13  7.9e-14  8.9e-14  7.9e-13  3.4e-08  7.1e-14

Only sigma2 of f has a bound other than the fixed one: 4.4e-7 from the initial state and 3.4e-7 from the state after 10 iterations
(10 x the spread), against deviations of 3.3e-8 and 1.0e-14 -- the device is inside the restatement's own spread, so the variance sums
stay as they are.  lambda = 0.1 stays under the fixed bounds; its spread (v^ 5.6e-11) is recorded all the same.  <alpha_m> element by
element: <= 5.7e-14 at kappa = 1e-3 (61 rows at or above 1e-300, the device exactly 0 on the other 155), <= 3.7e-15 elsewhere.
"""
import numpy as np
import pytest

from tests import bcpd_edge_cases as ec
from tests import bcpd_restatement as br
from tests import rot3_cases as rc
from tests.test_gpu_bcpd import compare, figures, inject, make

pytestmark = pytest.mark.gpu

# test_gpu_bcpd.compare's bounds by name, for the cases whose bound is rot3_cases.bound(well, spread, ill=True)
WELL = dict(yhat=1e-9, vhat=1e-9, uhat=1e-9, alpha=1e-9, nu=1e-9, nu_prime=1e-9, sigma_diag=1e-9, t=1e-9, Nhat=1e-9, s=1e-9, R=1e-9,
            sigma2=1e-8, sigma_bar2=1e-8)


def one_iteration(reg, st):
    inject(reg, st)
    reg.Iteration()
    return reg.state()


def compare_with_spread(got, want, p, st, label):
    """`compare` with every bound the usual one or 10 x the restatement's own spread over (yhat, x), where that is larger"""
    base, spread = rc.oracle_spread(ec.iteration_outputs(p, st), (st.yhat, p.x))
    spread = ec.spread_on_figure_scale(base, spread, p)
    fig = figures(got, want, p)
    fig["uhat"] = br.rel(p.y + got["vhat"], p.y + want.vhat)
    rows = {k: (fig[k], spread[k], rc.bound(WELL[k], spread[k], True)) for k in WELL}
    print(label + ": " + "; ".join(f"{k} dev {d:.2e} spread {s:.2e} bound {b:.2e}" for k, (d, s, b) in rows.items()))
    for k, (d, s, b) in rows.items():
        assert d < b, (label, k, d, s, b)


def compare_alpha_elementwise(got, want, label):
    """<alpha_m> row by row: 1e-9 relative wherever the restatement's value is a normal number, and no more than that floor where
    the restatement's has gone below it (psi(kappa + nu_m) - psi(kappa M + N^) under the logarithm of the smallest double)"""
    big = want.alpha >= ec.ALPHA_FLOOR
    err = np.abs(got["alpha"][big] - want.alpha[big]) / want.alpha[big]
    print(f"{label}: alpha element-wise max rel {err.max():.2e} over {int(big.sum())} rows, {int((~big).sum())} rows below {ec.ALPHA_FLOOR:g}"
          f" (device max there {got['alpha'][~big].max() if (~big).any() else 0.0:.2e}), smallest alpha {want.alpha.min():.2e}")
    assert (err < 1e-9).all(), (label, float(err.max()))
    assert (got["alpha"][~big] <= ec.ALPHA_FLOOR).all() and (got["alpha"] >= 0.0).all(), label


# ---------------------------------------------------------------------------------------------------------- a. size edges
@pytest.mark.parametrize("w", [0.0, 0.1])
@pytest.mark.parametrize("M,N", list(ec.SIZE_EDGES))
def test_size_edges(ctx, M, N, w):
    """Mp and its padding (none; 1; 63 rows), nb = 1, M < 16, M and N at 255 / 256 / 257, up to five chunks with a ragged last one"""
    ec.size_guard(M, N)
    p = ec.cloud_problem(M, N, w)
    reg = make(ctx, p)
    try:
        assert abs(reg.sigma2() - ec.cloud_state(M, N, w, "initial").sigma2) < 1e-12 * reg.sigma2()
        for start in ec.STARTS:
            st = ec.cloud_state(M, N, w, start)
            compare(one_iteration(reg, st), ec.cloud_reference(M, N, w, start), p, label=f"size {M}x{N} w={w} {start}")
    finally:
        reg.close()


# --------------------------------------------------------------------------------------------------- b. multi-tile chunks
@pytest.mark.parametrize("M,N,w", [(64, 65537, 0.1), (64, 65537, 0.0), (513, 130817, 0.1)])
def test_chunks_of_two_tiles(ctx, M, N, w):
    """the second trip of the tile loop of both pair passes, 129 and 256 chunks, a last chunk of one point; every nu'_n (the last
    target point is alone in its chunk), and nu_m, PX_m of every row through v^, y^ and the transform"""
    ec.multi_tile_guard(M, N)
    p, st, want = ec.cloud_problem(M, N, w), ec.cloud_state(M, N, w, "crafted"), ec.cloud_reference(M, N, w, "crafted")
    reg = make(ctx, p)
    try:
        got = one_iteration(reg, st)
        compare(got, want, p, label=f"two-tile {M}x{N} w={w}")
        # compare holds nu and nu' by norm; here also element by element, so that the one point of the last chunk counts by itself
        assert np.abs(got["nu_prime"] - want.nu_prime).max() < 1e-9 * want.nu_prime.max()
        assert abs(got["nu_prime"][-1] - want.nu_prime[-1]) < 1e-9 * want.nu_prime[-1]
        assert (np.abs(got["nu"] - want.nu) < 1e-9 * want.nu).all()
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ c. two runs, same bits
@pytest.mark.parametrize("M,N", [(64, 65537), (576, 700)])
def test_two_runs_from_the_same_state_give_the_same_bits(ctx, M, N):
    """129 row chunks of two tiles; three chunks in both passes: the partials are added in chunk order"""
    plan = ec.chunks(M, N)
    assert max(plan["col"][0], plan["row"][0]) > 2
    p, st = ec.cloud_problem(M, N, 0.1), ec.cloud_state(M, N, 0.1, "crafted")
    reg = make(ctx, p)
    try:
        a = one_iteration(reg, st)
        b = one_iteration(reg, st)
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ d. clamp branch, by value
@pytest.mark.parametrize("which", ec.CLAMP_CASES)
def test_clamped_pair_passes_by_value(ctx, which):
    """far_target, far_row: 3 am^2 . 2048 log2(e) / (2 sigma2) >= 2^41, the clamped copies of both inner loops run, and the far
    point's nu' (the far row's nu) is exactly 0 on both sides; unmoved: the same state with the condition false"""
    figure = ec.clamp_guard(which)
    assert (figure >= br.CLAMP_AT) == (which != "unmoved")
    p, st, want = ec.clamp_case(which)
    reg = make(ctx, p)
    try:
        got = one_iteration(reg, st)
        compare(got, want, p, label=f"clamp {which} figure/2^41={figure / br.CLAMP_AT:.2e}")
        if which == "far_target":
            assert want.nu_prime[ec.FAR_INDEX] == 0.0 and got["nu_prime"][ec.FAR_INDEX] == 0.0
        elif which == "far_row":
            assert want.nu[ec.FAR_INDEX] == 0.0 and got["nu"][ec.FAR_INDEX] == 0.0
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------------------- e. parameters
@pytest.mark.parametrize("name", list(ec.PARAMETER_CASES))
def test_parameters_one_at_a_time(ctx, name):
    """g6 with one parameter away from (lambda = 10, gamma = 0.3, kappa = 1, beta = 1.5, w = 0.1), from the restatement's states after
    0, 1 and 10 iterations under those parameters; <alpha_m> also element by element (the device's digamma below 1 and at 1e6)"""
    ec.parameter_guard(name)
    p, states, refs = ec.parameter_case(name)
    reg = make(ctx, p)
    try:
        for it in ec.PARAMETER_STATES:
            label = f"{name} from {it}"
            got = one_iteration(reg, states[it])
            if name == "lambda=0.1":
                compare_with_spread(got, refs[it], p, states[it], label)
            else:
                compare(got, refs[it], p, label=label)
            compare_alpha_elementwise(got, refs[it], label)
    finally:
        reg.close()


# --------------------------------------------------------------------------------------------------- f. far from the origin
def test_clouds_far_from_the_origin(ctx):
    """template and target shifted by 1e4 (the offset of test_initial_sigma2_from_moments): the restatement itself loses digits in
    xPx - 2 PX . y^ + nu |y^|^2, so every bound is the usual one or 10 x its own spread"""
    p, states, refs = ec.offset_case()
    reg = make(ctx, p)
    try:
        assert abs(reg.sigma2() - states[0].sigma2) < 1e-11 * states[0].sigma2      # the bound of test_initial_sigma2_from_moments
        for it in ec.OFFSET_STATES:
            compare_with_spread(one_iteration(reg, states[it]), refs[it], p, states[it], f"offset {ec.OFFSET:g} from {it}")
    finally:
        reg.close()
