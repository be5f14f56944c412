"""The r x r posterior solves, sampled proposals and transition densities of gingr_amd/csrc/gp.hip, kernel instance by kernel
instance, against the extended-precision reference of tests/posterior_solve_cases.py -- on INJECTED systems.

The seam: the row-sharded protocol hands the host exchange segment 1 (G [rp rp], rhs [rp], eight scalars, on the density route
Q0^T e [rp] in the tail) between phase 1 and phase 2 and expects it to be modified in place.  With one shard the `reduce` callback of
gingr_fitter_update_sharded_async / gingr_fitter_posterior_logpdf_sharded overwrites the r x r and r parts with a chosen system (the
padding stays as the Gram pass left it) and phase 2 solves whatever is there.  Nothing is added to G or rhs behind the exchange
(landmarks are added in phase 1).  Flavour: CPD with its eight sums left as found, so sigma^2 and the status do not depend on the
injected values; NoTransforms, step length 1, zero state, identity pose, so the committed alpha is (lam / (lam + eps))^2 a element by
element (posterior_solve_cases.py: alpha map) and is taken back to a through that map in extended precision.

Which instance a rank reaches is the restatement route_of / density_route_of (asserted on the host, test_posterior_solve_host.py):
    deterministic update   posterior_solve_lds_kernel<0>, <1>, posterior_solve_wide_kernel<64>, dense_spd_solve3
    sampled update         the same LDS kernels, posterior_solve_wide_kernel<64> up to rp 256, <32> above
    density (row shard)    posterior_logpdf_lds_kernel<false>, posterior_logpdf_wide_kernel<64>, <32>, two dense solves
posterior_solve_lds_kernel<2> (the three-block solve of a coordinate-separable model, uses_compact) takes the same injection with a
separable model in `parts`: tests/test_gpu_separable_edges.py.
Layer B (test_real_state_readback) reaches what injection cannot -- posterior_logpdf_split_kernel and the two
posterior_logpdf_cached_kernel instances, plus the wide / dense density once more: a real CPD state whose model's lam spans
[1e-3, 1e6], G / rhs / Q0^T e copied OUT of segment 1 by a read-only callback of the row-shard density, then the same state asked
through the single-shard gingr_fitter_posterior_logpdf_cpd twice (fresh, then cached) and every value held against the reference of
the copied-out system.  Family 6 (test_eigen_route) injects rhs alone into the point-cloud ICP flavour without landmarks:
posterior_solve_eig_kernel up to rank 192 (eig_ready), the Cholesky routes on the device's own G = S_tot / sigma^2 above.
posterior_sample_cached_kernel and the split kernel in the form that leaves the factor of I + G (keep_factor) run only behind
gingr_fitter_mh_step: test_real_state_mh_step takes the same kind of state (rp <= 112) through one step with need_forward (fresh
sampled solve, split kernel with keep_factor), gingr_fitter_mh_restore, and a second step whose proposal is the cached sample.

Bounds: 1000 x the figure of the plain float64 route (np.linalg.cholesky, two triangular solves, same density formula, same alpha
map) for the family and output, maximum over the ranks ("1 000 x the spread"); measured by the host file:

    family        forward   backward  sample fwd  sample bwd  density      (float64 route; the GPU bound is 1000 x)
    well          7.07e-14  8.08e-17  6.24e-14    8.00e-16    9.94e-16
    ill           4.75e-09  1.50e-16  4.31e-09    2.54e-13    5.36e-11
    graded_up     6.86e-14  7.06e-17  5.61e-14    4.34e-14    3.43e-15
    graded_down   2.44e-14  8.74e-17  1.74e-14    1.79e-14    1.75e-15
    zero          2.45e-16  1.23e-16  2.30e-16    3.04e-16    1.91e-16
    diagonal      4.10e-16  2.05e-16  2.39e-16    3.28e-16    3.71e-16

Closed form G = 0 (a = rhs, sample = rhs + z exactly): element by element within 4 ulp plus the rounding of the post-solve map itself,
which is not the solve's and cannot be separated from it (a is not exported) -- alpha_i = sum_d sum_j T^d_ij a_j with
T^d = Binv S[d][d] C / eps, whose off-diagonal entries of size sqrt(lam_j / lam_i) cancel only in the sum over d; every term is a
length-rp accumulation of products of length-rp accumulations, which the probabilistic rounding bound (Higham & Mary 2019:
gamma~_n = lambda sqrt(n) u, lambda = 4) puts at |delta alpha_i| <= 4 sqrt(rp + 4) 2^-53 sum_d sum_j |T^d_ij| |a_j|.  The same term
is added to the eigen family's bounds, whose float64 figures (a diagonal system) are far below what the map alone leaves.

Eigen route, backward error.  posterior_solve_eig_kernel forms a = V ((V^T rhs) / (1 + lam / sigma^2)) with a computed V that is
orthogonal to rounding only, so its error in a is of order u |a| in EVERY direction, the stiff ones included: normwise backward stable
(two length-r products: 4 sqrt(rp) 2^-53 with the probabilistic constant), and no better.  The float64 Cholesky of the nearly
diagonal I + S_tot / sigma^2 leaves 1e-19 .. 1e-17 there, which 1000 x cannot cover for any eigenvector method (MI355X: 6.3e-16 at
r = 128, full S_tot, sigma^2 = 0.1, against 1000 x 3.9e-19); that one bound therefore carries 4 sqrt(rp) 2^-53 on top.

Measured on an MI355X.  Every test prints its own rows (route, case, figure, MI355X, bound, float64); the table below was collated
from those prints of one run of this file -- per route and case the row closest to its bound over all ranks.  No code here produces
the aggregate.  The eigen and real-state bounds are per case, so theirs is the bound of that row:

    route                                        case          figure                             MI355X    bound     float64
    dense_spd_solve3                             diagonal      forward                            1.02e-14  4.10e-13  4.10e-16
    dense_spd_solve3                             diagonal      backward                           7.10e-16  2.05e-13  2.05e-16
    dense_spd_solve3                             graded_down   forward                            2.05e-14  2.44e-11  2.44e-14
    dense_spd_solve3                             graded_down   backward                           4.41e-17  8.74e-14  8.74e-17
    dense_spd_solve3                             graded_up     forward                            1.34e-13  6.86e-11  6.86e-14
    dense_spd_solve3                             graded_up     backward                           2.01e-15  7.06e-14  7.06e-17
    dense_spd_solve3                             ill           forward                            4.62e-09  4.75e-06  4.75e-09
    dense_spd_solve3                             ill           backward                           7.04e-16  1.50e-13  1.50e-16
    dense_spd_solve3                             orth s2=0.1   forward                            6.72e-16  4.23e-13  3.65e-16
    dense_spd_solve3                             orth s2=0.1   backward                           1.77e-19  3.95e-17  1.34e-20
    dense_spd_solve3                             orth s2=100   forward                            1.23e-15  5.49e-13  2.45e-16
    dense_spd_solve3                             orth s2=100   backward                           4.19e-18  2.12e-15  1.18e-18
    dense_spd_solve3                             well          forward                            6.45e-14  7.07e-11  7.07e-14
    dense_spd_solve3                             well          backward                           5.29e-16  8.08e-14  8.08e-17
    dense_spd_solve3                             zero          forward                            1.16e-14  2.45e-13  2.45e-16
    dense_spd_solve3                             zero          backward                           5.05e-16  1.23e-13  1.23e-16
    dense_spd_solve3                             zero          closed form a = rhs (x tol)        5.51e-02  1.00e+00  0.00e+00
    dense_spd_solve3 x2 + logpdf_finish_kernel   diagonal      density                            3.09e-15  3.71e-13  3.71e-16
    dense_spd_solve3 x2 + logpdf_finish_kernel   graded_down   density                            4.05e-16  1.75e-12  1.75e-15
    dense_spd_solve3 x2 + logpdf_finish_kernel   graded_up     density                            3.28e-15  3.43e-12  3.43e-15
    dense_spd_solve3 x2 + logpdf_finish_kernel   ill           density                            3.97e-14  5.36e-08  5.36e-11
    dense_spd_solve3 x2 + logpdf_finish_kernel   real state    density                            5.11e-18  2.23e-13  2.23e-16
    dense_spd_solve3 x2 + logpdf_finish_kernel   well          density                            4.47e-15  9.94e-13  9.94e-16
    dense_spd_solve3 x2 + logpdf_finish_kernel   zero          density                            7.69e-16  1.91e-13  1.91e-16
    posterior_logpdf_cached_kernel<false>        real state    density                            3.65e-16  7.60e-14  7.60e-17
    posterior_logpdf_cached_kernel<true>         real state    density                            7.55e-16  3.55e-13  3.55e-16
    posterior_logpdf_lds_kernel<false>           diagonal      density                            2.62e-15  3.71e-13  3.71e-16
    posterior_logpdf_lds_kernel<false>           graded_down   density                            1.86e-15  1.75e-12  1.75e-15
    posterior_logpdf_lds_kernel<false>           graded_up     density                            2.77e-15  3.43e-12  3.43e-15
    posterior_logpdf_lds_kernel<false>           ill           density                            1.30e-12  5.36e-08  5.36e-11
    posterior_logpdf_lds_kernel<false>           real state    density                            3.65e-16  7.60e-14  7.60e-17
    posterior_logpdf_lds_kernel<false>           well          density                            3.36e-15  9.94e-13  9.94e-16
    posterior_logpdf_lds_kernel<false>           zero          density                            5.75e-16  1.91e-13  1.91e-16
    posterior_logpdf_split_kernel                real state    density                            5.10e-16  7.60e-14  7.60e-17
    posterior_logpdf_split_kernel (keep_factor)  real state    density                            6.24e-17  6.24e-14  6.24e-17
    posterior_logpdf_wide_kernel<32>             diagonal      density                            1.51e-15  3.71e-13  3.71e-16
    posterior_logpdf_wide_kernel<32>             graded_down   density                            3.26e-16  1.75e-12  1.75e-15
    posterior_logpdf_wide_kernel<32>             graded_up     density                            4.39e-15  3.43e-12  3.43e-15
    posterior_logpdf_wide_kernel<32>             ill           density                            7.46e-14  5.36e-08  5.36e-11
    posterior_logpdf_wide_kernel<32>             well          density                            2.48e-15  9.94e-13  9.94e-16
    posterior_logpdf_wide_kernel<32>             zero          density                            4.09e-16  1.91e-13  1.91e-16
    posterior_logpdf_wide_kernel<64>             diagonal      density                            5.26e-15  3.71e-13  3.71e-16
    posterior_logpdf_wide_kernel<64>             graded_down   density                            1.01e-15  1.75e-12  1.75e-15
    posterior_logpdf_wide_kernel<64>             graded_up     density                            9.71e-15  3.43e-12  3.43e-15
    posterior_logpdf_wide_kernel<64>             ill           density                            2.00e-13  5.36e-08  5.36e-11
    posterior_logpdf_wide_kernel<64>             real state    density                            5.55e-16  3.55e-13  3.55e-16
    posterior_logpdf_wide_kernel<64>             well          density                            4.10e-15  9.94e-13  9.94e-16
    posterior_logpdf_wide_kernel<64>             zero          density                            7.16e-16  1.91e-13  1.91e-16
    posterior_sample_cached_kernel               real state    sample_forward                     8.42e-16  2.16e-13  2.16e-16
    posterior_sample_cached_kernel               real state    sample_backward                    2.01e-16  7.35e-14  7.35e-17
    posterior_solve_eig_kernel                   full S s2=0.1 forward                            1.46e-14  9.39e-13  9.03e-16
    posterior_solve_eig_kernel                   full S s2=0.1 backward                           6.26e-16  5.55e-15  3.90e-19
    posterior_solve_eig_kernel                   full S s2=100 forward                            1.00e-14  4.90e-12  4.79e-15
    posterior_solve_eig_kernel                   full S s2=100 backward                           6.50e-16  2.00e-14  1.37e-17
    posterior_solve_eig_kernel                   orth s2=0.1   forward                            6.15e-16  1.87e-13  1.74e-16
    posterior_solve_eig_kernel                   orth s2=0.1   backward                           3.39e-16  1.45e-13  1.42e-16
    posterior_solve_eig_kernel                   orth s2=100   forward                            9.10e-16  2.97e-13  2.14e-16
    posterior_solve_eig_kernel                   orth s2=100   backward                           1.39e-16  1.41e-13  1.39e-16
    posterior_solve_lds_kernel<0>                diagonal      forward                            4.31e-15  4.10e-13  4.10e-16
    posterior_solve_lds_kernel<0>                diagonal      backward                           1.02e-15  2.05e-13  2.05e-16
    posterior_solve_lds_kernel<0>                graded_down   forward                            2.00e-14  2.44e-11  2.44e-14
    posterior_solve_lds_kernel<0>                graded_down   backward                           2.50e-16  8.74e-14  8.74e-17
    posterior_solve_lds_kernel<0>                graded_up     forward                            3.46e-14  6.86e-11  6.86e-14
    posterior_solve_lds_kernel<0>                graded_up     backward                           1.44e-15  7.06e-14  7.06e-17
    posterior_solve_lds_kernel<0>                ill           forward                            1.29e-09  4.75e-06  4.75e-09
    posterior_solve_lds_kernel<0>                ill           backward                           8.06e-16  1.50e-13  1.50e-16
    posterior_solve_lds_kernel<0>                well          forward                            3.63e-14  7.07e-11  7.07e-14
    posterior_solve_lds_kernel<0>                well          backward                           4.15e-16  8.08e-14  8.08e-17
    posterior_solve_lds_kernel<0>                zero          forward                            4.91e-15  2.45e-13  2.45e-16
    posterior_solve_lds_kernel<0>                zero          backward                           7.05e-16  1.23e-13  1.23e-16
    posterior_solve_lds_kernel<0>                zero          closed form a = rhs (x tol)        1.78e-01  1.00e+00  0.00e+00
    posterior_solve_lds_kernel<0> (sampled)      diagonal      sample_forward                     5.55e-15  2.39e-13  2.39e-16
    posterior_solve_lds_kernel<0> (sampled)      diagonal      sample_backward                    2.43e-15  3.28e-13  3.28e-16
    posterior_solve_lds_kernel<0> (sampled)      graded_down   sample_forward                     1.82e-14  1.74e-11  1.74e-14
    posterior_solve_lds_kernel<0> (sampled)      graded_down   sample_backward                    1.79e-14  1.79e-11  1.79e-14
    posterior_solve_lds_kernel<0> (sampled)      graded_up     sample_forward                     2.61e-14  5.61e-11  5.61e-14
    posterior_solve_lds_kernel<0> (sampled)      graded_up     sample_backward                    4.25e-13  4.34e-11  4.34e-14
    posterior_solve_lds_kernel<0> (sampled)      ill           sample_forward                     1.15e-09  4.31e-06  4.31e-09
    posterior_solve_lds_kernel<0> (sampled)      ill           sample_backward                    3.65e-13  2.54e-10  2.54e-13
    posterior_solve_lds_kernel<0> (sampled)      real state    sample_forward                     4.99e-16  1.16e-13  1.16e-16
    posterior_solve_lds_kernel<0> (sampled)      real state    sample_backward                    2.92e-16  6.81e-14  6.81e-17
    posterior_solve_lds_kernel<0> (sampled)      well          sample_forward                     3.06e-14  6.24e-11  6.24e-14
    posterior_solve_lds_kernel<0> (sampled)      well          sample_backward                    1.13e-15  8.00e-13  8.00e-16
    posterior_solve_lds_kernel<0> (sampled)      zero          sample_forward                     5.91e-15  2.30e-13  2.30e-16
    posterior_solve_lds_kernel<0> (sampled)      zero          sample_backward                    1.20e-15  3.04e-13  3.04e-16
    posterior_solve_lds_kernel<0> (sampled)      zero          closed form rhs + z (x tol)        1.97e-01  1.00e+00  0.00e+00
    posterior_solve_lds_kernel<1>                diagonal      forward                            4.42e-15  4.10e-13  4.10e-16
    posterior_solve_lds_kernel<1>                diagonal      backward                           5.63e-16  2.05e-13  2.05e-16
    posterior_solve_lds_kernel<1>                graded_down   forward                            1.43e-14  2.44e-11  2.44e-14
    posterior_solve_lds_kernel<1>                graded_down   backward                           6.56e-17  8.74e-14  8.74e-17
    posterior_solve_lds_kernel<1>                graded_up     forward                            5.03e-14  6.86e-11  6.86e-14
    posterior_solve_lds_kernel<1>                graded_up     backward                           1.57e-15  7.06e-14  7.06e-17
    posterior_solve_lds_kernel<1>                ill           forward                            1.91e-09  4.75e-06  4.75e-09
    posterior_solve_lds_kernel<1>                ill           backward                           7.26e-16  1.50e-13  1.50e-16
    posterior_solve_lds_kernel<1>                well          forward                            3.25e-14  7.07e-11  7.07e-14
    posterior_solve_lds_kernel<1>                well          backward                           5.85e-16  8.08e-14  8.08e-17
    posterior_solve_lds_kernel<1>                zero          forward                            7.18e-15  2.45e-13  2.45e-16
    posterior_solve_lds_kernel<1>                zero          backward                           5.83e-16  1.23e-13  1.23e-16
    posterior_solve_lds_kernel<1>                zero          closed form a = rhs (x tol)        8.47e-02  1.00e+00  0.00e+00
    posterior_solve_lds_kernel<1> (sampled)      diagonal      sample_forward                     5.88e-15  2.39e-13  2.39e-16
    posterior_solve_lds_kernel<1> (sampled)      diagonal      sample_backward                    2.41e-15  3.28e-13  3.28e-16
    posterior_solve_lds_kernel<1> (sampled)      graded_down   sample_forward                     1.11e-14  1.74e-11  1.74e-14
    posterior_solve_lds_kernel<1> (sampled)      graded_down   sample_backward                    1.07e-16  1.79e-11  1.79e-14
    posterior_solve_lds_kernel<1> (sampled)      graded_up     sample_forward                     3.91e-14  5.61e-11  5.61e-14
    posterior_solve_lds_kernel<1> (sampled)      graded_up     sample_backward                    3.99e-15  4.34e-11  4.34e-14
    posterior_solve_lds_kernel<1> (sampled)      ill           sample_forward                     1.77e-09  4.31e-06  4.31e-09
    posterior_solve_lds_kernel<1> (sampled)      ill           sample_backward                    1.18e-13  2.54e-10  2.54e-13
    posterior_solve_lds_kernel<1> (sampled)      well          sample_forward                     3.12e-14  6.24e-11  6.24e-14
    posterior_solve_lds_kernel<1> (sampled)      well          sample_backward                    8.81e-16  8.00e-13  8.00e-16
    posterior_solve_lds_kernel<1> (sampled)      zero          sample_forward                     6.58e-15  2.30e-13  2.30e-16
    posterior_solve_lds_kernel<1> (sampled)      zero          sample_backward                    7.90e-16  3.04e-13  3.04e-16
    posterior_solve_lds_kernel<1> (sampled)      zero          closed form rhs + z (x tol)        8.19e-02  1.00e+00  0.00e+00
    posterior_solve_wide_kernel<32> (sampled)    diagonal      sample_forward                     1.08e-14  2.39e-13  2.39e-16
    posterior_solve_wide_kernel<32> (sampled)    diagonal      sample_backward                    4.34e-15  3.28e-13  3.28e-16
    posterior_solve_wide_kernel<32> (sampled)    graded_down   sample_forward                     2.72e-14  1.74e-11  1.74e-14
    posterior_solve_wide_kernel<32> (sampled)    graded_down   sample_backward                    6.44e-17  1.79e-11  1.79e-14
    posterior_solve_wide_kernel<32> (sampled)    graded_up     sample_forward                     2.29e-14  5.61e-11  5.61e-14
    posterior_solve_wide_kernel<32> (sampled)    graded_up     sample_backward                    2.58e-15  4.34e-11  4.34e-14
    posterior_solve_wide_kernel<32> (sampled)    ill           sample_forward                     6.37e-09  4.31e-06  4.31e-09
    posterior_solve_wide_kernel<32> (sampled)    ill           sample_backward                    2.93e-13  2.54e-10  2.54e-13
    posterior_solve_wide_kernel<32> (sampled)    well          sample_forward                     9.65e-14  6.24e-11  6.24e-14
    posterior_solve_wide_kernel<32> (sampled)    well          sample_backward                    1.34e-15  8.00e-13  8.00e-16
    posterior_solve_wide_kernel<32> (sampled)    zero          sample_forward                     1.16e-14  2.30e-13  2.30e-16
    posterior_solve_wide_kernel<32> (sampled)    zero          sample_backward                    6.92e-16  3.04e-13  3.04e-16
    posterior_solve_wide_kernel<32> (sampled)    zero          closed form rhs + z (x tol)        5.46e-02  1.00e+00  0.00e+00
    posterior_solve_wide_kernel<64>              diagonal      forward                            6.87e-15  4.10e-13  4.10e-16
    posterior_solve_wide_kernel<64>              diagonal      backward                           8.25e-16  2.05e-13  2.05e-16
    posterior_solve_wide_kernel<64>              graded_down   forward                            3.00e-14  2.44e-11  2.44e-14
    posterior_solve_wide_kernel<64>              graded_down   backward                           8.36e-17  8.74e-14  8.74e-17
    posterior_solve_wide_kernel<64>              graded_up     forward                            3.09e-14  6.86e-11  6.86e-14
    posterior_solve_wide_kernel<64>              graded_up     backward                           2.09e-15  7.06e-14  7.06e-17
    posterior_solve_wide_kernel<64>              ill           forward                            5.21e-09  4.75e-06  4.75e-09
    posterior_solve_wide_kernel<64>              ill           backward                           6.04e-16  1.50e-13  1.50e-16
    posterior_solve_wide_kernel<64>              orth s2=0.1   forward                            5.50e-16  3.21e-13  3.01e-16
    posterior_solve_wide_kernel<64>              orth s2=0.1   backward                           1.71e-19  2.44e-17  9.60e-21
    posterior_solve_wide_kernel<64>              orth s2=100   forward                            8.84e-16  4.47e-13  2.67e-16
    posterior_solve_wide_kernel<64>              orth s2=100   backward                           3.51e-18  1.95e-15  1.41e-18
    posterior_solve_wide_kernel<64>              well          forward                            5.67e-14  7.07e-11  7.07e-14
    posterior_solve_wide_kernel<64>              well          backward                           5.23e-16  8.08e-14  8.08e-17
    posterior_solve_wide_kernel<64>              zero          forward                            6.74e-15  2.45e-13  2.45e-16
    posterior_solve_wide_kernel<64>              zero          backward                           4.80e-16  1.23e-13  1.23e-16
    posterior_solve_wide_kernel<64>              zero          closed form a = rhs (x tol)        8.41e-02  1.00e+00  0.00e+00
    posterior_solve_wide_kernel<64> (sampled)    diagonal      sample_forward                     9.23e-15  2.39e-13  2.39e-16
    posterior_solve_wide_kernel<64> (sampled)    diagonal      sample_backward                    3.69e-15  3.28e-13  3.28e-16
    posterior_solve_wide_kernel<64> (sampled)    graded_down   sample_forward                     2.61e-14  1.74e-11  1.74e-14
    posterior_solve_wide_kernel<64> (sampled)    graded_down   sample_backward                    1.33e-16  1.79e-11  1.79e-14
    posterior_solve_wide_kernel<64> (sampled)    graded_up     sample_forward                     2.80e-14  5.61e-11  5.61e-14
    posterior_solve_wide_kernel<64> (sampled)    graded_up     sample_backward                    4.30e-15  4.34e-11  4.34e-14
    posterior_solve_wide_kernel<64> (sampled)    ill           sample_forward                     5.55e-09  4.31e-06  4.31e-09
    posterior_solve_wide_kernel<64> (sampled)    ill           sample_backward                    2.87e-13  2.54e-10  2.54e-13
    posterior_solve_wide_kernel<64> (sampled)    well          sample_forward                     8.10e-14  6.24e-11  6.24e-14
    posterior_solve_wide_kernel<64> (sampled)    well          sample_backward                    1.39e-15  8.00e-13  8.00e-16
    posterior_solve_wide_kernel<64> (sampled)    zero          sample_forward                     7.62e-15  2.30e-13  2.30e-16
    posterior_solve_wide_kernel<64> (sampled)    zero          sample_backward                    6.48e-16  3.04e-13  3.04e-16
    posterior_solve_wide_kernel<64> (sampled)    zero          closed form rhs + z (x tol)        7.53e-02  1.00e+00  0.00e+00
"""
import ctypes

import numpy as np
import pytest

from tests import posterior_solve_cases as pc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.have_extended(), reason="np.longdouble has no 64-bit mantissa on this platform")]

SIGMA2 = 25.0
CPD = (0.1, 1.0)  # w, lambda


class Injector:
    """One model and one single-shard fitter of rank r whose segment-1 exchange writes a chosen (G, rhs, qte)."""

    def __init__(self, ctx, r, parts=None, target=None, flavour=0, sigma2=SIGMA2):
        import gingr_amd as ga
        from gingr_amd import _native as nat
        from gingr_amd import sharded
        self.nat, self.ctx, self.r, self.rp, self.flavour, self.sigma2 = nat, ctx, r, pc.rp_of(r), flavour, sigma2
        ref, mean, U, lam = (parts or pc.model_parts(r))[:4]
        rng = np.random.default_rng(r)
        self.mesh = ref + mean
        if target is None:
            target = self.mesh[: max(150, ref.shape[0] - 13)] + rng.normal(0, 2.0, (max(150, ref.shape[0] - 13), 3))
        self.captured = None
        self.sf = sharded.ShardedFitter(ctx, ga.PointDistributionModel(ref, mean, U, lam), target, world=1,
                                        global_transform=ga.GlobalTranformationType.NoTransforms, step_length=1.0)
        p = ctypes.c_void_p()
        offs, cnts = (ctypes.c_int64 * nat.NUM_SEGMENTS)(), (ctypes.c_int64 * nat.NUM_SEGMENTS)()
        assert self.sf._lib.gingr_fitter_exchange(self.sf.handle, ctypes.byref(p), offs, cnts) == 0
        rp = self.rp
        assert cnts[1] >= rp * rp + rp + 8 + rp
        self.seg1 = sharded.as_torch(p.value + 8 * offs[1], cnts[1], ctx.device)
        self.inject = None
        self.cb = nat.ALLREDUCE_FN(self._reduce)
        self.cb_error = None

    def _reduce(self, _user, seg, _ptr, _count):
        try:
            if int(seg) != 1 or self.inject is None:
                return 0
            import torch
            r, rp, dev = self.r, self.rp, self.seg1.device
            self.ctx.synchronize()  # phase 1 has written the segment
            if self.inject == "capture":  # read only
                h = self.seg1.cpu().numpy()
                o = rp * rp + rp + 8
                self.captured = (h[: rp * rp].reshape(rp, rp)[:r, :r].copy(), h[rp * rp: rp * rp + r].copy(), h[o: o + r].copy())
                return 0
            G, rhs, qte = self.inject
            if G is not None:
                self.seg1[: rp * rp].view(rp, rp)[:r, :r] = torch.from_numpy(np.array(G)).to(dev)
            self.seg1[rp * rp: rp * rp + r] = torch.from_numpy(np.array(rhs)).to(dev)
            if qte is not None:
                o = rp * rp + rp + 8
                self.seg1[o: o + r] = torch.from_numpy(np.array(qte)).to(dev)
            torch.cuda.synchronize(dev)  # in place before phase 2 reads it
            return 0
        except BaseException as e:  # must not propagate through the C frame
            self.cb_error = e
            return 1

    def _reset(self, iteration=0):
        self.sf.set_state(np.zeros(self.r), self.sigma2, iteration=iteration)

    def update(self, G, rhs, z=None, iteration=0):
        """-> (alpha, status) of one update on the injected system"""
        nat = self.nat
        self._reset(iteration)
        self.inject = (G, rhs, None)
        cp, ip = nat.CpdParams(*CPD), nat.IcpParams(1.0, 0.5, 100)
        zz = None if z is None else nat.f64(z)
        rc = self.sf._lib.gingr_fitter_update_sharded_async(self.sf.handle, self.flavour, ctypes.byref(cp) if self.flavour == 0 else None,
                                                            ctypes.byref(ip) if self.flavour else None, 1, nat.dptr(zz), self.cb, None)
        self.inject = None
        if self.cb_error is not None:
            raise self.cb_error
        assert rc == 0, rc
        alpha, s, _ = self.sf.get_state()
        return alpha, int(s.status)

    def retry_counter(self, set_to=-1):
        v = ctypes.c_int32(-1)
        assert self.sf._lib.gingr_fitter_retry_counter(self.sf.handle, int(set_to), ctypes.byref(v)) == 0
        return int(v.value)

    def capture(self, mesh):
        """(G, rhs, Q0^T e) of the current state and `mesh`, copied out of segment 1 by the row-shard density; -> its value too"""
        self.mesh = mesh
        rc, lp = self.logpdf(None, None, None, capture=True)
        assert rc == 0, rc
        return self.captured, lp

    def logpdf_single_shard(self, mesh):
        """gingr_fitter_posterior_logpdf_cpd on the state as it stands (no reset: the memo and the factor cache stay)"""
        nat = self.nat
        cp = nat.CpdParams(*CPD)
        out = ctypes.c_double(float("nan"))
        m = nat.f64(mesh)
        rc = self.sf._lib.gingr_fitter_posterior_logpdf_cpd(self.sf.handle, ctypes.byref(cp), nat.dptr(m), ctypes.byref(out))
        return int(rc), float(out.value)

    def logpdf(self, G, rhs, qte, capture=False):
        """-> (return code, value)"""
        nat = self.nat
        self._reset()
        self.inject = "capture" if capture else (G, rhs, qte)
        cp = nat.CpdParams(*CPD)
        out = ctypes.c_double(float("nan"))
        m = nat.f64(self.mesh)
        rc = self.sf._lib.gingr_fitter_posterior_logpdf_sharded(self.sf.handle, 0, ctypes.byref(cp), None, nat.dptr(m), self.cb, None,
                                                                 ctypes.byref(out))
        self.inject = None
        if self.cb_error is not None:
            raise self.cb_error
        return int(rc), float(out.value)

    def close(self):
        self.sf.close()


def _map_rounding_bound(r, a, parts=None):
    """4 sqrt(rp + 4) 2^-53 sum_d sum_j |T^d_ij| |a_j|, T^d = Binv S[d][d] C / eps (module docstring)."""
    parts = parts or pc.model_parts(r)
    U, lam = parts[2], parts[3]
    Q = U * np.sqrt(lam)[None, :]
    S = Q.T @ Q
    left = np.linalg.inv(S + pc.EPS * np.eye(r))  # Binv / eps
    right = left @ S                               # C
    tot = np.zeros(r)
    for d in range(3):
        tot += np.abs(left @ (Q[d::3].T @ Q[d::3]) @ right) @ np.abs(a)
    return 4.0 * np.sqrt(pc.rp_of(r) + 4) * 2.0 ** -53 * tot


@pytest.mark.parametrize("r", pc.RANKS)
def test_injected_systems(ctx, r):
    inj = Injector(ctx, r)
    cmap = pc.alpha_map_ld(pc.model_parts(r)[3])
    routes = {"forward": pc.route_of(r, False), "backward": pc.route_of(r, False), "sample_forward": pc.route_of(r, True) + " (sampled)",
              "sample_backward": pc.route_of(r, True) + " (sampled)", "density": pc.density_route_of(r, "sharded")}
    failures, rows = [], []
    try:
        for fam in pc.families_at(r):
            ref = pc.reference(fam, r)
            alpha, status = inj.update(ref["G"], ref["rhs"])
            assert status == 0 and np.all(np.isfinite(alpha)), (routes["forward"], r, fam, status)
            alpha_s, status = inj.update(ref["G"], ref["rhs"], z=ref["z"])
            assert status == 0 and np.all(np.isfinite(alpha_s)), (routes["sample_forward"], r, fam, status)
            rc, lp = inj.logpdf(ref["G"], ref["rhs"], ref["qte"])
            assert rc == 0 and np.isfinite(lp), (routes["density"], r, fam, rc, lp)
            fig = pc.figures(ref, alpha.astype(pc.LD) / cmap, alpha_s.astype(pc.LD) / cmap, lp)
            for k in pc.FIGURE_NAMES:
                bound = pc.gpu_bound(fam, k, r)
                rows.append((routes[k], fam, k, fig[k], bound, pc.F64_FIGURES[fam][k]))
                if not fig[k] <= bound:
                    failures.append((routes[k], r, fam, k, fig[k], bound))
            if fam == "zero":  # closed form, element by element
                for what, got, want in (("a = rhs", alpha, ref["a"]), ("rhs + z", alpha_s, ref["s"])):
                    want_alpha = cmap * want
                    tol = 4.0 * np.spacing(np.abs(np.asarray(want_alpha, dtype=np.float64))) + _map_rounding_bound(r, np.asarray(want, dtype=np.float64))
                    dev = np.abs(np.asarray(got.astype(pc.LD) - want_alpha, dtype=np.float64))
                    worst = float(np.max(dev / tol))
                    rows.append((routes["forward"] if what == "a = rhs" else routes["sample_forward"], fam, "closed form " + what + " (x tol)", worst, 1.0, 0.0))
                    if not worst <= 1.0:
                        failures.append((what, r, fam, "closed form", worst, 1.0))
        for fam in pc.BAD_FAMILIES:  # I + G not positive definite: the reference's Try rules, nothing non-finite committed
            G, rhs, z, qdir = pc.make_case(fam, r)
            for zz in (None, z):
                alpha, status = inj.update(G, rhs, z=zz, iteration=0)  # iteration 0: state unchanged
                assert status == 0 and not alpha.any(), (pc.route_of(r, zz is not None), r, fam, status, alpha[:4])
            alpha, status = inj.update(G, rhs, iteration=1)  # later, deterministic: ModelFlexibilityError, state unchanged
            assert status == 3 and not alpha.any(), (pc.route_of(r, False), r, fam, status, alpha[:4])
            before = inj.retry_counter()
            alpha, status = inj.update(G, rhs, z=z, iteration=1)  # later, sampled: one retry is used up, state unchanged, status stays
            assert status == 0 and not alpha.any() and before > 0 and inj.retry_counter() == before - 1, \
                (pc.route_of(r, True), r, fam, status, before, inj.retry_counter())
            rc, lp = inj.logpdf(G, rhs, pc.qte_of(pc.stot_cached(r), qdir))
            # GINGR_ERR_NOT_SPD and no value: the code gingr_amd.api maps to -inf (logTransitionProbability)
            assert rc == inj.nat.ERR_NOT_SPD and not np.isfinite(lp), (pc.density_route_of(r, "sharded"), r, fam, rc, lp)
    finally:
        inj.close()
        print(f"\n  r = {r}: route | family | figure | MI355X | bound | float64")
        for row in rows:
            print("    %-44s %-12s %-34s %.2e  %.2e  %.2e" % row)
    assert not failures, failures


def _print_rows(title, rows):
    print(f"\n  {title}: route | case | figure | MI355X | bound | float64")
    for row in rows:
        print("    %-44s %-12s %-34s %.2e  %.2e  %.2e" % row)


@pytest.mark.parametrize("r", pc.EIG_RANKS)
def test_eigen_route(ctx, r):
    """Family 6: point-cloud ICP without landmarks, rhs injected, G the device's own S_tot / sigma^2 (the eigen kernel ignores it)."""
    failures, rows = [], []
    variants = [(True, s2) for s2 in pc.EIG_SIGMA2] + ([(False, s2) for s2 in pc.EIG_SIGMA2] if r <= pc.EIG_MAX_RANK else [])
    route = pc.route_of(r, False, eig=True)
    try:
        for orthonormal in (True, False):
            todo = [s2 for o, s2 in variants if o == orthonormal]
            if not todo:
                continue
            parts = pc.eig_model_parts(r, orthonormal)
            inj = Injector(ctx, r, parts=parts, flavour=1)
            try:
                for s2 in todo:
                    ref, f64 = pc.eig_reference(r, s2, orthonormal)
                    inj.sigma2 = s2
                    alpha, status = inj.update(None, ref["rhs"])
                    assert status == 0 and np.all(np.isfinite(alpha)), (route, r, s2, status)
                    a = pc.undo_alpha_map(alpha, ref["S"], ref["lam"], orthonormal)
                    fig = pc.figures(ref, a, None, None)
                    # what the map alone may leave in a (module docstring), carried into both figures
                    da = np.abs(np.asarray(pc.undo_alpha_map(_map_rounding_bound(r, np.asarray(ref["a"], dtype=np.float64), parts), ref["S"],
                                                             ref["lam"], orthonormal), dtype=np.float64))
                    extra = {"forward": float(np.linalg.norm(da) / np.linalg.norm(np.asarray(ref["a"], dtype=np.float64))),
                             "backward": float(np.linalg.norm(np.abs(np.asarray(ref["N"], dtype=np.float64)) @ da) /
                                               (np.linalg.norm(np.asarray(ref["N"], dtype=np.float64)) * np.linalg.norm(np.asarray(ref["a"], dtype=np.float64))
                                                + np.linalg.norm(ref["rhs"])))}
                    for k in ("forward", "backward"):
                        bound = 1000.0 * f64[k] + extra[k]
                        if k == "backward" and route == "posterior_solve_eig_kernel":
                            bound += 4.0 * np.sqrt(pc.rp_of(r)) * 2.0 ** -53  # (module docstring: normwise stable, no better)
                        rows.append((route, ("orth" if orthonormal else "full S") + f" s2={s2:g}", k, fig[k], bound, f64[k]))
                        if not fig[k] <= bound:
                            failures.append((route, r, orthonormal, s2, k, fig[k], bound))
            finally:
                inj.close()
    finally:
        _print_rows(f"r = {r}", rows)
    assert not failures, failures


@pytest.mark.parametrize("r", pc.READBACK_RANKS)
def test_real_state_readback(ctx, r):
    """Layer B: the split kernel / the wide or dense kernels (first query) and the cached kernels (second query) of the single-shard
    density, against the reference of the system the device itself built for a real CPD state."""
    ref_pts, mean, U, lam, target, mesh = pc.readback_model_parts(r)
    inj = Injector(ctx, r, parts=(ref_pts, mean, U, lam), target=target, sigma2=pc.READBACK_SIGMA2)
    rows, failures = [], []
    try:
        (G, rhs, qte), lp_shard = inj.capture(mesh)
        assert np.abs(G - G.T).max() <= 1e-12 * np.abs(G).max()
        G = 0.5 * (G + G.T)
        cond = pc.cond_of(G)
        assert r == 1 or cond >= 1e6, (r, cond)  # (a 1 x 1 matrix has condition 1)
        S = pc.stot_ld(U, lam)
        want = pc.density_only(G, rhs, S, qte, pc.LD)["logpdf"]
        got64 = pc.density_only(G, rhs, np.asarray(S, dtype=np.float64), qte, np.float64, chol=np.linalg.cholesky)["logpdf"]
        f64 = float(abs(pc.LD(got64) - want) / abs(want))
        bound = 1000.0 * f64 if f64 > 0.0 else r * 2.0 ** -53
        inj.sf.set_state(np.zeros(r), pc.READBACK_SIGMA2)  # the same state again: the single-shard routes start from its memo
        rc1, first = inj.logpdf_single_shard(mesh)
        rc2, second = inj.logpdf_single_shard(mesh)
        assert rc1 == 0 and rc2 == 0, (r, rc1, rc2)
        for route, got in ((pc.density_route_of(r, "sharded"), lp_shard), (pc.density_route_of(r, "fresh"), first),
                           (pc.density_route_of(r, "cached"), second)):
            dev = float(abs(pc.LD(got) - want) / abs(want))
            rows.append((route, "real state", "density", dev, bound, f64))
            if not dev <= bound:
                failures.append((route, r, "real state", dev, bound))
    finally:
        inj.close()
        _print_rows(f"r = {r}", rows)
    assert not failures, failures


def _triangle_strip(n):
    i = np.arange(n - 2, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], axis=1)


@pytest.mark.parametrize("r", pc.MH_RANKS)
def test_real_state_mh_step(ctx, r):
    """Layer B behind gingr_fitter_mh_step: step 1 (z1, need_forward) = the fresh sampled solve and the split density kernel with
    keep_factor; restore; step 2 (z2) = posterior_sample_cached_kernel on the factor step 1 left.  All against the reference of the
    system copied out of the device for this state."""
    nat = pc_nat()
    ref_pts, mean, U, lam, target, _ = pc.readback_model_parts(r)
    inj = Injector(ctx, r, parts=(ref_pts, mean, U, lam), target=target, sigma2=pc.READBACK_SIGMA2)
    rows, failures = [], []
    try:
        inj.sf.set_meshes(_triangle_strip(ref_pts.shape[0]), _triangle_strip(target.shape[0]))
        inj.sf.set_state(np.zeros(r), pc.READBACK_SIGMA2)
        _, _, fit = inj.sf.get_state()
        (G, rhs, qte), _ = inj.capture(fit)  # q(x'|x) projects x's own fit (fitter_mh.hip: step (4))
        G = 0.5 * (G + G.T)
        cond = pc.cond_of(G)
        assert r == 1 or cond >= 1e6, (r, cond)
        S = pc.stot_ld(U, lam)
        rng = np.random.default_rng(77 + r)
        z1, z2 = rng.normal(0, 1, r), rng.normal(0, 1, r)
        cmap = pc.alpha_map_ld(lam)
        lib, f = inj.sf._lib, inj.sf.handle
        inj.sf.set_state(np.zeros(r), pc.READBACK_SIGMA2)
        cp = nat.CpdParams(*CPD)
        req = nat.MhRequest()
        req.flavour, req.kind, req.cpd, req.eval_sdev, req.eval_points, req.need_forward = 0, 0, ctypes.pointer(cp), 5.0, 0, 1
        res, alpha = nat.MhResult(), np.empty(r)
        for step, (z, route) in enumerate(((z1, pc.route_of(r, True) + " (sampled)"), (z2, pc.route_of(r, True, factor_cached=True)))):
            zz = nat.f64(z)
            req.z = nat.dptr(zz)
            assert lib.gingr_fitter_mh_step(f, ctypes.byref(req), nat.dptr(alpha), None, ctypes.byref(res)) == 0, (r, step)
            assert res.scalars.status == 0 and np.all(np.isfinite(alpha)), (route, r, res.scalars.status)
            ref = pc.reference_on(G, rhs, z, S, qte, lam)
            f64 = pc.float64_route_on(ref, S)
            fig = pc.figures(ref, None, alpha.astype(pc.LD) / cmap, res.log_q_forward if step == 0 else None)
            assert step == 1 or res.forward_status == 0, (r, res.forward_status)
            for k, v in fig.items():
                bound = 1000.0 * f64[k] if f64[k] > 0.0 else r * 2.0 ** -53
                rt = "posterior_logpdf_split_kernel (keep_factor)" if k == "density" else route
                rows.append((rt, "real state", k, v, bound, f64[k]))
                if not v <= bound:
                    failures.append((rt, r, "real state", k, v, bound))
            if step == 0:
                assert lib.gingr_fitter_mh_restore(f) == 0
                req.need_forward = 0  # (the host holds q(.|x) now, as a chain does)
    finally:
        inj.close()
        _print_rows(f"r = {r}", rows)
    assert not failures, failures


def pc_nat():
    from gingr_amd import _native as nat
    return nat
