// Scalar mathematics of the Bayesian coherent point drift (bcpd.hip) as plain C++: the digamma function of the <alpha_m> update, the
// similarity transform from the singular vectors of S_xu, and the planner of the two pair passes.  Compiled for the device by
// bcpd.hip and for the host alone by the CPU tests (tests/test_bcpd_host.py, tests/c/bcpd_math_driver.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "host_device.h"

// psi(x) for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to an argument >= 6, then the asymptotic series
//   psi(x) ~ ln x - 1 / (2 x) - sum_k B_2k / (2 k x^2k),  k = 1 .. 10
// (first omitted term: B_22 / (22 x^22) < 2.2e-15 at x = 6).  The reciprocals of the recurrence are summed from the smallest up and
// subtracted last, so that near the root (1.4616...) the error is that of one subtraction of two numbers near 1.8.
GINGR_HD inline double bcpd_digamma(double x) {
    if (!(x > 0.0)) return NAN;
    if (x > kDblMax) return x;
    double rec[6];
    int n = 0;
    while (x < 6.0) {
        rec[n++] = 1.0 / x;
        x += 1.0;
    }
    double shift = 0.0;
    for (int k = n - 1; k >= 0; --k) shift += rec[k];
    const double r = 1.0 / x, r2 = r * r;
    // B_2k / (2 k): 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12, -3617/8160, 43867/14364, -174611/6600
    double p = -174611.0 / 6600.0;
    p = fma(p, r2, 43867.0 / 14364.0);
    p = fma(p, r2, -3617.0 / 8160.0);
    p = fma(p, r2, 1.0 / 12.0);
    p = fma(p, r2, -691.0 / 32760.0);
    p = fma(p, r2, 1.0 / 132.0);
    p = fma(p, r2, -1.0 / 240.0);
    p = fma(p, r2, 1.0 / 252.0);
    p = fma(p, r2, -1.0 / 120.0);
    p = fma(p, r2, 1.0 / 12.0);
    const double tail = fma(p, r2, 0.5 * r);  // 1 / (2 x) + sum_k
    return (log(x) - tail) - shift;
}

// <alpha_m> = exp(psi(kappa + nu_m) - psi(kappa M + N^)); kappa = +inf: 1 / M (the Dirichlet prior pins the mixing weights)
GINGR_HD inline double bcpd_alpha(double kappa, double nu, double psi_total, double M) {
    if (kappa > kDblMax) return 1.0 / M;
    return exp(bcpd_digamma(kappa + nu) - psi_total);
}

// The similarity step from the singular vectors of S_xu = Phi diag(.) Psi^T (all 3 x 3 row-major; the columns of Phi and Psi):
//   R = Phi diag(1, 1, det(Phi Psi^T)) Psi^T,  s = tr(R^T S_xu) / tr(S_uu),  t = xbar - s R ubar
// The sign of a singular vector pair does not matter, and neither does the choice of the last column of Phi for a rank-2 S_xu: a flip
// changes the determinant with it.  out13 = {s, R row-major, t}.
GINGR_HD inline void bcpd_similarity_finish(const double Sxu[9], const double Phi[9], const double Psi[9], double tr_Suu, const double xbar[3],
                                            const double ubar[3], double out13[13]) {
    double W[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) W[a * 3 + b] = Phi[a * 3] * Psi[b * 3] + Phi[a * 3 + 1] * Psi[b * 3 + 1] + Phi[a * 3 + 2] * Psi[b * 3 + 2];
    const double d = det3(W) < 0.0 ? -1.0 : 1.0;
    double *R = out13 + 1, tr = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            R[a * 3 + b] = Phi[a * 3] * Psi[b * 3] + Phi[a * 3 + 1] * Psi[b * 3 + 1] + d * Phi[a * 3 + 2] * Psi[b * 3 + 2];
            tr += R[a * 3 + b] * Sxu[a * 3 + b];
        }
    const double s = tr / tr_Suu;
    out13[0] = s;
    for (int a = 0; a < 3; ++a) out13[10 + a] = xbar[a] - s * (R[a * 3] * ubar[0] + R[a * 3 + 1] * ubar[1] + R[a * 3 + 2] * ubar[2]);
}

// Chunks of the streamed cloud of a pair pass: `owners` points have one thread each (256 to a workgroup), the `streamed` points are
// split into chunks of whole 256-point tiles, one partial per chunk, enough of them for about kBcpdTargetGroups workgroups.
constexpr int64_t kBcpdTile = 256;
constexpr int64_t kBcpdTargetGroups = 1024;
constexpr int64_t kBcpdMaxChunks = 256;
struct BcpdChunks {
    int64_t count, length;  // length: a multiple of kBcpdTile; count * length >= streamed
};
inline BcpdChunks bcpd_plan_chunks(int64_t owners, int64_t streamed) {
    const int64_t groups = ceil_div(owners, kBcpdTile), tiles = ceil_div(streamed, kBcpdTile);
    int64_t want = ceil_div(kBcpdTargetGroups, groups);
    if (want > tiles) want = tiles;
    if (want > kBcpdMaxChunks) want = kBcpdMaxChunks;
    if (want < 1) want = 1;
    const int64_t length = ceil_div(tiles, want) * kBcpdTile;
    return BcpdChunks{ceil_div(streamed, length), length};
}
