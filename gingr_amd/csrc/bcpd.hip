// Bayesian coherent point drift (Hirose 2020, Fig. 4) on the device -- the method of the reference's draft other/algorithms/cpd/BCPD.scala,
// in this package's definition (DESIGN.md section 5 lists where it follows the paper against the draft).  One iteration from the state
// (y^, sigma_m^2, s, R, t, sigma2, <alpha_m>), template y (M x 3), target x (N x 3), G = (g(y_m, y_m')) fixed:
//
//   1  a_m = (1 - w) <alpha_m> exp(-1.5 s^2 sigma_m^2 / sigma2),  e_mn = exp(-|x_n - y^_m|^2 / 2 sigma2),  c = w p_out (2 pi sigma2)^1.5
//      den_n = sum_m a_m e_mn,  p_mn = a_m e_mn / (den_n + c);  P is never formed: nu = P 1, nu' = P^T 1, P x, xPx           [two pair passes]
//   2  c2 = s^2 / sigma2, K = G / lambda, D = c2 diag nu, r_m = (1 / s) R^T (PX_m - nu_m t) - nu_m y_m
//      A = I + D^1/2 K D^1/2 = L L^T (dense_spd.hip; the identity rides along and comes back as L^-T)
//      z = K r,  q = A^-1 D^1/2 z = L^-T (L^-1 D^1/2 z),  v^ = c2 (z - K D^1/2 q),  sigma_m^2 = K_mm - |L^-1 D^1/2 k_m|^2  (MFMA),  u^ = y + v^
//      <alpha_m> = exp(psi(kappa + nu_m) - psi(kappa M + N^))
//   3  xbar, ubar, sbar2 (nu-weighted), S_xu, tr S_uu, R = Phi diag(1, 1, det(Phi Psi^T)) Psi^T, s = tr(R^T S_xu) / tr S_uu, t = xbar - s R ubar
//   4  y^ = s R u^ + t,  sigma2 = (xPx - 2 sum PX_m . y^_m + sum nu_m |y^_m|^2) / (3 N^) + s^2 sbar2
//
// Nothing divides by nu_m: a row with nu_m = 0 (a template point without counterpart) is an ordinary row.  Every reduction adds its
// partials in a fixed order: two runs give the same bits.
//
// A handle of gingr_bcpd_create_lowrank holds a factor L (G ~ L L^T) in place of G and runs step 2 over it (bcpd_lowrank.hip); steps 1,
// 3 and 4 and every M- and N-sized buffer are the same.
#include "common.h"
#include "bcpd_lowrank.h"
#include "bcpd_math.h"
#include "cloud_sums.h"
#include "dense_spd.h"
#include "fastexp.h"
#include "kernel_warp.h"
#include "svd3.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

namespace {

constexpr int kNBc = DenseSpdWork::kBlock;
constexpr int kRedBlocks = 64;  // workgroups of the O(M + N) reductions
constexpr int kTile = (int)kBcpdTile;

typedef double bcpd_v4f64 __attribute__((ext_vector_type(4)));

Cloud cloud_at(const double *soa, int64_t n) { return Cloud{soa, soa + n, soa + 2 * n, n}; }

// device scalars: sc[0] sigma2, [1] N^, [2] sbar2, [3] xPx, [5] the c2 = s^2 / sigma2 that went into the last iteration;  params: s, R row-major, t;  mu: xbar, ubar, [6] psi(kappa M + N^)

// a_m = (1 - w) <alpha_m> exp(-1.5 s^2 sigma_m^2 / sigma2)
__global__ __launch_bounds__(256) void bcpd_weights_kernel(int64_t M, double w, const double *__restrict__ alpha, const double *__restrict__ sig,
                                                           const double *__restrict__ params, const double *__restrict__ sc,
                                                           double *__restrict__ a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const double s = params[0];
    a[m] = (1.0 - w) * alpha[m] * exp(-1.5 * (s * s) * sig[m] / sc[0]);
}

// ---------------------------------------------------------------------------------------------------- the two pair passes
// Both: one thread per owned point, the streamed cloud staged in LDS as 256 records of four doubles (a record is read by every lane
// of a wave at once: two 16-byte broadcasts), the exponential from the 2048-entry table in its round-to-nearest form (fastexp.h,
// degree 3: one ulp of its argument), the argument clamped where the clouds' extent could push it out of the table's range.
// grid (owner tiles, chunks of the streamed cloud); one partial per chunk, added up in chunk order by the kernel that follows.
struct PairScale {
    double c, lim;
    bool clamp;
};
__device__ __forceinline__ PairScale pair_scale(const double *__restrict__ sc, const double *__restrict__ aux) {
    PairScale p;
    p.c = fastexp_scale_for_variance<11>(2.0 * sc[0]);
    const double am = aux[0] + aux[1];  // 3 am^2 bounds every squared distance between the two clouds
    p.clamp = fastexp_needs_clamp(3.0 * am * am, p.c);  // wave-uniform
    p.lim = fastexp_d2_limit<11>(p.c);
    return p;
}

// column pass: part[chunk][n] = sum over the chunk's rows of a_m e_mn
__global__ __launch_bounds__(256) void bcpd_colsum_kernel(Cloud X, Cloud Yh, const double *__restrict__ a, const double *__restrict__ sc,
                                                          const double *__restrict__ aux, int64_t chunk_len, double *__restrict__ part) {
    __shared__ double T[GINGR_EXP_TABLE];
    __shared__ double rec[kTile * 4] __attribute__((aligned(16)));
    fastexp_table_init(T);
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * kTile + tid, no = n < X.n ? n : X.n - 1;  // (a thread past the end computes a copy of the last point)
    const double px = X.x[no], py = X.y[no], pz = X.z[no];
    const PairScale ps = pair_scale(sc, aux);
    const int64_t m0 = (int64_t)blockIdx.y * chunk_len, m1 = m0 + chunk_len < Yh.n ? m0 + chunk_len : Yh.n;
    double acc = 0.0;
    for (int64_t mb = m0; mb < m1; mb += kTile) {
        __syncthreads();  // the previous tile has been consumed (first round: nothing to wait for but the table)
        const int64_t m = mb + tid;
        const bool in = m < m1;
        rec[4 * tid] = in ? Yh.x[m] : 0.0;
        rec[4 * tid + 1] = in ? Yh.y[m] : 0.0;
        rec[4 * tid + 2] = in ? Yh.z[m] : 0.0;
        rec[4 * tid + 3] = in ? a[m] : 0.0;
        __syncthreads();
        const int cnt = (int)(m1 - mb < kTile ? m1 - mb : kTile);  // records past the end are never evaluated
        if (ps.clamp) {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double dx = px - rec[4 * k], dy = py - rec[4 * k + 1], dz = pz - rec[4 * k + 2];
                const double d2 = fastexp_clamp_d2(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)), ps.lim);
                acc = __builtin_fma(rec[4 * k + 3], fastexp2_scaled<3>(d2, ps.c, T), acc);
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double dx = px - rec[4 * k], dy = py - rec[4 * k + 1], dz = pz - rec[4 * k + 2];
                const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
                acc = __builtin_fma(rec[4 * k + 3], fastexp2_scaled<3>(d2, ps.c, T), acc);
            }
        }
    }
    if (n < X.n) part[(int64_t)blockIdx.y * X.n + n] = acc;
}

// den_n = sum of the chunk partials; inv_n = 1 / (den_n + c), nu'_n = den_n inv_n, xpart[block] = sum nu'_n |x_n|^2;
// a non-finite 1 / (den_n + c) raises the flag
__global__ __launch_bounds__(256) void bcpd_den_finalize_kernel(Cloud X, const double *__restrict__ part, int chunks, double w, double p_out,
                                                                const double *__restrict__ sc, double *__restrict__ inv,
                                                                double *__restrict__ nup, double *__restrict__ xpart,
                                                                int32_t *__restrict__ flag) {
    __shared__ double sh[256];
    const double t2 = 2.0 * 3.14159265358979323846 * sc[0];
    const double c = w > 0.0 ? w * p_out * (t2 * sqrt(t2)) : 0.0;
    double acc = 0.0;
    bool bad = false;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < X.n; n += (int64_t)kRedBlocks * 256) {
        double den = 0.0;
        for (int ch = 0; ch < chunks; ++ch) den += part[(int64_t)ch * X.n + n];
        const double iv = 1.0 / (den + c), p = den * iv;
        bad = bad || !finite_d(iv);
        inv[n] = iv;
        nup[n] = p;
        const double x = X.x[n], y = X.y[n], z = X.z[n];
        acc += p * ((x * x + y * y) + z * z);
    }
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) xpart[blockIdx.x] = t;
    if (bad) *flag = GINGR_ERR_NONFINITE;  // (every writer stores the same value)
}

// row pass: part[chunk][q][m], q = 0: a_m sum_n e_mn inv_n (nu_m), q = 1..3: a_m sum_n e_mn inv_n x_n (PX_m), over the chunk's target points
__global__ __launch_bounds__(256) void bcpd_rowstats_kernel(Cloud Yh, Cloud X, const double *__restrict__ a, const double *__restrict__ inv,
                                                            const double *__restrict__ sc, const double *__restrict__ aux, int64_t chunk_len,
                                                            double *__restrict__ part) {
    __shared__ double T[GINGR_EXP_TABLE];
    __shared__ double rec[kTile * 4] __attribute__((aligned(16)));
    fastexp_table_init(T);
    const int tid = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * kTile + tid, mo = m < Yh.n ? m : Yh.n - 1;
    const double px = Yh.x[mo], py = Yh.y[mo], pz = Yh.z[mo];
    const PairScale ps = pair_scale(sc, aux);
    const int64_t n0 = (int64_t)blockIdx.y * chunk_len, n1 = n0 + chunk_len < X.n ? n0 + chunk_len : X.n;
    double s0 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t nb = n0; nb < n1; nb += kTile) {
        __syncthreads();
        const int64_t n = nb + tid;
        const bool in = n < n1;
        rec[4 * tid] = in ? X.x[n] : 0.0;
        rec[4 * tid + 1] = in ? X.y[n] : 0.0;
        rec[4 * tid + 2] = in ? X.z[n] : 0.0;
        rec[4 * tid + 3] = in ? inv[n] : 0.0;
        __syncthreads();
        const int cnt = (int)(n1 - nb < kTile ? n1 - nb : kTile);
        if (ps.clamp) {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double qx = rec[4 * k], qy = rec[4 * k + 1], qz = rec[4 * k + 2];
                const double dx = qx - px, dy = qy - py, dz = qz - pz;
                const double d2 = fastexp_clamp_d2(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)), ps.lim);
                const double t = fastexp2_scaled<3>(d2, ps.c, T) * rec[4 * k + 3];
                s0 += t;
                sx = __builtin_fma(t, qx, sx);
                sy = __builtin_fma(t, qy, sy);
                sz = __builtin_fma(t, qz, sz);
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double qx = rec[4 * k], qy = rec[4 * k + 1], qz = rec[4 * k + 2];
                const double dx = qx - px, dy = qy - py, dz = qz - pz;
                const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
                const double t = fastexp2_scaled<3>(d2, ps.c, T) * rec[4 * k + 3];
                s0 += t;
                sx = __builtin_fma(t, qx, sx);
                sy = __builtin_fma(t, qy, sy);
                sz = __builtin_fma(t, qz, sz);
            }
        }
    }
    if (m < Yh.n) {
        const double am = a[m];
        double *p = part + (int64_t)blockIdx.y * 4 * Yh.n + m;
        p[0] = am * s0;
        p[Yh.n] = am * sx;
        p[2 * Yh.n] = am * sy;
        p[3 * Yh.n] = am * sz;
    }
}

// nu_m, PX_m from the chunk partials; r_m = (1 / s) R^T (PX_m - nu_m t) - nu_m y_m; dh_m = (c2 nu_m)^1/2; *c2_keep = c2 (the end of the
// iteration overwrites s and sigma2: the coefficients of the kernel warp need the c2 that went in)
__global__ __launch_bounds__(256) void bcpd_rows_finish_kernel(int64_t M, const double *__restrict__ part, int chunks, const double *__restrict__ y,
                                                               const double *__restrict__ params, const double *__restrict__ sc,
                                                               double *__restrict__ nu, double *__restrict__ PX, double *__restrict__ r,
                                                               double *__restrict__ dh, double *c2_keep) {  // (c2_keep points into sc's buffer)
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    if (m == 0) *c2_keep = params[0] * params[0] / sc[0];
    double v[4] = {0, 0, 0, 0};
    for (int ch = 0; ch < chunks; ++ch)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += part[((int64_t)ch * 4 + q) * M + m];
    const double s = params[0], *R = params + 1, *t = params + 10;
    nu[m] = v[0];
    const double e[3] = {v[1] - v[0] * t[0], v[2] - v[0] * t[1], v[3] - v[0] * t[2]};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        PX[d * M + m] = v[1 + d];
        r[d * M + m] = ((e[0] * R[d] + e[1] * R[3 + d]) + e[2] * R[6 + d]) / s - v[0] * y[d * M + m];
    }
    dh[m] = sqrt(s * s / sc[0] * v[0]);
}

// ---------------------------------------------------------------------------------------------------- the deformation
// z = K r (K = G / lambda) and the right-hand sides b = D^1/2 z (planes of stride Mp): 16 lanes per row of G
__global__ __launch_bounds__(256) void bcpd_kr_kernel(int64_t M, int64_t Mp, const double *__restrict__ G, double lambda,
                                                      const double *__restrict__ r, const double *__restrict__ dh, double *__restrict__ z,
                                                      double *__restrict__ b) {
    const int lane16 = threadIdx.x & 15;
    const int64_t m = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    double a[3];
    row_dot3(G + m * M, 0, m < M ? M : 0, lane16, r, M, nullptr, a);
    if (m < M && lane16 == 0)
        for (int d = 0; d < 3; ++d) {
            const double v = a[d] / lambda;
            z[d * M + m] = v;
            b[d * Mp + m] = dh[m] * v;
        }
}

// v^ = c2 (z - K D^1/2 q), u^ = y + v^
__global__ __launch_bounds__(256) void bcpd_deform_kernel(int64_t M, int64_t Mp, const double *__restrict__ G, double lambda,
                                                          const double *__restrict__ q, const double *__restrict__ dh,
                                                          const double *__restrict__ z, const double *__restrict__ y,
                                                          const double *__restrict__ params, const double *__restrict__ sc,
                                                          double *__restrict__ vhat, double *__restrict__ u) {
    const int lane16 = threadIdx.x & 15;
    const int64_t m = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    double a[3];
    row_dot3(G + m * M, 0, m < M ? M : 0, lane16, q, Mp, dh, a);
    if (m < M && lane16 == 0) {
        const double c2 = params[0] * params[0] / sc[0];
        for (int d = 0; d < 3; ++d) {
            const double v = c2 * (z[d * M + m] - a[d] / lambda);
            vhat[d * M + m] = v;
            u[d * M + m] = y[d * M + m] + v;
        }
    }
}

// The coefficients of the kernel warp: c = (c2 / lambda) (r - nu o v^), so that v^ = G c (Sigma^-1 v^ = c2 r with
// Sigma^-1 = lambda G^-1 + c2 diag nu; L L^T in place of G on the low-rank route) -- no inverse of G, no division by nu_m
__global__ __launch_bounds__(256) void bcpd_coefficients_kernel(int64_t M, double lambda, const double *__restrict__ sc,
                                                                const double *__restrict__ r, const double *__restrict__ nu,
                                                                const double *__restrict__ vhat, double *__restrict__ c) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const double f = sc[5] / lambda, p = nu[m];
    for (int d = 0; d < 3; ++d) c[d * M + m] = f * (r[d * M + m] - p * vhat[d * M + m]);
}

struct BcpdSystemElem {  // I + D^1/2 K D^1/2
    const double *__restrict__ G;
    const double *__restrict__ dh;
    int64_t M;
    double lambda;
    __device__ double operator()(int64_t row, int64_t c) const { return dh[row] * (G[row * M + c] / lambda) * dh[c] + (row == c ? 1.0 : 0.0); }
};

// With X = L^-T (upper triangular, row stride Mp; rows and columns past M: the identity):  w = X^T b = L^-1 b.  32 columns to a workgroup
// (the loads of half a wave are one 256-byte row segment of X), the rows dealt to eight groups of threads (row i to group i & 7) whose
// partial sums are added in group order ...
__global__ __launch_bounds__(256) void bcpd_forward_kernel(int64_t Mp, const double *__restrict__ X, const double *__restrict__ b,
                                                           double *__restrict__ wv) {
    __shared__ double sh[3][8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int64_t j = (int64_t)blockIdx.x * 32 + c;  // < Mp: a multiple of 64
    double a[3] = {0, 0, 0};
#pragma unroll 4
    for (int64_t i = g; i <= j; i += 8) {
        const double x = X[i * Mp + j];
        a[0] = __builtin_fma(x, b[i], a[0]);
        a[1] = __builtin_fma(x, b[Mp + i], a[1]);
        a[2] = __builtin_fma(x, b[2 * Mp + i], a[2]);
    }
    for (int d = 0; d < 3; ++d) sh[d][g][c] = a[d];
    __syncthreads();
    if (g < 3) {
        double v = sh[g][0][c];
        for (int q = 1; q < 8; ++q) v += sh[g][q][c];
        wv[g * Mp + j] = v;
    }
}
// ... and q = X w = A^-1 b, 16 lanes per row
__global__ __launch_bounds__(256) void bcpd_backward_kernel(int64_t Mp, const double *__restrict__ X, const double *__restrict__ wv,
                                                            double *__restrict__ q) {
    const int lane16 = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    double a[3];
    row_dot3(X + i * Mp, i, i < Mp ? Mp : 0, lane16, wv, Mp, nullptr, a);  // (X is upper triangular: from the diagonal on)
    if (i < Mp && lane16 == 0)
        for (int d = 0; d < 3; ++d) q[d * Mp + i] = a[d];
}

// The M x M x M product of the iteration on the matrix pipe: the 64 x 64 tile (jb, mb) of W = X^T (D^1/2 K) = L^-1 D^1/2 K,
//   W[j][m] = sum_{i <= j} X[i][j] dh_i K[i][m],
// summed over the row blocks ib <= jb (X is upper triangular), never stored: part[jb][m] = sum_{j in block jb} W[j][m]^2.
// Both operands are k-major ([i][j], [i][m]), staged through LDS 32 rows of k at a time (row stride 80 doubles: the four k of a
// fragment read land in different banks).  Fragment layout of v_mfma_f64_16x16x4: lane l supplies A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15] and holds D[i = (l >> 4) + 4 reg][j = l & 15]; wave w owns the rows j = 16 w .. 16 w + 15 of the tile.
__global__ __launch_bounds__(256) void bcpd_sigma_tiles_kernel(const double *__restrict__ X, int64_t Mp, const double *__restrict__ G, int64_t M,
                                                               const double *__restrict__ dh, double lambda, double *__restrict__ part) {
    constexpr int kLd = 80;
    __shared__ double As[32 * kLd], Bs[32 * kLd];
    __shared__ double red[4][kNBc];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int mb = blockIdx.x, jb = blockIdx.y;
    bcpd_v4f64 acc[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = bcpd_v4f64{0.0, 0.0, 0.0, 0.0};
    for (int ib = 0; ib <= jb; ++ib)
        for (int half = 0; half < 2; ++half) {
            __syncthreads();
            double va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = tid + 256 * u, k = e >> 6, c = e & 63;
                const int64_t i = (int64_t)ib * kNBc + 32 * half + k, col = (int64_t)mb * kNBc + c;
                va[u] = X[i * Mp + (int64_t)jb * kNBc + c];
                vb[u] = (i < M && col < M) ? dh[i] * (G[i * M + col] / lambda) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = tid + 256 * u, k = e >> 6, c = e & 63;
                As[k * kLd + c] = va[u];
                Bs[k * kLd + c] = vb[u];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const double a = As[(4 * q + l4) * kLd + 16 * wave + l15];
#pragma unroll
                for (int tj = 0; tj < 4; ++tj)
                    acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(4 * q + l4) * kLd + 16 * tj + l15], acc[tj], 0, 0, 0);
            }
        }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) s = __builtin_fma(acc[tj][g], acc[tj][g], s);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (l4 == 0) red[wave][16 * tj + l15] = s;
    }
    __syncthreads();
    if (tid < kNBc) part[(int64_t)jb * Mp + (int64_t)mb * kNBc + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// sigma_m^2 = K_mm - sum over the row blocks of W's column sums of squares
__global__ __launch_bounds__(256) void bcpd_sigma_finish_kernel(int64_t M, int64_t Mp, const double *__restrict__ G, double lambda,
                                                                const double *__restrict__ part, int nb, double *__restrict__ sig) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double s = 0.0;
    for (int jb = 0; jb < nb; ++jb) s += part[(int64_t)jb * Mp + m];
    sig[m] = G[m * M + m] / lambda - s;
}

// ---------------------------------------------------------------------------------------------------- similarity, shape, variance
// partial[b][0] = sum nu, [1..3] sum PX, [4..6] sum nu u^, [7] sum nu sigma_m^2
__global__ __launch_bounds__(256) void bcpd_sums_a_kernel(int64_t M, const double *__restrict__ nu, const double *__restrict__ PX,
                                                          const double *__restrict__ u, const double *__restrict__ sig,
                                                          double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)kRedBlocks * 256) {
        const double p = nu[m];
        a[0] += p;
        for (int d = 0; d < 3; ++d) {
            a[1 + d] += PX[d * M + m];
            a[4 + d] += p * u[d * M + m];
        }
        a[7] += p * sig[m];
    }
    block_sums<8>(a, sh, partial + blockIdx.x * 8);
}

// sc[1] = N^, sc[2] = sbar2, sc[3] = xPx; mu[0..2] = xbar, mu[3..5] = ubar, mu[6] = psi(kappa M + N^)
__global__ void bcpd_means_finish_kernel(int64_t M, double kappa, const double *__restrict__ partial, const double *__restrict__ xpart,
                                         double *__restrict__ sc, double *__restrict__ mu) {
    if (threadIdx.x != 0) return;
    double v[8];
    for (int q = 0; q < 8; ++q) v[q] = sum_partials(partial, kRedBlocks, 8, q);
    const double Nh = v[0];
    sc[1] = Nh;
    sc[2] = v[7] / Nh;
    sc[3] = sum_partials(xpart, kRedBlocks, 1, 0);
    for (int d = 0; d < 6; ++d) mu[d] = v[1 + d] / Nh;
    mu[6] = kappa > kDblMax ? 0.0 : bcpd_digamma(kappa * (double)M + Nh);
}

__global__ __launch_bounds__(256) void bcpd_alpha_kernel(int64_t M, double kappa, const double *__restrict__ nu, const double *__restrict__ mu,
                                                         double *__restrict__ alpha) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < M) alpha[m] = bcpd_alpha(kappa, nu[m], mu[6], (double)M);
}

// partial[b][0..8] = sum (PX_m - nu_m xbar)(u^_m - ubar)^T (row-major), [9] = sum nu_m |u^_m - ubar|^2
__global__ __launch_bounds__(256) void bcpd_sums_b_kernel(int64_t M, const double *__restrict__ nu, const double *__restrict__ PX,
                                                          const double *__restrict__ u, const double *__restrict__ mu,
                                                          double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[10];
    for (int q = 0; q < 10; ++q) a[q] = 0.0;
    const double xb[3] = {mu[0], mu[1], mu[2]}, ub[3] = {mu[3], mu[4], mu[5]};
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)kRedBlocks * 256) {
        const double p = nu[m];
        const double e[3] = {PX[m] - p * xb[0], PX[M + m] - p * xb[1], PX[2 * M + m] - p * xb[2]};
        const double uc[3] = {u[m] - ub[0], u[M + m] - ub[1], u[2 * M + m] - ub[2]};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) a[r * 3 + c] += e[r] * uc[c];
        a[9] += p * ((uc[0] * uc[0] + uc[1] * uc[1]) + uc[2] * uc[2]);
    }
    block_sums<10>(a, sh, partial + blockIdx.x * 10);
}

// one thread of 3 x 3 algebra: S_xu, tr S_uu, the singular vectors (svd3.h), then (s, R, t) (bcpd_math.h)
__global__ void bcpd_similarity_kernel(const double *__restrict__ partial, const double *__restrict__ sc, const double *__restrict__ mu,
                                       double *__restrict__ params) {
    if (threadIdx.x != 0) return;
    double v[10];
    for (int q = 0; q < 10; ++q) v[q] = sum_partials(partial, kRedBlocks, 10, q) / sc[1];
    const double tr_suu = v[9] + 3.0 * sc[2];
    double Phi[9], S[3], Psi[9], out[13];
    svd3(v, Phi, S, Psi);
    bcpd_similarity_finish(v, Phi, Psi, tr_suu, mu, mu + 3, out);
    for (int q = 0; q < 13; ++q) params[q] = out[q];
}

// y^ = s R u^ + t; partial[b][0] = sum PX_m . y^_m, [1] = sum nu_m |y^_m|^2
__global__ __launch_bounds__(256) void bcpd_shape_kernel(int64_t M, const double *__restrict__ u, const double *__restrict__ params,
                                                         const double *__restrict__ nu, const double *__restrict__ PX, double *__restrict__ yh,
                                                         double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[2] = {0, 0};
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)kRedBlocks * 256) {
        double p[3];
        similarity_apply(params, u[m], u[M + m], u[2 * M + m], p);
        for (int d = 0; d < 3; ++d) yh[d * M + m] = p[d];
        a[0] += (PX[m] * p[0] + PX[M + m] * p[1]) + PX[2 * M + m] * p[2];
        a[1] += nu[m] * ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    }
    block_sums<2>(a, sh, partial + blockIdx.x * 2);
}

// sigma2 = (xPx - 2 sum PX . y^ + sum nu |y^|^2) / (3 N^) + s^2 sbar2; flags[1] (sticky until the host reads it: the first failure is
// the one reported) takes the failure of a diagonal block of A (flags[0], which the next iteration's system kernel clears) and a
// non-finite result
__global__ void bcpd_variance_kernel(const double *__restrict__ partial, const double *__restrict__ params, double *__restrict__ sc,
                                     int32_t *__restrict__ flags) {
    if (threadIdx.x != 0) return;
    const double pxy = sum_partials(partial, kRedBlocks, 2, 0), ypy = sum_partials(partial, kRedBlocks, 2, 1), s = params[0];
    const double ns = (sc[3] - 2.0 * pxy + ypy) / (sc[1] * 3.0) + s * s * sc[2];
    sc[0] = ns;
    if (flags[1]) return;  // (a non-finite 1 / (den_n + c) came first: the system it poisons fails its factorisation as well)
    if (flags[0])
        flags[1] = flags[0];
    else if (!finite_d(ns) || !finite_d(s))
        flags[1] = GINGR_ERR_NONFINITE;
}

}  // namespace

struct gingr_bcpd {
    gingr_ctx *ctx = nullptr;
    int64_t M = 0, N = 0, Mp = 0;
    double w = 0.0, lambda = 2.0, gamma = 1.0, kappa = 1.0, beta = 2.0, p_out = 0.0, sigma2_init = 0.0;
    BcpdChunks col{1, kBcpdTile}, row{1, kBcpdTile};
    DevBuf X, Y, Yh, V, U, PX, Rr, Z, B, Wv, Q, sig, alpha, a, nu, dh, nup, inv, ws, xpart, red, mu, params, sc, aux, flags, G, Aw, Linv, stage;
    std::unique_ptr<BcpdLowRank> lowrank;  // gingr_bcpd_create_lowrank: G, Aw, Linv, B and Q stay empty, Z stays zero
    // the kernel warp (gingr_bcpd_transform_points): the map belongs to the last successful iteration; C, its coefficients, is formed on
    // the first query after it
    bool map_valid = false, coeff_ready = false;
    DevBuf C;
    KernelWarpWork warp;
};

// what gingr_bcpd_create_lowrank adds to the arguments of gingr_bcpd_create
struct BcpdLowRankRequest {
    double relative_tolerance;
    int32_t max_columns;
    gingr_classic_cpd_lowrank_info *info;
};

extern "C" {

void gingr_bcpd_destroy(gingr_bcpd *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    delete h;
}

}  // extern "C"

static int bcpd_create_impl(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, double w, double lambda,
                            double gamma, double kappa, double beta, const BcpdLowRankRequest *lowrank, gingr_bcpd **out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!out || !moving_xyz || !target_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: null argument");
    if (M < 1 || N < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: need M >= 1 and N >= 1");
    if (!(w >= 0.0 && w < 1.0)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: need 0 <= w < 1");
    if (!(lambda > 0.0) || !(gamma > 0.0) || !(kappa > 0.0) || !(beta > 0.0) || !(lambda <= kDblMax) || !(gamma <= kDblMax) || !(beta <= kDblMax))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: need lambda, gamma, kappa, beta > 0 (kappa alone may be +inf)");
    if (!lowrank && M > 32768)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: template too large (M <= 32768: the iteration keeps M x M double buffers)");
    double p_out = 0.0;
    if (w > 0.0) {  // the outlier density 1 / V, V the volume of the target's bounding box
        double lo[3], hi[3];
        for (int d = 0; d < 3; ++d) lo[d] = hi[d] = target_xyz[d];
        for (int64_t n = 1; n < N; ++n)
            for (int d = 0; d < 3; ++d) {
                lo[d] = std::min(lo[d], target_xyz[3 * n + d]);
                hi[d] = std::max(hi[d], target_xyz[3 * n + d]);
            }
        const double vol = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
        if (!(vol > 0.0) || !(vol <= kDblMax))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create: w > 0 needs a target whose bounding box has a volume");
        p_out = 1.0 / vol;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gingr_bcpd *h = new gingr_bcpd;
    h->ctx = ctx;
    h->M = M;
    h->N = N;
    h->Mp = round_up(M, kNBc);
    h->w = w;
    h->lambda = lambda;
    h->gamma = gamma;
    h->kappa = kappa;
    h->beta = beta;
    h->p_out = p_out;
    h->col = bcpd_plan_chunks(N, M);
    h->row = bcpd_plan_chunks(M, N);
    auto fail = [&](int rc) {
        gingr_bcpd_destroy(h);
        return rc;
    };
    const int64_t Mp = h->Mp, big = M > N ? M : N, nb = Mp / kNBc;
    const DenseSpdWork sys(Mp, DenseSpdWork::kIdentity);
    HANDLE_TRY(ctx, fail, h->X.alloc((size_t)3 * N * sizeof(double)));
    for (DevBuf *b : {&h->Y, &h->Yh, &h->V, &h->U, &h->PX, &h->Rr, &h->Z}) HANDLE_TRY(ctx, fail, b->alloc((size_t)3 * M * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->Wv.alloc((size_t)3 * Mp * sizeof(double)));
    if (!lowrank)
        for (DevBuf *b : {&h->B, &h->Q}) HANDLE_TRY(ctx, fail, b->alloc((size_t)3 * Mp * sizeof(double)));
    for (DevBuf *b : {&h->sig, &h->alpha, &h->a, &h->nu}) HANDLE_TRY(ctx, fail, b->alloc((size_t)M * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->dh.alloc((size_t)Mp * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->nup.alloc((size_t)N * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->inv.alloc((size_t)N * sizeof(double)));
    const int64_t ws = std::max(std::max(h->col.count * N, h->row.count * 4 * M), std::max(lowrank ? 0 : nb * Mp, sumsq_pairs_ws_doubles(M)));
    HANDLE_TRY(ctx, fail, h->ws.alloc((size_t)ws * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->stage.alloc((size_t)3 * big * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->xpart.alloc(kRedBlocks * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->red.alloc((size_t)kRedBlocks * 10 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->mu.alloc(8 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->params.alloc(16 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->sc.alloc(8 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->aux.alloc(GINGR_AUX * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->flags.alloc(2 * sizeof(int32_t)));
    if (!lowrank) {
        HANDLE_TRY(ctx, fail, h->G.alloc((size_t)M * M * sizeof(double)));
        HANDLE_TRY(ctx, fail, h->Aw.alloc((size_t)sys.aw_doubles() * sizeof(double)));
        HANDLE_TRY(ctx, fail, h->Linv.alloc((size_t)sys.linv_doubles() * sizeof(double)));
    }
    for (DevBuf *b : {&h->B, &h->Wv, &h->Q, &h->dh, &h->V, &h->nu, &h->nup, &h->sc, &h->mu, &h->aux, &h->flags})
        if (b->p) HANDLE_TRY(ctx, fail, hipMemsetAsync(b->p, 0, b->bytes, ctx->stream));  // (the padding of the Mp-long vectors stays zero)
    if (lowrank) HANDLE_TRY(ctx, fail, hipMemsetAsync(h->Z.p, 0, h->Z.bytes, ctx->stream));  // the zero `ty` of the Gram pass
    if (int rc = upload_cloud(ctx, h->stage.as<double>(), target_xyz, N, h->X.as<double>())) return fail(rc);
    if (int rc = upload_cloud(ctx, h->stage.as<double>(), moving_xyz, M, h->Y.as<double>())) return fail(rc);
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->Yh.p, h->Y.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    const Cloud X = cloud_at(h->X.as<double>(), N), Y = cloud_at(h->Y.as<double>(), M);
    double *aux = h->aux.as<double>();
    launch_cloud_centroid(ctx, X, aux + 2);
    launch_cloud_absmax(ctx, X, aux + 2, aux);
    // sigma2_0 = gamma sum |x_n - y_m|^2 / (3 N M)
    if (int rc = first_variance(ctx, Y, X, gamma, h->ws.as<double>(), h->sc.as<double>() + 4, &h->sigma2_init)) return fail(rc);
    std::vector<double> ones((size_t)M, 1.0), am((size_t)M, 1.0 / (double)M);
    const double ident[13] = {1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->sc.p, &h->sigma2_init, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->sig.p, ones.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->alpha.p, am.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->params.p, ident, sizeof(ident), hipMemcpyHostToDevice, ctx->stream));
    if (lowrank) {
        h->lowrank.reset(new BcpdLowRank);
        const int rc = bcpd_lowrank_build(ctx, Y, beta, lowrank->relative_tolerance, lowrank->max_columns, *h->lowrank);
        if (rc != GINGR_OK) {
            (void)hipGetLastError();  // (a refused allocation must not surface again in the next call's launch check)
            return fail(rc);
        }
        if (lowrank->info) {
            const BcpdLowRank &lr = *h->lowrank;
            *lowrank->info = gingr_classic_cpd_lowrank_info{lr.plan.k, lr.tolerance_reached, lr.residual_fraction, (int64_t)lr.L.bytes};
        }
    } else {
        // G = exp(-|y_i - y_j|^2 / (2 beta^2)) over the template points (the Gaussian kernel of CPDFactory)
        launch_gauss_block(ctx, Y, Y, sqrt(2.0) * beta, 1.0, h->G.as<double>());
    }
    HANDLE_TRY(ctx, fail, hipGetLastError());
    HANDLE_TRY(ctx, fail, hipStreamSynchronize(ctx->stream));
    *out = h;
    return GINGR_OK;
}

extern "C" {

int gingr_bcpd_create(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, double w, double lambda,
                      double gamma, double kappa, double beta, gingr_bcpd **out) {
    return bcpd_create_impl(ctx, M, moving_xyz, N, target_xyz, w, lambda, gamma, kappa, beta, nullptr, out);
}

int gingr_bcpd_create_lowrank(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, double w,
                              double lambda, double gamma, double kappa, double beta, double relative_tolerance, int32_t max_columns,
                              gingr_classic_cpd_lowrank_info *info, gingr_bcpd **out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (info) memset(info, 0, sizeof(*info));
    if (!(relative_tolerance >= 0.0) || !(relative_tolerance < 1.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create_lowrank: relative tolerance must be in [0, 1)");
    if (max_columns > GINGR_CLASSIC_CPD_MAX_COLUMNS)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_create_lowrank: max_columns = %d is above the ceiling of %d factor columns",
                               (int)max_columns, GINGR_CLASSIC_CPD_MAX_COLUMNS);
    const BcpdLowRankRequest req{relative_tolerance, max_columns, info};
    return bcpd_create_impl(ctx, M, moving_xyz, N, target_xyz, w, lambda, gamma, kappa, beta, &req, out);
}

int gingr_bcpd_get_factor(gingr_bcpd *h, int32_t *columns, double *L_rowmajor_M_by_k) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (!h->lowrank)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_get_factor: the handle holds the dense kernel matrix, not a factor");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (columns) *columns = h->lowrank->plan.k;
    if (L_rowmajor_M_by_k) return lowrank_cpd_get_factor(ctx, *h->lowrank, L_rowmajor_M_by_k);
    return GINGR_OK;
}

int gingr_bcpd_iterate(gingr_bcpd *h, int32_t n_iterations) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (n_iterations < 0) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_iterate: negative count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = h->M, N = h->N, Mp = h->Mp;
    const int nb = (int)(Mp / kNBc);
    const DenseSpdWork sys(Mp, DenseSpdWork::kIdentity);
    const Cloud X = cloud_at(h->X.as<double>(), N), Yh = cloud_at(h->Yh.as<double>(), M);
    double *sc = h->sc.as<double>(), *aux = h->aux.as<double>(), *params = h->params.as<double>(), *ws = h->ws.as<double>();
    double *G = h->G.as<double>(), *Aw = h->Aw.as<double>(), *Xt = Aw ? Aw + sys.lt() : nullptr, *dh = h->dh.as<double>(), *nu = h->nu.as<double>();
    double *PX = h->PX.as<double>(), *U = h->U.as<double>(), *red = h->red.as<double>(), *mu = h->mu.as<double>();
    int32_t *flags = h->flags.as<int32_t>();
    hipStream_t st = ctx->stream;
    const unsigned gM = (unsigned)ceil_div(M, 256), gM16 = (unsigned)ceil_div(M, 16);
    if (n_iterations > 0) h->map_valid = h->coeff_ready = false;
    for (int32_t it = 0; it < n_iterations; ++it) {
        // 1  soft assignment
        launch_cloud_absmax(ctx, Yh, aux + 2, aux + 1);
        hipLaunchKernelGGL(bcpd_weights_kernel, dim3(gM), dim3(256), 0, st, M, h->w, h->alpha.as<double>(), h->sig.as<double>(), params, sc,
                           h->a.as<double>());
        hipLaunchKernelGGL(bcpd_colsum_kernel, dim3((unsigned)ceil_div(N, kBcpdTile), (unsigned)h->col.count), dim3(256), 0, st, X, Yh,
                           h->a.as<double>(), sc, aux, h->col.length, ws);
        hipLaunchKernelGGL(bcpd_den_finalize_kernel, dim3(kRedBlocks), dim3(256), 0, st, X, ws, (int)h->col.count, h->w, h->p_out, sc,
                           h->inv.as<double>(), h->nup.as<double>(), h->xpart.as<double>(), flags + 1);
        hipLaunchKernelGGL(bcpd_rowstats_kernel, dim3((unsigned)ceil_div(M, kBcpdTile), (unsigned)h->row.count), dim3(256), 0, st, Yh, X,
                           h->a.as<double>(), h->inv.as<double>(), sc, aux, h->row.length, ws);
        hipLaunchKernelGGL(bcpd_rows_finish_kernel, dim3(gM), dim3(256), 0, st, M, ws, (int)h->row.count, h->Y.as<double>(), params, sc, nu, PX,
                           h->Rr.as<double>(), dh, sc + 5);
        // 2  deformation
        if (h->lowrank) {
            BcpdLowRank &lr = *h->lowrank;
            const double *Xl = bcpd_lowrank_system(ctx, lr, nu, h->Rr.as<double>(), h->Z.as<double>(), params, sc, h->lambda, flags);
            hipLaunchKernelGGL(bcpd_forward_kernel, dim3((unsigned)(lr.plan.kp / 32)), dim3(256), 0, st, (int64_t)lr.plan.kp, Xl,
                               lr.svec.as<double>(), h->Wv.as<double>());
            bcpd_lowrank_deform(ctx, lr, Xl, h->Wv.as<double>(), h->Y.as<double>(), params, sc, h->lambda, h->V.as<double>(), U,
                                h->sig.as<double>());
        } else {
            hipLaunchKernelGGL(bcpd_kr_kernel, dim3(gM16), dim3(256), 0, st, M, Mp, G, h->lambda, h->Rr.as<double>(), dh, h->Z.as<double>(),
                               h->B.as<double>());
            launch_spd_system(st, (int)M, sys, BcpdSystemElem{G, dh, M, h->lambda}, SpdIdentityBorder{}, Aw, flags);
            dense_spd_inverse(ctx, Aw, Mp, h->Linv.as<double>(), nullptr, flags);
            hipLaunchKernelGGL(bcpd_forward_kernel, dim3((unsigned)(Mp / 32)), dim3(256), 0, st, Mp, Xt, h->B.as<double>(), h->Wv.as<double>());
            hipLaunchKernelGGL(bcpd_backward_kernel, dim3((unsigned)ceil_div(Mp, 16)), dim3(256), 0, st, Mp, Xt, h->Wv.as<double>(), h->Q.as<double>());
            hipLaunchKernelGGL(bcpd_deform_kernel, dim3(gM16), dim3(256), 0, st, M, Mp, G, h->lambda, h->Q.as<double>(), dh, h->Z.as<double>(),
                               h->Y.as<double>(), params, sc, h->V.as<double>(), U);
            hipLaunchKernelGGL(bcpd_sigma_tiles_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, st, Xt, Mp, G, M, dh, h->lambda, ws);
            hipLaunchKernelGGL(bcpd_sigma_finish_kernel, dim3(gM), dim3(256), 0, st, M, Mp, G, h->lambda, ws, nb, h->sig.as<double>());
        }
        // 3  similarity
        hipLaunchKernelGGL(bcpd_sums_a_kernel, dim3(kRedBlocks), dim3(256), 0, st, M, nu, PX, U, h->sig.as<double>(), red);
        hipLaunchKernelGGL(bcpd_means_finish_kernel, dim3(1), dim3(64), 0, st, M, h->kappa, red, h->xpart.as<double>(), sc, mu);
        hipLaunchKernelGGL(bcpd_alpha_kernel, dim3(gM), dim3(256), 0, st, M, h->kappa, nu, mu, h->alpha.as<double>());
        hipLaunchKernelGGL(bcpd_sums_b_kernel, dim3(kRedBlocks), dim3(256), 0, st, M, nu, PX, U, mu, red);
        hipLaunchKernelGGL(bcpd_similarity_kernel, dim3(1), dim3(64), 0, st, red, sc, mu, params);
        // 4  shape and variance
        hipLaunchKernelGGL(bcpd_shape_kernel, dim3(kRedBlocks), dim3(256), 0, st, M, U, params, nu, PX, h->Yh.as<double>(), red);
        hipLaunchKernelGGL(bcpd_variance_kernel, dim3(1), dim3(64), 0, st, red, params, sc, flags);
    }
    const int rc = finish_iterate(ctx, flags, 2, 1, "bcpd_iterate");
    if (rc == GINGR_OK && n_iterations > 0) h->map_valid = true;
    return rc;
}

// the coefficients of the last iteration in h->C (three planes of stride M), formed once
static int bcpd_coefficients(gingr_bcpd *h, const char *name) {
    gingr_ctx *ctx = h->ctx;
    if (!h->map_valid) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: no successful iteration since the state was created or set", name);
    if (h->coeff_ready) return GINGR_OK;
    const int64_t M = h->M;
    if (!h->C.p && h->C.alloc((size_t)3 * M * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        h->C.release();
        return gingr_set_error(ctx, GINGR_ERR_HIP, "%s: out of device memory", name);
    }
    hipLaunchKernelGGL(bcpd_coefficients_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, h->lambda, h->sc.as<double>(),
                       h->Rr.as<double>(), h->nu.as<double>(), h->V.as<double>(), h->C.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    h->coeff_ready = true;
    return GINGR_OK;
}

int gingr_bcpd_get_coefficients(gingr_bcpd *h, double *c_xyz) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (!c_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_get_coefficients: null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GINGR_TRY(bcpd_coefficients(h, "bcpd_get_coefficients"));
    return download_cloud(ctx, h->stage.as<double>(), h->C.as<double>(), h->M, c_xyz);
}

int gingr_bcpd_transform_points(gingr_bcpd *h, int64_t P, const double *points_xyz, double *out_xyz) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (P < 0 || (P > 0 && (!points_xyz || !out_xyz))) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "bcpd_transform_points: bad argument");
    if (P == 0) return GINGR_OK;  // (whatever the state: nothing is asked for)
    if (!h->map_valid)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "bcpd_transform_points: no successful iteration since the state was created or set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GINGR_TRY(bcpd_coefficients(h, "bcpd_transform_points"));
    return kernel_warp_points(ctx, h->warp, cloud_at(h->Y.as<double>(), h->M), h->C.as<double>(), h->M, h->beta, h->params.as<double>(), false, P,
                              points_xyz, out_xyz);
}

int gingr_bcpd_get(gingr_bcpd *h, double *yhat_xyz, double *vhat_xyz, double *sigma_diag, double *alpha, double *nu, double *nu_prime,
                   double *transform13, double *scalars3) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = h->M, N = h->N;
    hipStream_t st = ctx->stream;
    double *const aos[2] = {yhat_xyz, vhat_xyz};
    const double *const soa[2] = {h->Yh.as<double>(), h->V.as<double>()};
    for (int q = 0; q < 2; ++q)
        if (aos[q]) GINGR_TRY(download_cloud(ctx, h->stage.as<double>(), soa[q], M, aos[q]));
    if (sigma_diag) HIP_TRY(ctx, hipMemcpyAsync(sigma_diag, h->sig.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (alpha) HIP_TRY(ctx, hipMemcpyAsync(alpha, h->alpha.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nu) HIP_TRY(ctx, hipMemcpyAsync(nu, h->nu.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nu_prime) HIP_TRY(ctx, hipMemcpyAsync(nu_prime, h->nup.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (transform13) HIP_TRY(ctx, hipMemcpyAsync(transform13, h->params.p, 13 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (scalars3) HIP_TRY(ctx, hipMemcpyAsync(scalars3, h->sc.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return GINGR_OK;
}

int gingr_bcpd_set(gingr_bcpd *h, const double *yhat_xyz, const double *sigma_diag, const double *alpha, const double *transform13,
                   double sigma2) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = h->M;
    hipStream_t st = ctx->stream;
    h->map_valid = h->coeff_ready = false;
    if (yhat_xyz) GINGR_TRY(upload_cloud(ctx, h->stage.as<double>(), yhat_xyz, M, h->Yh.as<double>()));
    if (sigma_diag) HIP_TRY(ctx, hipMemcpyAsync(h->sig.p, sigma_diag, (size_t)M * sizeof(double), hipMemcpyHostToDevice, st));
    if (alpha) HIP_TRY(ctx, hipMemcpyAsync(h->alpha.p, alpha, (size_t)M * sizeof(double), hipMemcpyHostToDevice, st));
    if (transform13) HIP_TRY(ctx, hipMemcpyAsync(h->params.p, transform13, 13 * sizeof(double), hipMemcpyHostToDevice, st));
    if (sigma2 > 0.0) HIP_TRY(ctx, hipMemcpyAsync(h->sc.p, &sigma2, sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return GINGR_OK;
}

}  // extern "C"
