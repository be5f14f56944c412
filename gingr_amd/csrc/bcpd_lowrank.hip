// Bayesian coherent point drift past dense sizes: the deformation step (step 2 of bcpd.hip) over a low-rank factor of the kernel
// matrix, the acceleration Hirose 2020 proposes.  With L (M x k, G ~ L L^T: the factor of classic_cpd_lowrank.hip), K = L L^T / lambda,
// c2 = s^2 / sigma2 and r as bcpd_rows_finish_kernel writes it, Sigma = K - K D^1/2 (I + D^1/2 K D^1/2)^-1 D^1/2 K, D = c2 diag nu,
// becomes by the push-through identity Sigma = L C^-1 L^T / lambda with
//
//     S = L^T diag(nu) L  (k x k)        s = L^T r  (k x 3)        C = I + (c2 / lambda) S = R R^T        X = R^-T
//     T = L X  (M x k, never stored)     w = X^T s = R^-1 s
//     v^ = c2 Sigma r = (c2 / lambda) T w          u^ = y + v^          sigma_m^2 = Sigma_mm = |row m of T|^2 / lambda
//
// (T w = L C^-1 s: the solution z = C^-1 s itself is never needed, the pass that forms T for sigma_m^2 multiplies it by w on the way).
// sigma_m^2 is a sum of squares: never negative, no K_mm - ... cancellation; nothing divides by nu_m and nothing is of size M x M.
// C is positive definite for any nu >= 0.  Rows and columns k .. kp - 1 of the padded system are the identity and the padded columns
// of L are zero: T is zero there and adds +0.
//
//   lowrank_gram (classic_cpd_lowrank.hip)   pass 1: S and s on the float64 MFMA, with P1 := nu, PX := r and a zero ty
//   spd_system_kernel, dense_spd_inverse     C in its identity-border form -> X = R^-T (dense_spd.hip)
//   bcpd_forward_kernel (bcpd.hip)           w = X^T s
//   bcpd_lowrank_deform_kernel               pass 2: T = L X on the float64 MFMA, reduced on the fly to v^, u^ and sigma_m^2
#include "bcpd_lowrank.h"

#include "cloud_sums.h"
#include "dense_spd.h"

namespace {

using lowrank_plan::kBlock;

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct BcpdLowRankElem {  // I + (c2 / lambda) S, c2 = s^2 / sigma2 read from the device scalars
    const double *__restrict__ S;
    int kp;
    const double *__restrict__ params, *__restrict__ sc;
    double lambda;
    __device__ double operator()(int64_t row, int64_t c) const {
        const double cl = params[0] * params[0] / sc[0] / lambda;
        return cl * S[row * kp + c] + (row == c ? 1.0 : 0.0);
    }
};

constexpr int kRows = 64;  // rows of L to a workgroup: wave w owns the rows 16 w .. 16 w + 15
constexpr int kHalf = 32;  // columns of L (= rows of X) staged at a time
// Row strides of the staged pieces in doubles.  The A operand is read across the rows of the L piece (lane l: row l & 15, column
// l >> 4): 34 doubles = 68 dwords put the sixteen rows of a 32-lane half four banks apart and its two columns two banks apart, so
// the 32 eight-byte reads of a half cover the 64 banks once.  The B operand is read along the rows of the X piece, as in
// bcpd_sigma_tiles_kernel: 80 doubles put the second row of a half on the other half of the 256-byte bank row.
constexpr int kLdA = kHalf + 2;
constexpr int kLdB = kBlock + 16;

// Pass 2.  Workgroup g: the rows m = 64 g .. 64 g + 63 of T = L X, one 64 x 64 tile (column block bj) at a time,
//   T[m][j] = sum_{i <= j} L[m][i] X[i][j],
// summed over the column blocks bi <= bj of L (X is upper triangular: block products with bi > bj are skipped), 32 columns of L at a
// time: the 64 x 32 piece of L and the 32 x 64 piece of X reach LDS by 16-byte loads, one piece ahead in registers.  Fragment layout
// of v_mfma_f64_16x16x4: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds
// D[i = (l >> 4) + 4 reg][j = l & 15].  A finished tile is folded into the lane's sums for its four rows, sum_j T[m][j]^2 and
// sum_j T[m][j] w_d[j]: over k inside a tile, over the tiles' columns and the column blocks in index order, at the end over the sixteen
// lanes of a row by the fixed butterfly of sum16.  Two runs give the same bits.
__global__ __launch_bounds__(256) void bcpd_lowrank_deform_kernel(const double *__restrict__ L, int64_t Mpad, int64_t M, int nb, int kp,
                                                                  const double *__restrict__ X, const double *__restrict__ wv,
                                                                  const double *__restrict__ y, const double *__restrict__ params,
                                                                  const double *__restrict__ sc, double lambda, double *__restrict__ vhat,
                                                                  double *__restrict__ u, double *__restrict__ sig) {
    __shared__ __attribute__((aligned(16))) double As[kRows * kLdA], Bs[kHalf * kLdB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * kRows;
    double ra[8], rb[8];
    auto load = [&](int bi, int bj, int half) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = q * 256 + tid;
            // (a workgroup's last rows may lie past the padded factor: they repeat its last row, and rows from M on are never written)
            const int64_t row = m0 + (e >> 4) < Mpad ? m0 + (e >> 4) : Mpad - 1;
            const double2 a = *reinterpret_cast<const double2 *>(L + ((int64_t)bi * Mpad + row) * kBlock + kHalf * half + 2 * (e & 15));
            const double2 b = *reinterpret_cast<const double2 *>(X + (int64_t)(bi * kBlock + kHalf * half + (e >> 5)) * kp + bj * kBlock + 2 * (e & 31));
            ra[2 * q] = a.x, ra[2 * q + 1] = a.y;
            rb[2 * q] = b.x, rb[2 * q + 1] = b.y;
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = q * 256 + tid;
            *reinterpret_cast<double2 *>(As + (e >> 4) * kLdA + 2 * (e & 15)) = double2{ra[2 * q], ra[2 * q + 1]};
            *reinterpret_cast<double2 *>(Bs + (e >> 5) * kLdB + 2 * (e & 31)) = double2{rb[2 * q], rb[2 * q + 1]};
        }
    };
    v4f64 acc[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = v4f64{0.0, 0.0, 0.0, 0.0};
    double sq[4] = {0.0, 0.0, 0.0, 0.0}, vv[3][4];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) vv[d][g] = 0.0;
    load(0, 0, 0);
    for (int bj = 0; bj < nb; ++bj) {
        for (int bi = 0; bi <= bj; ++bi)
            for (int half = 0; half < 2; ++half) {
                __syncthreads();  // the previous piece has been read
                store();
                __syncthreads();
                {  // the piece after this one, in the order of these loops
                    int nbi = bi, nbj = bj, nhalf = half + 1;
                    if (nhalf == 2) {
                        nhalf = 0;
                        if (++nbi > nbj) {
                            nbi = 0;
                            ++nbj;
                        }
                    }
                    if (nbj < nb) load(nbi, nbj, nhalf);
                }
#pragma unroll
                for (int q = 0; q < kHalf / 4; ++q) {
                    const double a = As[(16 * wave + l15) * kLdA + 4 * q + l4];
#pragma unroll
                    for (int tj = 0; tj < 4; ++tj)
                        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(4 * q + l4) * kLdB + 16 * tj + l15], acc[tj], 0, 0, 0);
                }
            }
        // the tile (rows of the workgroup, column block bj) is complete
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            const int j = bj * kBlock + 16 * tj + l15;
            const double w0 = wv[j], w1 = wv[kp + j], w2 = wv[2 * kp + j];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double t = acc[tj][g];
                sq[g] = __builtin_fma(t, t, sq[g]);
                vv[0][g] = __builtin_fma(t, w0, vv[0][g]);
                vv[1][g] = __builtin_fma(t, w1, vv[1][g]);
                vv[2][g] = __builtin_fma(t, w2, vv[2][g]);
            }
            acc[tj] = v4f64{0.0, 0.0, 0.0, 0.0};
        }
    }
    const double cl = params[0] * params[0] / sc[0] / lambda;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const double s = sum16(sq[g]), a0 = sum16(vv[0][g]), a1 = sum16(vv[1][g]), a2 = sum16(vv[2][g]);
        const int64_t m = m0 + 16 * wave + l4 + 4 * g;
        if (l15 == 0 && m < M) {
            const double v[3] = {cl * a0, cl * a1, cl * a2};
            sig[m] = s / lambda;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                vhat[d * M + m] = v[d];
                u[d * M + m] = y[d * M + m] + v[d];
            }
        }
    }
}

}  // namespace

int bcpd_lowrank_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, BcpdLowRank &lr) {
    GINGR_TRY(lowrank_factor_build(ctx, Y, beta, relative_tolerance, max_columns, "bcpd_create_lowrank", lr));
    const DenseSpdWork sys(lr.plan.k, DenseSpdWork::kIdentity);  // sys.Mp == plan.kp: both round k up to 64
    HIP_TRY(ctx, lr.Aw.alloc((size_t)sys.aw_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.Linv.alloc((size_t)sys.linv_doubles() * sizeof(double)));
    return GINGR_OK;
}

const double *bcpd_lowrank_system(gingr_ctx *ctx, BcpdLowRank &lr, const double *nu, const double *r, const double *zero,
                                  const double *params, const double *sc, double lambda, int32_t *flags) {
    const lowrank_plan::Plan &p = lr.plan;
    const DenseSpdWork sys(p.k, DenseSpdWork::kIdentity);
    double *Aw = lr.Aw.as<double>();
    lowrank_gram(ctx, lr, nu, r, zero);  // u = r - nu . 0 = r exactly
    launch_spd_system(ctx->stream, p.k, sys, BcpdLowRankElem{lr.S.as<double>(), p.kp, params, sc, lambda}, SpdIdentityBorder{}, Aw, flags);
    dense_spd_inverse(ctx, Aw, sys.Mp, lr.Linv.as<double>(), nullptr, flags);
    return Aw + sys.lt();
}

void bcpd_lowrank_deform(gingr_ctx *ctx, const BcpdLowRank &lr, const double *X, const double *wv, const double *y, const double *params,
                         const double *sc, double lambda, double *vhat, double *u, double *sig) {
    const lowrank_plan::Plan &p = lr.plan;
    hipLaunchKernelGGL(bcpd_lowrank_deform_kernel, dim3((unsigned)ceil_div(p.M, kRows)), dim3(256), 0, ctx->stream, lr.L.as<double>(), p.Mpad,
                       p.M, p.nb, p.kp, X, wv, y, params, sc, lambda, vhat, u, sig);
}
