// Non-rigid classic CPD past dense sizes: the Maximization over a low-rank factor of the kernel matrix (Myronenko & Song 2010,
// "fast implementation": G ~ L L^T and the Woodbury identity).  With L (M x k) from the pivoted Cholesky of gpmm.hip, D = diag(P1),
// c = lambda sigma2 and B = D^-1 P X - Y, the reference's step (G + c D^-1) W = B, TY = Y + G W (NonRigidCPD.scala:45-88) becomes
//
//     S = L^T D L  (k x k)        s = L^T (P X - D Y)  (k x 3)        (c I + S) z = s
//     V = L z                     TY = Y + V                          W = D (B - V) / c
//
// (L^T W = z exactly, so TY = Y + L L^T W needs no second reduction.)  Two passes over L and one k x k solve with three right-hand
// sides (dense_spd.hip); nothing of size M x M exists.
//
//   lowrank_gram_kernel    pass 1: S and s on the float64 MFMA (v_mfma_f64_16x16x4), one 64 x 64 block pair x one row slab per
//                          workgroup, rows staged through LDS in chunks of 32
//   lowrank_reduce_kernel  the slab partials in index order -> S (both triangles), s
//   lowrank_apply_kernel   pass 2: V, TY, W and the partial sums of sigma2', 16 lanes per row
//   lowrank_finish_kernel  sigma2' (the formula of nonrigid_finish_kernel over this pass's partials)
#include "classic_cpd_lowrank.h"

#include "cloud_sums.h"
#include "dense_spd.h"
#include "gpmm_factor.h"

#include <algorithm>
#include <cmath>

namespace {

using lowrank_plan::kBlock;
using lowrank_plan::kChunk;

typedef double v4f64 __attribute__((ext_vector_type(4)));

// Row stride of a staged block in doubles.  A fragment read takes rows r and r + 1 in one 32-lane half: 80 doubles = 640 bytes put
// the second row on the other half of the 256-byte bank row (a stride of 64 would make the two rows collide two-way).
constexpr int kLdsRow = kBlock + 16;
constexpr int kTile = kBlock * kBlock;

// L_b[i][j] = Lb[64 b + j][i] (the pivoted Cholesky's [column][point] layout), zero past (M, k)
__global__ __launch_bounds__(256) void lowrank_layout_kernel(const double *__restrict__ Lb, int64_t M, int64_t Mpad, int32_t k, int32_t nb,
                                                             double *__restrict__ L) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nb * Mpad * kBlock) return;
    const int j = (int)(idx & (kBlock - 1));
    const int64_t row = idx >> 6;
    const int64_t b = row / Mpad, i = row - b * Mpad;
    const int64_t c = b * kBlock + j;
    L[idx] = (i < M && c < k) ? Lb[c * M + i] : 0.0;
}

// Pass 1.  Workgroup (slab, pair): the 64 x 64 block  sum_i p_i L[i][64 bi + a] L[i][64 bj + b]  over the slab's rows, wave w the
// strip a in [16 w, 16 w + 16) as four MFMA tiles.  Diagonal pairs also form  sum_i L[i][64 bi + a] u_d[i],  u = P X - D Y, as a
// fifth tile whose B operand carries u in its first three columns.  Rows of a chunk reach LDS by 16-byte loads of contiguous memory
// (a chunk of a block is 16 KB in one piece), one chunk ahead in registers.
template <bool DIAG>
__device__ __forceinline__ void lowrank_gram_body(const double *__restrict__ La, const double *__restrict__ Lbk, int64_t M, int64_t r0,
                                                  int64_t r1, const double *__restrict__ P1, const double *__restrict__ PX,
                                                  const double *__restrict__ ty, double *__restrict__ sh, double *__restrict__ out,
                                                  double *__restrict__ rhs_out) {
    double *sa = sh, *sb = DIAG ? sh : sh + kChunk * kLdsRow, *sp = sh + 2 * kChunk * kLdsRow, *su = sp + kChunk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, cl = lane & 15;
    double2 ra[4], rb[4];
    double rp = 0.0, ru = 0.0;
    auto load = [&](int64_t r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t off = r * kBlock + 2 * (q * 256 + tid);
            ra[q] = *reinterpret_cast<const double2 *>(La + off);
            if (!DIAG) rb[q] = *reinterpret_cast<const double2 *>(Lbk + off);
        }
        if (tid < kChunk) {
            const int64_t i = r + tid;
            rp = i < M ? P1[i] : 0.0;
        } else if (DIAG && tid >= 64 && tid < 64 + 3 * kChunk) {
            const int d = (tid - 64) / kChunk;
            const int64_t i = r + (tid - 64) % kChunk;
            ru = i < M ? PX[d * M + i] - P1[i] * ty[d * M + i] : 0.0;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = q * 256 + tid, row = e >> 5, c2 = e & 31;
            *reinterpret_cast<double2 *>(sa + row * kLdsRow + 2 * c2) = ra[q];
            if (!DIAG) *reinterpret_cast<double2 *>(sb + row * kLdsRow + 2 * c2) = rb[q];
        }
        if (tid < kChunk)
            sp[tid] = rp;
        else if (DIAG && tid >= 64 && tid < 64 + 3 * kChunk)
            su[tid - 64] = ru;
    };
    v4f64 acc[4], accu = v4f64{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4f64{0, 0, 0, 0};
    load(r0);
    for (int64_t r = r0; r < r1; r += kChunk) {
        __syncthreads();  // the previous chunk has been read
        store();
        __syncthreads();
        if (r + kChunk < r1) load(r + kChunk);
#pragma unroll
        for (int ks = 0; ks < kChunk / 4; ++ks) {
            const int row = 4 * ks + kq;
            const double a = sa[row * kLdsRow + 16 * wave + cl];
            const double aw = a * sp[row];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, sb[row * kLdsRow + 16 * t + cl], acc[t], 0, 0, 0);
            if (DIAG) accu = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cl < 3 ? su[cl * kChunk + row] : 0.0, accu, 0, 0, 0);
        }
    }
    // D[i][j]: i = kq + 4 reg on the A side, j = cl on the B side
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(16 * wave + kq + 4 * reg) * kBlock + 16 * t + cl] = acc[t][reg];
    if (DIAG && cl < 3)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) rhs_out[cl * kBlock + 16 * wave + kq + 4 * reg] = accu[reg];
}

__global__ __launch_bounds__(256) void lowrank_gram_kernel(const double *__restrict__ L, int64_t Mpad, int64_t M, int nb, int npairs,
                                                           int64_t rows_per_slab, const double *__restrict__ P1,
                                                           const double *__restrict__ PX, const double *__restrict__ ty,
                                                           double *__restrict__ gram_part, double *__restrict__ rhs_part) {
    __shared__ __attribute__((aligned(16))) double sh[2 * kChunk * kLdsRow + 4 * kChunk];
    int bi, bj;
    lowrank_plan::pair_of((int)blockIdx.y, nb, bi, bj);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab, r1 = min(Mpad, r0 + rows_per_slab);
    const double *La = L + (int64_t)bi * Mpad * kBlock, *Lbk = L + (int64_t)bj * Mpad * kBlock;
    double *out = gram_part + ((int64_t)blockIdx.x * npairs + blockIdx.y) * kTile;
    double *rhs_out = rhs_part + ((int64_t)blockIdx.x * nb + bi) * 3 * kBlock;
    if (bi == bj)
        lowrank_gram_body<true>(La, Lbk, M, r0, r1, P1, PX, ty, sh, out, rhs_out);
    else
        lowrank_gram_body<false>(La, Lbk, M, r0, r1, P1, PX, ty, sh, out, rhs_out);
}

// S and s from the slab partials, slab 0 first.  One thread per element; a diagonal pair holds both (a, b) and (b, a), computed from
// differently rounded products: the one with a <= b is taken for both.
__global__ __launch_bounds__(256) void lowrank_reduce_kernel(const double *__restrict__ gram_part, const double *__restrict__ rhs_part,
                                                             int nslabs, int nb, int npairs, int kp, double *__restrict__ S,
                                                             double *__restrict__ svec) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ng = (int64_t)npairs * kTile;
    if (idx < ng) {
        const int p = (int)(idx / kTile), e = (int)(idx % kTile), a = e / kBlock, b = e % kBlock;
        int bi, bj;
        lowrank_plan::pair_of(p, nb, bi, bj);
        if (bi == bj && a > b) return;
        double v = 0.0;
        for (int s = 0; s < nslabs; ++s) v += gram_part[((int64_t)s * npairs + p) * kTile + e];
        const int ga = bi * kBlock + a, gb = bj * kBlock + b;
        S[(int64_t)ga * kp + gb] = v;
        S[(int64_t)gb * kp + ga] = v;
    } else if (idx - ng < (int64_t)nb * 3 * kBlock) {
        const int q = (int)(idx - ng), bi = q / (3 * kBlock), e = q % (3 * kBlock), d = e / kBlock, a = e % kBlock;
        double v = 0.0;
        for (int s = 0; s < nslabs; ++s) v += rhs_part[((int64_t)s * nb + bi) * 3 * kBlock + e];
        svec[d * kp + bi * kBlock + a] = v;
    }
}

struct LowRankElem {  // c I + S, c = lambda sigma2 read from the device scalar
    const double *__restrict__ S;
    int kp;
    const double *__restrict__ scalars;
    double lambda;
    __device__ double operator()(int64_t row, int64_t c) const { return S[row * kp + c] + (row == c ? lambda * scalars[8] : 0.0); }
};
struct LowRankBorder {  // s in the first three border rows
    const double *__restrict__ svec;
    int kp;
    __device__ double operator()(int64_t brow, int64_t c, int r) const { return (brow < 3 && c < r) ? svec[brow * kp + c] : 0.0; }
};

// Pass 2.  Sixteen lanes per row: lane l adds the columns {32 h + 2 l, 32 h + 2 l + 1} of every block in ascending order, the
// sixteen sums are combined by a fixed butterfly.  partial[group] = {sum_i P1_i |TY_i|^2, sum_i TY_i . PX_i}.
__global__ __launch_bounds__(256) void lowrank_apply_kernel(const double *__restrict__ L, int64_t Mpad, int64_t M, int nb, int kp,
                                                            const double *__restrict__ z, const double *__restrict__ P1,
                                                            const double *__restrict__ PX, double *__restrict__ ty,
                                                            const double *__restrict__ scalars, double lambda, double *__restrict__ W,
                                                            int64_t w_stride, double *__restrict__ partial) {
    __shared__ double zs[3 * lowrank_plan::kMaxColumns];
    __shared__ double sh[256];
    for (int t = threadIdx.x; t < 3 * kp; t += 256) zs[t] = z[t];
    __syncthreads();
    const double c = lambda * scalars[8];
    const int lane16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
    double sums[2] = {0, 0};  // sum_i P1_i |TY_i|^2, sum_i TY_i . PX_i
    for (int64_t i = (int64_t)blockIdx.x * lowrank_plan::kApplyRows + grp; i < M; i += (int64_t)gridDim.x * lowrank_plan::kApplyRows) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int b = 0; b < nb; ++b) {
            const double *row = L + ((int64_t)b * Mpad + i) * kBlock;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double2 l = *reinterpret_cast<const double2 *>(row + 32 * h + 2 * lane16);
                const int col = b * kBlock + 32 * h + 2 * lane16;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    v[d] = __builtin_fma(l.x, zs[d * kp + col], v[d]);
                    v[d] = __builtin_fma(l.y, zs[d * kp + col + 1], v[d]);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = sum16(v[d]);
        if (lane16 == 0) {
            const double p = P1[i];
            double tn[3], px[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double y = ty[d * M + i];
                px[d] = PX[d * M + i];
                tn[d] = y + v[d];
                ty[d * M + i] = tn[d];
                W[d * w_stride + i] = ((px[d] - p * y) - p * v[d]) / c;
            }
            sums[0] += p * ((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
            sums[1] += (tn[0] * px[0] + tn[1] * px[1]) + tn[2] * px[2];
        }
    }
    block_sums<2>(sums, sh, partial + blockIdx.x * 2);
}

// sigma2' = (xPx - 2 tr(TY^T P X) + sum P1 |TY|^2) / (3 Np)      (NonRigidCPD.scala:74-77)
__global__ __launch_bounds__(256) void lowrank_finish_kernel(const double *__restrict__ partial, int n, double *__restrict__ scalars,
                                                             const int32_t *__restrict__ sysflag, int32_t *__restrict__ flag) {
    __shared__ double sh[256];
    double a = 0.0, b = 0.0;
    for (int q = threadIdx.x; q < n; q += 256) {
        a += partial[q * 2];
        b += partial[q * 2 + 1];
    }
    const double ypy = block_sum<256>(a, sh);
    __syncthreads();  // sh is reused
    const double tr = block_sum<256>(b, sh);
    if (threadIdx.x != 0) return;
    const double ns = (scalars[1] - 2 * tr + ypy) / (scalars[0] * 3.0);
    scalars[8] = ns;
    if (!finite_d(ns)) *flag = GINGR_ERR_NONFINITE;
    if (*sysflag) *flag = *sysflag;
}

}  // namespace

int lowrank_factor_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, const char *who,
                         LowRankFactor &lr) {
    const int64_t M = Y.n;
    const int32_t cap = (int32_t)std::min<int64_t>(M, max_columns > 0 ? max_columns : lowrank_plan::kMaxColumns);
    int32_t k = 0;
    {
        gpmm_factor::Factor fac;  // its buffers ([cap][M] and the pivot search) live until the factor is laid out
        GINGR_TRY(fac.init(ctx, gpmm_factor::gaussian_specs(sqrt(2.0) * beta, 1.0), Y, false, cap));
        GINGR_TRY(fac.run_to_tolerance(relative_tolerance));
        k = fac.ks;
        if (k < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: empty factor (tolerance too large)", who);
        const double residual = fac.htrace[(size_t)k], trace = fac.htrace[0];
        lr.residual_fraction = residual / trace;
        lr.tolerance_reached = (residual < relative_tolerance * trace || (int64_t)k == M) ? 1 : 0;
        lr.plan = lowrank_plan::make_plan(M, k);
        const lowrank_plan::Plan &p = lr.plan;
        HIP_TRY(ctx, lr.L.alloc((size_t)p.factor_doubles() * sizeof(double)));
        hipLaunchKernelGGL(lowrank_layout_kernel, dim3((unsigned)ceil_div(p.factor_doubles(), 256)), dim3(256), 0, ctx->stream,
                           fac.Lb.as<double>(), M, p.Mpad, k, p.nb, lr.L.as<double>());
        GINGR_TRY(check_launch(ctx));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const lowrank_plan::Plan &p = lr.plan;
    HIP_TRY(ctx, lr.gram_part.alloc((size_t)p.gram_partial_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.rhs_part.alloc((size_t)p.rhs_partial_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.S.alloc((size_t)p.kp * p.kp * sizeof(double)));
    HIP_TRY(ctx, lr.svec.alloc((size_t)3 * p.kp * sizeof(double)));
    return GINGR_OK;
}

int lowrank_cpd_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, LowRankCpd &lr) {
    GINGR_TRY(lowrank_factor_build(ctx, Y, beta, relative_tolerance, max_columns, "classic_cpd_create_lowrank", lr));
    const lowrank_plan::Plan &p = lr.plan;
    const DenseSpdWork sys(p.k, DenseSpdWork::kRhsRows);
    HIP_TRY(ctx, lr.Aw.alloc((size_t)sys.aw_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.Linv.alloc((size_t)sys.linv_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.Z.alloc((size_t)sys.w_doubles() * sizeof(double)));
    HIP_TRY(ctx, lr.sysflag.alloc(2 * sizeof(int32_t)));
    HIP_TRY(ctx, lr.apply_part.alloc((size_t)2 * p.apply_groups * sizeof(double)));
    return GINGR_OK;
}

void lowrank_gram(gingr_ctx *ctx, LowRankFactor &lr, const double *P1, const double *PX, const double *ty) {
    const lowrank_plan::Plan &p = lr.plan;
    hipLaunchKernelGGL(lowrank_gram_kernel, dim3((unsigned)p.nslabs, (unsigned)p.npairs), dim3(256), 0, ctx->stream, lr.L.as<double>(),
                       p.Mpad, p.M, p.nb, p.npairs, p.rows_per_slab, P1, PX, ty, lr.gram_part.as<double>(), lr.rhs_part.as<double>());
    const int64_t nred = (int64_t)p.npairs * kTile + (int64_t)p.nb * 3 * kBlock;
    hipLaunchKernelGGL(lowrank_reduce_kernel, dim3((unsigned)ceil_div(nred, 256)), dim3(256), 0, ctx->stream, lr.gram_part.as<double>(),
                       lr.rhs_part.as<double>(), p.nslabs, p.nb, p.npairs, p.kp, lr.S.as<double>(), lr.svec.as<double>());
}

void lowrank_cpd_mstep(gingr_ctx *ctx, LowRankCpd &lr, const double *P1, const double *PX, double *ty, double *scalars, double lambda,
                       double *W, int64_t w_stride, int32_t *flag) {
    const lowrank_plan::Plan &p = lr.plan;
    const DenseSpdWork sys(p.k, DenseSpdWork::kRhsRows);  // sys.Mp == p.kp: both round k up to 64
    int32_t *sysflag = lr.sysflag.as<int32_t>();
    lowrank_gram(ctx, lr, P1, PX, ty);
    launch_spd_system(ctx->stream, p.k, sys, LowRankElem{lr.S.as<double>(), p.kp, scalars, lambda}, LowRankBorder{lr.svec.as<double>(), p.kp},
                      lr.Aw.as<double>(), sysflag);
    dense_spd_solve3(ctx, lr.Aw.as<double>(), sys.Mp, lr.Linv.as<double>(), lr.Z.as<double>(), sysflag);
    hipLaunchKernelGGL(lowrank_apply_kernel, dim3((unsigned)p.apply_groups), dim3(256), 0, ctx->stream, lr.L.as<double>(), p.Mpad, p.M, p.nb,
                       p.kp, lr.Z.as<double>(), P1, PX, ty, scalars, lambda, W, w_stride, lr.apply_part.as<double>());
    hipLaunchKernelGGL(lowrank_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, lr.apply_part.as<double>(), p.apply_groups, scalars, sysflag,
                       flag);
}

int lowrank_cpd_get_factor(gingr_ctx *ctx, const LowRankFactor &lr, double *out) {
    const lowrank_plan::Plan &p = lr.plan;
    std::vector<double> hl((size_t)p.factor_doubles());
    HIP_TRY(ctx, hipMemcpyAsync(hl.data(), lr.L.p, hl.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < p.M; ++i)
        for (int32_t c = 0; c < p.k; ++c) out[i * p.k + c] = hl[(size_t)p.at(i, c)];
    return GINGR_OK;
}
