// Basis packing and the basis sweeps of the GiNGR update for gfx950 (MI355X).
//
//   sweep_kernel      every pass over the 3M x r basis: Q^T L (y - m) (G/api/GingrAlgorithm.scala:300), coefficients (:215,236),
//                     instance (:222,224, ModelFittingParameters.scala:134), Umeyama partial sums (:260-279);
//                     HBM-bound streaming of Q0, fused with the pose / projection epilogues
//
// Layout: Q0 is row-major [3M][rp]: the 3 x rp block of one point is contiguous (2.7 KB at r = 100), so one point's
// observation weight, rotation and epilogue touch one contiguous block; rp = rank rounded up to 16 (MFMA tile).
// All reductions across workgroups go through per-block partials combined in a fixed order (bitwise reproducible).
#include "gp.h"
#include "gp_device.h"

#include <algorithm>

namespace {

// Basis of a model on a NEW reference whose every point takes a fixed convex combination of three source points (nearest
// neighbour: weights (1,0,0); triangle-mesh interpolation: barycentric weights of the closest surface point):
//   Q0_new[(3 s + d) rp + q] = sum_k w[3 o + k] Q0_src[(3 inv_src[ids[3 o + k]] + d) rp + q],   o = row_begin + perm_new[s]
__global__ __launch_bounds__(256) void interp_pack_kernel(const double *__restrict__ Qs, int32_t rp, const int32_t *__restrict__ inv_src,
                                                          const int32_t *__restrict__ ids, const double *__restrict__ w,
                                                          const int32_t *__restrict__ perm_new, int64_t row_begin, int64_t M,
                                                          double *__restrict__ Q0) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * M * rp) return;
    const int64_t row = idx / rp;
    const int32_t q = (int32_t)(idx - row * rp);
    const int64_t s = row / 3;
    const int d = (int)(row - 3 * s);
    const int64_t o = row_begin + perm_new[s];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double wk = w[3 * o + k];
        if (wk != 0.0) acc += wk * Qs[((int64_t)3 * inv_src[ids[3 * o + k]] + d) * rp + q];
    }
    Q0[idx] = acc;
}

// ------------------------------------------------------------------------------------------------- basis packing
__global__ void pack_basis_kernel(const double *__restrict__ stage, const double *__restrict__ variance, int64_t rows,
                                  int32_t r, int32_t rp, const int32_t *__restrict__ perm, double *__restrict__ Q0) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * rp) return;
    const int64_t row = idx / rp;
    const int32_t k = (int32_t)(idx - row * rp);
    const int64_t pt = row / 3, d = row - 3 * pt;
    const int64_t src = 3 * (int64_t)(perm ? perm[pt] : pt) + d;
    // Q(i, j) = eigenvector * sqrt(eigenvalue)   (scalismo genericRegressionComputations)
    Q0[idx] = k < r ? stage[(int64_t)k * rows + src] * sqrt(variance[k]) : 0.0;
}

// ------------------------------------------------------------------------------------------------- basis sweeps
constexpr int kSweepThreads = 256;
constexpr int kGroups = kSweepThreads / 16;  // points per block step
constexpr int kSweepMaxBlocks = 1024;

template <int MODE, int KMAX>
__global__ __launch_bounds__(kSweepThreads) void sweep_kernel(SweepArgs a) {
    constexpr bool FWD = (MODE == SWEEP_PROJ1 || MODE == SWEEP_SHAPES || MODE == SWEEP_FIT || MODE == SWEEP_POSED);
    constexpr bool FWD2 = (MODE == SWEEP_SHAPES);
    constexpr bool TRANS = (MODE == SWEEP_RHS || MODE == SWEEP_PROJ1 || MODE == SWEEP_PROJ2 || MODE == SWEEP_RHS_ICP);
    extern __shared__ double lds[];  // [2*rp] coefficients, then [kGroups*rp] reduction scratch
    const int tid = threadIdx.x, lane16 = tid & 15, grp = tid >> 4;
    const int rp = a.rp, km = rp >> 4;
    const int64_t M = a.M;
    double *coef = lds;
    double *red = lds + 2 * rp;
    if (MODE == SWEEP_RHS && !gate_open(a.gate)) return;  // (workgroup-uniform)
    if (a.zero_slot && blockIdx.x == 0 && tid == 0) *a.zero_slot = 0.0;  // e.g. the |coordinate| maximum of the fit this pass rewrites
    if (FWD) {
        for (int k = tid; k < rp; k += kSweepThreads) {
            coef[k] = a.coef0[k];
            if (FWD2) coef[rp + k] = a.coef1[k];
        }
        __syncthreads();
    }
    // pose scalars (wave-uniform loads)
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0}, cen[3] = {0, 0, 0}, scale = 1.0;
    if (MODE == SWEEP_SHAPES || MODE == SWEEP_FIT || MODE == SWEEP_POSED || MODE == SWEEP_RHS_ICP) {
        for (int q = 0; q < 9; ++q) R[q] = a.state->R[q];
        for (int q = 0; q < 3; ++q) {
            tr[q] = a.state->t[q];
            cen[q] = a.state->center[q];
        }
        scale = a.state->scale;
    } else if (MODE == SWEEP_PROJ2) {
        if (a.frame) {  // the rigid part of a device state directly (scale 1): no pose object has to be filled first
            for (int q = 0; q < 9; ++q) R[q] = a.frame->R[q];
            for (int q = 0; q < 3; ++q) {
                tr[q] = a.frame->t[q];
                cen[q] = a.frame->center[q];
            }
        } else {
            for (int q = 0; q < 9; ++q) R[q] = a.pose->R[q];
            for (int q = 0; q < 3; ++q) {
                tr[q] = a.pose->t[q];
                cen[q] = a.pose->center[q];
            }
        }
    }
    double acc[KMAX];
#pragma unroll
    for (int m = 0; m < KMAX; ++m) acc[m] = 0.0;
    double us[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) us[s] = 0.0;

    for (int64_t base = (int64_t)blockIdx.x * kGroups; base < M; base += (int64_t)gridDim.x * kGroups) {
        const int64_t p = base + grp;
        const bool valid = p < M;
        const int64_t pc = valid ? p : 0;
        const double *q0 = a.Q0 + (3 * pc) * rp + lane16;
        const double *q1 = q0 + rp;
        const double *q2 = q1 + rp;
        double f0[3] = {0, 0, 0}, f1[3] = {0, 0, 0};
        if (FWD) {
#pragma unroll 4
            for (int m = 0; m < km; ++m) {
                const int k = m * 16;
                const double c0 = coef[k + lane16];
                const double u0 = q0[k], u1 = q1[k], u2 = q2[k];
                f0[0] = __builtin_fma(u0, c0, f0[0]);
                f0[1] = __builtin_fma(u1, c0, f0[1]);
                f0[2] = __builtin_fma(u2, c0, f0[2]);
                if (FWD2) {
                    const double c1 = coef[rp + k + lane16];
                    f1[0] = __builtin_fma(u0, c1, f1[0]);
                    f1[1] = __builtin_fma(u1, c1, f1[1]);
                    f1[2] = __builtin_fma(u2, c1, f1[2]);
                }
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                f0[d] = group16_sum(f0[d]);
                if (FWD2) f1[d] = group16_sum(f1[d]);
            }
        }
        double e[3] = {0, 0, 0};
        const double rx = a.ref[pc], ry = a.ref[M + pc], rz = a.ref[2 * M + pc];
        const double mx = a.mean[pc], my = a.mean[M + pc], mz = a.mean[2 * M + pc];
        if (MODE == SWEEP_RHS) {
            e[0] = a.evec[pc];
            e[1] = a.evec[M + pc];
            e[2] = a.evec[2 * M + pc];
        } else if (MODE == SWEEP_RHS_ICP) {
            // the observation of obs_points_kernel (ICP branch), formed here: one launch and one round trip of e less per iteration.
            // Same expressions, so the same e; weight and e are still written out for whoever reads them later.
            const int32_t j = a.icp_idx[pc];
            const bool inside = j >= 0 && (int64_t)j < a.n_targets;  // -1: no finite distance (non-finite fit)
            const int32_t jc = inside ? j : 0;
            const double nanv = __builtin_nan("");
            const double ox = inside ? a.tx[jc] : nanv, oy = inside ? a.ty[jc] : nanv, oz = inside ? a.tz[jc] : nanv;
            const double w = 1.0 / a.state->sigma2;
            const bool off = (a.lm_mask && a.lm_mask[pc]) || w == 0.0;
            const double dx = ox - cen[0] - tr[0], dy = oy - cen[1] - tr[1], dz = oz - cen[2] - tr[2];
            const double ex = R[0] * dx + R[3] * dy + R[6] * dz - (rx - cen[0]) - mx;
            const double ey = R[1] * dx + R[4] * dy + R[7] * dz - (ry - cen[1]) - my;
            const double ez = R[2] * dx + R[5] * dy + R[8] * dz - (rz - cen[2]) - mz;
            e[0] = off ? 0.0 : w * ex;
            e[1] = off ? 0.0 : w * ey;
            e[2] = off ? 0.0 : w * ez;
            if (valid && lane16 == 0) {
                a.weight_out[p] = off ? 0.0 : w;
                a.evec_out[p] = e[0];
                a.evec_out[M + p] = e[1];
                a.evec_out[2 * M + p] = e[2];
            }
        } else if (MODE == SWEEP_PROJ1) {
            // shape - ref' - mean' = R (Q0_i a); projecting back multiplies by R^T: e = Q0_i a
            e[0] = f0[0];
            e[1] = f0[1];
            e[2] = f0[2];
        } else if (MODE == SWEEP_SHAPES) {
            // newshape = R (ref + mean + Q0_i alpha_c - c) + c + t      (transformedModelInit.instance, :222)
            // cur0     = ref + mean + Q0_i alpha                        (model.instance, :224)
            const double ix = rx + mx + f0[0] - cen[0], iy = ry + my + f0[1] - cen[1], iz = rz + mz + f0[2] - cen[2];
            const double nx = R[0] * ix + R[1] * iy + R[2] * iz + cen[0] + tr[0];
            const double ny = R[3] * ix + R[4] * iy + R[5] * iz + cen[1] + tr[1];
            const double nz = R[6] * ix + R[7] * iy + R[8] * iz + cen[2] + tr[2];
            if (valid && lane16 == 0) {
                a.shape_out[p] = nx;
                a.shape_out[M + p] = ny;
                a.shape_out[2 * M + p] = nz;
                const double x0 = rx + mx + f1[0] - a.c0[0], x1 = ry + my + f1[1] - a.c0[1], x2 = rz + mz + f1[2] - a.c0[2];
                const double y0 = nx - a.c0[0], y1 = ny - a.c0[1], y2 = nz - a.c0[2];
                us[0] += x0; us[1] += x1; us[2] += x2;
                us[3] += y0; us[4] += y1; us[5] += y2;
                us[6] += y0 * x0; us[7] += y0 * x1; us[8] += y0 * x2;
                us[9] += y1 * x0; us[10] += y1 * x1; us[11] += y1 * x2;
                us[12] += y2 * x0; us[13] += y2 * x1; us[14] += y2 * x2;
                us[15] += x0 * x0 + x1 * x1 + x2 * x2;
            }
        } else if (MODE == SWEEP_PROJ2) {
            // newshape - (R2 ref + t2) - R2 mean, rotated back by R2^T      (transformedModel.coefficients, :234-237)
            const double sx = a.shape_in[pc] - cen[0] - tr[0], sy = a.shape_in[M + pc] - cen[1] - tr[1],
                         sz = a.shape_in[2 * M + pc] - cen[2] - tr[2];
            e[0] = R[0] * sx + R[3] * sy + R[6] * sz - (rx - cen[0]) - mx;
            e[1] = R[1] * sx + R[4] * sy + R[7] * sz - (ry - cen[1]) - my;
            e[2] = R[2] * sx + R[5] * sy + R[8] * sz - (rz - cen[2]) - mz;
        } else if (MODE == SWEEP_FIT || MODE == SWEEP_POSED) {
            // fit = s * (R (inst - c) + c + t)       ModelFittingParameters.scala:130-143
            const double ix = rx + mx + f0[0] - cen[0], iy = ry + my + f0[1] - cen[1], iz = rz + mz + f0[2] - cen[2];
            const double nx = R[0] * ix + R[1] * iy + R[2] * iz + cen[0] + tr[0];
            const double ny = R[3] * ix + R[4] * iy + R[5] * iz + cen[1] + tr[1];
            const double nz = R[6] * ix + R[7] * iy + R[8] * iz + cen[2] + tr[2];
            if (valid && lane16 == 0) {
                const double s = (MODE == SWEEP_FIT) ? scale : 1.0;
                a.shape_out[p] = s * nx;
                a.shape_out[M + p] = s * ny;
                a.shape_out[2 * M + p] = s * nz;
            }
        }
        if (TRANS) {
            if (!valid) e[0] = e[1] = e[2] = 0.0;
#pragma unroll
            for (int m = 0; m < KMAX; ++m) {
                if (m < km) {
                    const int k = m * 16;
                    acc[m] = __builtin_fma(q0[k], e[0], __builtin_fma(q1[k], e[1], __builtin_fma(q2[k], e[2], acc[m])));
                }
            }
        }
    }
    if (TRANS) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < KMAX; ++m)
            if (m < km) red[grp * rp + m * 16 + lane16] = acc[m];
        __syncthreads();
        for (int k = tid; k < rp; k += kSweepThreads) {
            double s = 0.0;
            for (int g = 0; g < kGroups; ++g) s += red[g * rp + k];
            a.partial[(int64_t)blockIdx.x * rp + k] = s;
        }
    }
    if (MODE == SWEEP_SHAPES) {
        __syncthreads();
        if (lane16 == 0)
            for (int s = 0; s < 16; ++s) red[grp * 16 + s] = us[s];
        __syncthreads();
        if (tid < 24) {
            double s = 0.0;
            if (tid < 16)
                for (int g = 0; g < kGroups; ++g) s += red[g * 16 + tid];
            a.partial[(int64_t)blockIdx.x * 24 + tid] = s;
        }
    }
}

// out[k] = sum over blocks of partial[b][k]: one workgroup per k, fixed summation tree (bitwise reproducible)
__global__ __launch_bounds__(256) void block_partials_reduce_kernel(const double *__restrict__ partial, int nblocks, int width,
                                                                    double *__restrict__ out) {
    __shared__ double sh[256];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(int64_t)b * width + k];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = sh[0];
}

// SWEEP_FIT with quarter boxes (round 4): fit = s (R (ref + mean + Q0 alpha - c) + c + t) as in sweep_kernel<SWEEP_FIT>, but a
// workgroup owns whole 64-point QUARTERS of the fit -- sixteen 16-lane groups x four points each, the basis rows of all four
// requested before the first is used -- and leaves the bounding box of each quarter behind, plus the largest |coordinate - centre|
// of the cloud: what tile_bbox_kernel computed for the column-sum pass of the next iteration in a launch of its own (5 us + a kernel
// boundary per iteration; exact minima / maxima, so the same bits).  KM >= rp / 16.
// S points per 16-lane group in flight (4 for KM <= 8: the whole quarter at once; 1 above: the basis rows of a point are 3 KM values
// per lane, requested eight column blocks at a time -- ranks above 128 keep the quarter-box form with the registers of three waves per
// SIMD instead of falling back to the generic pass + a box launch of its own).
// SEP: the compact basis of a coordinate-separable model (gp.h: gingr_model::Qc) -- coordinate d of a point is the product of its
// kCompactCols-wide row in plane d with the coefficients of class d's columns (KM = kCompactCols / 16)
template <int KM, int S, bool SEP = false>
__global__ __launch_bounds__(kSweepThreads) void sweep_fit_boxes_kernel(SweepArgs a) {
    constexpr int CH = KM < 8 ? KM : 8;  // column blocks per request
    constexpr int ND = SEP ? 3 : 1;      // coefficient sets: one per coordinate class, or the one vector
    static_assert(4 % S == 0, "points per group and round");
    extern __shared__ double lds[];  // [rp] coefficients, then [16][8] box scratch + 8
    const int tid = threadIdx.x, lane16 = tid & 15, grp = tid >> 4;
    const int rp = a.rp, km = SEP ? KM : rp >> 4;
    const int64_t M = a.M;
    const int64_t qstride = SEP ? kCompactCols : rp, dstride = SEP ? compact_plane_doubles(M) : rp;  // point to point, coordinate to coordinate
    const double *basis = SEP ? a.Qc : a.Q0;
    double *coef = lds, *red = lds + rp;
    for (int k = tid; k < rp; k += kSweepThreads) coef[k] = a.coef0[k];
    double R[9], tr[3], cen[3];
    for (int q = 0; q < 9; ++q) R[q] = a.state->R[q];
    for (int q = 0; q < 3; ++q) {
        tr[q] = a.state->t[q];
        cen[q] = a.state->center[q];
    }
    const double scale = a.state->scale;
    double cf[ND][KM];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < ND; ++e)
#pragma unroll
        for (int m = 0; m < KM; ++m) {
            if constexpr (SEP) {
                const int col = a.sep_map[SepMap{rp}.col(e, m * 16 + lane16)];
                cf[e][m] = col >= 0 ? coef[col] : 0.0;
            } else {
                cf[e][m] = m < km ? coef[m * 16 + lane16] : 0.0;
            }
        }
    double amax = 0.0;
    for (int64_t qd = blockIdx.x; qd * 64 < M; qd += gridDim.x) {
        double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
        double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
#pragma unroll
        for (int s0 = 0; s0 < 4; s0 += S) {
            double facc[S][3], rm[S][3];
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int d = 0; d < 3; ++d) facc[s][d] = 0.0;
#pragma unroll
            for (int mc = 0; mc < KM; mc += CH) {
                double u[S][3][CH];
#pragma unroll
                for (int s = 0; s < S; ++s) {  // every load of the round's column blocks in flight
                    const int64_t p = qd * 64 + (s0 + s) * kGroups + grp;
                    const int64_t pc = p < M ? p : 0;
                    const double *q0 = basis + (SEP ? pc : 3 * pc) * qstride + lane16;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
#pragma unroll
                        for (int m = 0; m < CH; ++m) u[s][d][m] = (mc + m < KM && mc + m < km) ? q0[d * dstride + (mc + m) * 16] : 0.0;
                        if (mc == 0) rm[s][d] = a.ref[d * M + pc] + a.mean[d * M + pc];
                    }
                }
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int m = 0; m < CH; ++m)
                            if (mc + m < KM) facc[s][d] = __builtin_fma(u[s][d][m], cf[SEP ? d : 0][mc + m], facc[s][d]);  // (m >= km: 0 * 0)
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int64_t p = qd * 64 + (s0 + s) * kGroups + grp;
                double f[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) f[d] = group16_sum(facc[s][d]);
                // fit = s * (R (inst - c) + c + t)       ModelFittingParameters.scala:130-143
                const double ix = rm[s][0] + f[0] - cen[0], iy = rm[s][1] + f[1] - cen[1], iz = rm[s][2] + f[2] - cen[2];
                const double nx = scale * (R[0] * ix + R[1] * iy + R[2] * iz + cen[0] + tr[0]);
                const double ny = scale * (R[3] * ix + R[4] * iy + R[5] * iz + cen[1] + tr[1]);
                const double nz = scale * (R[6] * ix + R[7] * iy + R[8] * iz + cen[2] + tr[2]);
                if (p < M) {
                    if (lane16 == 0) {
                        a.shape_out[p] = nx;
                        a.shape_out[M + p] = ny;
                        a.shape_out[2 * M + p] = nz;
                    }
                    // (fmin / fmax skip a NaN coordinate: it never widens a box, as in tile_bbox_kernel)
                    lo[0] = fmin(lo[0], nx), lo[1] = fmin(lo[1], ny), lo[2] = fmin(lo[2], nz);
                    hi[0] = fmax(hi[0], nx), hi[1] = fmax(hi[1], ny), hi[2] = fmax(hi[2], nz);
                }
            }
        }
        if (lane16 == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                red[grp * 8 + d] = lo[d];
                red[grp * 8 + 3 + d] = hi[d];
            }
        }
        __syncthreads();
        if (tid < 6) {
            double v = red[tid];
            for (int g = 1; g < kGroups; ++g) v = tid < 3 ? fmin(v, red[g * 8 + tid]) : fmax(v, red[g * 8 + tid]);
            a.qboxes[qd * 6 + tid] = v;
            red[kGroups * 8 + tid] = fabs(v - a.box_centre[tid % 3]);
        }
        __syncthreads();
        if (tid == 0)
            for (int q = 0; q < 6; ++q) amax = fmax(amax, red[kGroups * 8 + q]);
        __syncthreads();  // red is rewritten by the next quarter
    }
    if (tid == 0 && a.absmax_slot) {
        // non-negative doubles order like their bit patterns; only a value above what is already there needs the atomic (the slot was
        // cleared by an EARLIER launch on the stream: post_solve_kernel / state_init_kernel)
        const unsigned long long mb = __builtin_bit_cast(unsigned long long, amax);
        if (mb > __hip_atomic_load(reinterpret_cast<unsigned long long *>(a.absmax_slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(reinterpret_cast<unsigned long long *>(a.absmax_slot), mb);
    }
}

}  // namespace

// =====================================================================================================  launchers
int sweep_num_blocks(int64_t M) {
    const int64_t nb = ceil_div(M, kGroups);
    return (int)(nb < kSweepMaxBlocks ? (nb > 0 ? nb : 1) : kSweepMaxBlocks);
}

int64_t sweep_ws_doubles(int64_t M, int32_t rp) {
    const int w = rp > 24 ? rp : 24;
    return (int64_t)sweep_num_blocks(M) * w;
}

template <int MODE>
static void launch_sweep_mode(gingr_ctx *ctx, const SweepArgs &a, int width) {
    if (MODE == SWEEP_FIT && a.qboxes && a.rp <= 512) {  // one workgroup per 64-point quarter (gp.h: SweepArgs::qboxes)
        const int nq = (int)std::min<int64_t>(4096, ceil_div(a.M, 64));
        const size_t l2 = (size_t)(a.rp + kGroups * 8 + 8) * sizeof(double);
        TimerScope ts(ctx, 4);
        if (a.Qc && a.sep_map)  // (rp <= 112: three kCompactCols-wide rows per point, 36 basis values per thread in flight)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<kCompactCols / 16, 4, true>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 64)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<4, 4>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 112)  // (rank 100: 84 basis values per thread in flight; eight column blocks would spill into AGPRs)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<7, 4>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 128)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<8, 4>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 192)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<12, 1>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 256)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<16, 1>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else if (a.rp <= 384)
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<24, 1>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        else
            hipLaunchKernelGGL((sweep_fit_boxes_kernel<32, 1>), dim3(nq), dim3(kSweepThreads), l2, ctx->stream, a);
        return;
    }
    const int nb = sweep_num_blocks(a.M);
    const size_t lds = (size_t)(2 * a.rp + kGroups * (a.rp > 16 ? a.rp : 16)) * sizeof(double);
    TimerScope ts(ctx, 4);
    if (a.rp <= 128) {
        hipLaunchKernelGGL((sweep_kernel<MODE, 8>), dim3(nb), dim3(kSweepThreads), lds, ctx->stream, a);
    } else {
        if (lds > 48 * 1024)
            set_dynamic_lds(&sweep_kernel<MODE, 32>, (size_t)(lds));
        hipLaunchKernelGGL((sweep_kernel<MODE, 32>), dim3(nb), dim3(kSweepThreads), lds, ctx->stream, a);
    }
    ts.stop();
    if (width > 0 && !a.no_reduce)
        hipLaunchKernelGGL(block_partials_reduce_kernel, dim3((unsigned)width), dim3(256), 0, ctx->stream, a.partial, nb,
                           width, a.out);
}

void launch_sweep(gingr_ctx *ctx, SweepMode mode, const SweepArgs &a) {
    switch (mode) {
        case SWEEP_RHS: launch_sweep_mode<SWEEP_RHS>(ctx, a, a.rp); break;
        case SWEEP_PROJ1: launch_sweep_mode<SWEEP_PROJ1>(ctx, a, a.rp); break;
        case SWEEP_SHAPES: launch_sweep_mode<SWEEP_SHAPES>(ctx, a, 24); break;
        case SWEEP_PROJ2: launch_sweep_mode<SWEEP_PROJ2>(ctx, a, a.rp); break;
        case SWEEP_FIT: launch_sweep_mode<SWEEP_FIT>(ctx, a, 0); break;
        case SWEEP_POSED: launch_sweep_mode<SWEEP_POSED>(ctx, a, 0); break;
        case SWEEP_RHS_ICP: launch_sweep_mode<SWEEP_RHS_ICP>(ctx, a, a.rp); break;
    }
}

void launch_interp_pack(gingr_ctx *ctx, const double *Qs, int32_t rp, const int32_t *inv_src, const int32_t *ids, const double *w,
                        const int32_t *perm_new, int64_t row_begin, int64_t M, double *Q0) {
    const int64_t total = 3 * M * rp;
    hipLaunchKernelGGL(interp_pack_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, Qs, rp, inv_src, ids, w,
                       perm_new, row_begin, M, Q0);
}
void launch_pack_basis(gingr_ctx *ctx, const double *stage_colmajor, const double *variance_dev, int64_t M, int32_t r,
                       int32_t rp, const int32_t *perm, double *Q0) {
    const int64_t total = 3 * M * rp;
    hipLaunchKernelGGL(pack_basis_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, stage_colmajor,
                       variance_dev, 3 * M, r, rp, perm, Q0);
}
