// What the kernels of the classic family (classic_cpd.hip, classic_cpd_lowrank.hip, bcpd.hip, rigid_icp.hip) share, one body each: the
// sum over sixteen lanes, a row of a dense matrix against three planes, per-thread sums -> block partials -> their fixed-order total,
// and the similarity transform of a point.  Every sum adds in one fixed order: the same bits on every run.
#pragma once
#include "block_sum.h"
#include "host_device.h"

namespace {

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= kDblMax; }

// the sum over the caller's group of 16 lanes, in every lane of it: the butterfly 8, 4, 2, 1
__device__ __forceinline__ double sum16(double v) {
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// acc[d] = sum_i row[i] f[i] in[d stride + i] over begin <= i < end (f == nullptr: 1), lane16 taking i = begin + lane16, + 16, ...;
// valid in every lane of the group.  A group without a row passes end <= begin.
__device__ __forceinline__ void row_dot3(const double *__restrict__ row, int64_t begin, int64_t end, int lane16, const double *__restrict__ in,
                                         int64_t stride, const double *__restrict__ f, double acc[3]) {
    acc[0] = acc[1] = acc[2] = 0.0;
    for (int64_t i = begin + lane16; i < end; i += 16) {
        const double g = f ? row[i] * f[i] : row[i];
        acc[0] = __builtin_fma(g, in[i], acc[0]);
        acc[1] = __builtin_fma(g, in[stride + i], acc[1]);
        acc[2] = __builtin_fma(g, in[2 * stride + i], acc[2]);
    }
    for (int d = 0; d < 3; ++d) acc[d] = sum16(acc[d]);
}

// out_row[q] = the sum of a[q] over the 256 threads of the workgroup, q < K (sh: 256 doubles)
template <int K>
__device__ __forceinline__ void block_sums(const double *a, double *sh, double *__restrict__ out_row) {
    for (int q = 0; q < K; ++q) {
        __syncthreads();  // sh is reused by every pass
        const double t = block_sum<256>(a[q], sh);
        if (threadIdx.x == 0) out_row[q] = t;
    }
}

// entry q of the K-wide rows block_sums left, added up over the blocks in block order
__device__ __forceinline__ double sum_partials(const double *__restrict__ partial, int nblocks, int K, int q) {
    double v = 0.0;
    for (int b = 0; b < nblocks; ++b) v += partial[b * K + q];
    return v;
}

// out = s L p + t from params13 = {s, L row-major, t}
__device__ __forceinline__ void similarity_apply(const double *__restrict__ params13, double x, double y, double z, double out[3]) {
    const double s = params13[0], *L = params13 + 1, *t = params13 + 10;
    for (int d = 0; d < 3; ++d) out[d] = s * ((L[3 * d] * x + L[3 * d + 1] * y) + L[3 * d + 2] * z) + t[d];
}

}  // namespace
