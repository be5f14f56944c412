// Block-wide fixed-order sum of one double per thread (the reductions of cpd_pairs.hip, cloud_ops.hip and cloud_sums.h).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// result valid in every thread after the last barrier (callers read it in thread 0).  NT = blockDim.x, sh: NT doubles.  The first
// thing it does is write sh: a caller that reuses sh back to back (or read it last in other threads) puts a __syncthreads() in front.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace
