// Device helpers every spatially pruned kernel shares (cpd_pairs.hip, nn_scan.hip, nn_grid.hip, cloud_ops.hip, surface*.hip): the
// staged point record, wave-uniform axis-aligned boxes and the separately rounded squared distance.  ONE body each, inlined.
#pragma once
#include <hip/hip_runtime.h>

namespace {  // (one private copy per translation unit, like the kernels that use it)

struct __attribute__((aligned(32))) P4 {
    double x, y, z, w;
};

// The box arrays in memory are records of six doubles, {lo[3], hi[3]}: the same layout.
struct Box {
    double lo[3], hi[3];
};

// v of the first active lane as a wave-uniform value (two scalar registers)
__device__ __forceinline__ double uniform_d(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// wave-wide bounding box of the valid lanes' points, wave-uniform
__device__ __forceinline__ Box wave_box(bool ok, double qx, double qy, double qz) {
    double lo[3] = {ok ? qx : __builtin_huge_val(), ok ? qy : __builtin_huge_val(), ok ? qz : __builtin_huge_val()};
    double hi[3] = {ok ? qx : -__builtin_huge_val(), ok ? qy : -__builtin_huge_val(), ok ? qz : -__builtin_huge_val()};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
        }
    Box b;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        b.lo[d] = uniform_d(lo[d]);
        b.hi[d] = uniform_d(hi[d]);
    }
    return b;
}

// squared gap between two boxes (0 when they meet; NaN when a bound is NaN: callers never prune on NaN)
__device__ __forceinline__ double box_gap2(const Box &a, const double *__restrict__ b /* lo[3], hi[3] */) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double g = fmax(fmax(a.lo[d] - b[3 + d], b[d] - a.hi[d]), 0.0);
        s = __builtin_fma(g, g, s);
    }
    return s;
}

// Squared distance with separately rounded multiplies and adds (no FMA contraction), so that d2 is bit-identical to the reference
// expression dx*dx + dy*dy + dz*dz evaluated in float64 on a CPU; the argmin of every closest-point search is then index-exact.
__device__ __forceinline__ double norm2_exact(double dx, double dy, double dz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

}  // namespace
