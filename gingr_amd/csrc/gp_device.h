// Device helpers shared by the low-rank GP kernels (gp*.hip, solve_blocks.h).  Internal to libgingr_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

typedef double v4f64 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// sum over the caller's 16-lane group, the same bits in every lane: the butterfly 8, 4, 2, 1.  Round 4: on the DPP crossbar (row
// rotations) instead of __shfl_xor, which goes through ds_bpermute (~100 cycles per step; twelve of these sums sit on the critical
// path of a one-wave-per-SIMD launch like the fit pass of a small model).  Bit-identical to the shuffle butterfly: after the step
// with distance 2d every lane holds the same bits as the lane 2d away, so the lane d "behind" (what a rotation delivers) holds
// exactly what the xor partner holds, and a + b = b + a.
__device__ __forceinline__ double group16_sum(double v) {
    auto step = [&](auto ctrl) {
        constexpr int c = decltype(ctrl)::value;
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, c, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), c, 0xf, 0xf, false);
        v += __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    };
    step(std::integral_constant<int, 0x128>{});  // row_ror:8
    step(std::integral_constant<int, 0x124>{});  // row_ror:4
    step(std::integral_constant<int, 0x122>{});  // row_ror:2
    step(std::integral_constant<int, 0x121>{});  // row_ror:1
    return v;
}

// compile-time loop: f(std::integral_constant<int, I>) for I = BEGIN .. END-1 (DPP controls must be immediates)
template <int BEGIN, int END, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (BEGIN < END) {
        f(std::integral_constant<int, BEGIN>{});
        static_for<BEGIN + 1, END>(f);
    }
}
