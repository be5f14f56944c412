// The kernel warp (kernel_warp.hip) for the two handle types that use it, classic_cpd.hip and bcpd.hip.  Internal to libgingr_hip.so.
#pragma once

#include "common.h"

// The buffers of the pass, kept by the handle across calls (grown on demand, never shrunk): the staging buffer and the planes of a
// slab of queries, the chunk partials, and aux = {largest |coordinate| of the slab, of the centres}.
struct KernelWarpWork {
    DevBuf stage, Z, part, aux;
    bool centres_measured = false;
};

// out_p = A (z_p + sum_m g(z_p, y_m) c_m) + t for the P host points `points_xyz` into `out_xyz` (both [3 P] interleaved; they may be
// the same array), g(a, b) = exp(-|a - b|^2 / (2 beta^2)).  Y: the M centres; coeff: three planes of stride coeff_stride >= M;
// both ignored with no_sum.  params13 (device; nullable: A = I, t = 0) = {s, L row-major, t}: A = s L.  Synchronises.
int kernel_warp_points(gingr_ctx *ctx, KernelWarpWork &work, Cloud Y, const double *coeff, int64_t coeff_stride, double beta,
                       const double *params13, bool no_sum, int64_t P, const double *points_xyz, double *out_xyz);
