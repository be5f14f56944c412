// The value of one scalar kernel of a GPMM build (gpmm_factor.h: KSpec) between two points given by their coordinates: what the pivoted
// Cholesky evaluates on the reference (gpmm.hip) and the kernel extension evaluates off it (model_extend.hip).  One copy, so that a
// model's own vertices get the bits of the build: unfused |x-y|^2, multiply-then-add dot products, the table exponential of fastexp.h.
// (c.) is the non-pivot argument -- the one the mirrored copy mirrors -- and (p.) the pivot.  Device code only.
#pragma once

#include "fastexp.h"
#include "gpmm_factor.h"

namespace gpmm_factor {

__device__ __forceinline__ double mixture_value(const Mixture &mix, double d2, const double *T) {
    double v = 0.0;
    for (int i = 0; i < mix.n; ++i) {
        const double e = mix.s[i] * fastexp2_scaled<3>(fastexp_clamp_d2(d2, fastexp_d2_limit(mix.c[i])), mix.c[i], T);
        v = i == 0 ? e : v + e;
    }
    return v;
}

// kinds 0 (Gaussian mixture, optionally with its x-mirrored copy) and 1 (dot product); a lookup kernel (kind 2) has no value off its table
__device__ __forceinline__ double kspec_value_xyz(const KSpec &k, double cx, double cy, double cz, double px, double py, double pz,
                                                  const double *T) {
    if (k.kind == 1) {
        const double dot = __dadd_rn(__dadd_rn(__dmul_rn(cx, px), __dmul_rn(cy, py)), __dmul_rn(cz, pz));
        return __dmul_rn(dot, k.scale);
    }
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    double v = mixture_value(k.mix, d2, T);
    if (k.mirror != 0.0) {
        const double mx = __dmul_rn(cx, -1.0) - px;
        const double m2 = __dadd_rn(__dadd_rn(__dmul_rn(mx, mx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        v = __dadd_rn(v, __dmul_rn(mixture_value(k.mix, m2, T), k.mirror));
    }
    return v;
}

// f_t(nn) of one radial term (gingr_gpmm_build_radial): the Gaussian through the table exponential exactly as mixture_value has it; the
// other two as the reference writes them (KernelHelper.scala:53-73), IEEE division and square root, par = beta * beta
__device__ __forceinline__ double radial_family_value(int32_t family, double par, double nn, const double *T) {
    if (family == GINGR_RADIAL_RATIONAL_QUADRATIC) return __dsub_rn(1.0, __ddiv_rn(nn, __dadd_rn(nn, par)));
    if (family == GINGR_RADIAL_INVERSE_MULTIQUADRIC) return __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(nn, par)));
    return fastexp2_scaled<3>(fastexp_clamp_d2(nn, fastexp_d2_limit(par)), par, T);
}

// sum_t scaling_t f_t(|c - p|^2) of radial terms WITHOUT weight fields, terms added left to right as radial_value (gpmm.hip) adds them;
// family[t] by value (the extension keeps the table on the host side of the launch)
__device__ __forceinline__ double radial_value_xyz(const Mixture &mix, const int32_t *family, double cx, double cy, double cz, double px,
                                                   double py, double pz, const double *T) {
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double nn = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    double v = 0.0;
    for (int i = 0; i < mix.n; ++i) {
        const double e = __dmul_rn(mix.s[i], radial_family_value(family[i], mix.c[i], nn, T));
        v = i == 0 ? e : __dadd_rn(v, e);
    }
    return v;
}

}  // namespace gpmm_factor
