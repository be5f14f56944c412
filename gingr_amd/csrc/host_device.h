// What the plain-C++ headers (cpd_plan.h, tri_grid_plan.h: compiled for the host alone by the CPU tests) share with the HIP
// translation units: the host / device qualifier, integer rounding, the largest finite double and the 3 x 3 determinant.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GINGR_HD __host__ __device__
#else
#define GINGR_HD
#endif

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

constexpr double kDblMax = 1.79769313486231570815e308;  // |x| <= kDblMax: x is finite (false for a NaN)

// determinant of a row-major 3 x 3 matrix, by the first row
GINGR_HD inline double det3(const double *m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
