// What the plain-C++ headers (cpd_plan.h, tri_grid_plan.h: compiled for the host alone by the CPU tests) share with the HIP
// translation units: the host / device qualifier and integer rounding.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GINGR_HD __host__ __device__
#else
#define GINGR_HD
#endif

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }
