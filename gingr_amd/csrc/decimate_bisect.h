// The scalar side of the vertex-clustering decimation (mesh_decimate.hip): the cube-size bisection and the packing of a cell into
// one 64-bit key.  One home for both, compiled for the device (the control block's step kernel) and for the host
// (tests/c/decimate_bisect_driver.cpp feeds it count sequences).  All of it is IEEE double, no contraction; it restates
// gingr_amd/simple.py: cluster_decimate line by line:
//     extent = max(v.max(0) - v.min(0)) or 1.0;  lo, hi = extent * 1e-6, extent * 2.0
//     up to 60 times:  mid = sqrt(lo * hi);  k = distinct cells at mid;  k >= n_target ? (accept mid; lo = mid) : hi = mid;
//                      stop once hi / lo < 1.0005
//     h = the last accepted mid, else lo
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GINGR_HD __host__ __device__
#else
#define GINGR_HD
#endif

#define GINGR_DECIMATE_MAX_STEPS 60

struct DecimateBisect {
    double lo, hi, mid;  // mid: the cube size the NEXT count is wanted for (meaningless once done)
    double h;            // the chosen cube size (valid once done)
    int32_t steps, done, accepted, pad;
};

GINGR_HD inline double decimate_extent(double ex, double ey, double ez) {
    double e = ex > ey ? ex : ey;
    e = e > ez ? e : ez;
    return e == 0.0 ? 1.0 : e;
}

GINGR_HD inline void decimate_bisect_init(DecimateBisect *b, double extent) {
    b->lo = extent * 1e-6;
    b->hi = extent * 2.0;
    b->mid = sqrt(b->lo * b->hi);
    b->h = b->lo;
    b->steps = 0;
    b->done = 0;
    b->accepted = 0;
    b->pad = 0;
}

// `count` = distinct cells at b->mid
GINGR_HD inline void decimate_bisect_step(DecimateBisect *b, int64_t count, int64_t n_target) {
    if (b->done) return;
    if (count >= n_target) {
        b->accepted = 1;
        b->h = b->mid;
        b->lo = b->mid;
    } else {
        b->hi = b->mid;
    }
    b->steps += 1;
    if (b->hi / b->lo < 1.0005 || b->steps >= GINGR_DECIMATE_MAX_STEPS) {
        b->done = 1;
        if (!b->accepted) b->h = b->lo;
    } else {
        b->mid = sqrt(b->lo * b->hi);
    }
}

// cell = floor((x - lo_corner) / h) per axis (a true division), 21 bits per axis: h >= 1e-6 extent keeps every index <= 1e6 < 2^20.
// The top bit stays clear, so no key equals the table's empty mark (all ones).
#define GINGR_DECIMATE_AXIS_BITS 21
GINGR_HD inline uint64_t decimate_cell_key(double x, double y, double z, double lx, double ly, double lz, double h) {
    const uint64_t m = ((uint64_t)1 << GINGR_DECIMATE_AXIS_BITS) - 1;
    const uint64_t cx = (uint64_t)(int64_t)floor((x - lx) / h) & m;
    const uint64_t cy = (uint64_t)(int64_t)floor((y - ly) / h) & m;
    const uint64_t cz = (uint64_t)(int64_t)floor((z - lz) / h) & m;
    return cx | (cy << GINGR_DECIMATE_AXIS_BITS) | (cz << (2 * GINGR_DECIMATE_AXIS_BITS));
}
