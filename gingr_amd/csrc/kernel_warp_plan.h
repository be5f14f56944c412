// Planning of the kernel warp (kernel_warp.hip): out_p = A (z_p + sum_m g(z_p, y_m) c_m) + t for P query points over M centres.
// Plain C++ (compiled for the host alone by tests/test_kernel_warp_host.py).
//
// The centres are cut into chunks of kChunkLength (whole 256-centre tiles; the last chunk may be shorter): one workgroup takes the
// 256 queries of a tile through one chunk and leaves three partial sums per query, and the finish kernel adds a query's partials in
// chunk order.  The chunk boundaries depend on M alone, so the order in which a query's sum is taken does not depend on P or on the
// other queries of the call.  The queries go through the device in slabs: a slab is what is uploaded, warped and downloaded at a
// time, and its length only bounds the buffers -- the partials [chunk][3][slab], the staging buffer and the planes of the slab.
#pragma once

#include "host_device.h"

namespace kernel_warp_plan {

constexpr int64_t kTile = 256;                   // queries per workgroup = centres staged in LDS at a time
constexpr int64_t kChunkTiles = 8;
constexpr int64_t kChunkLength = kTile * kChunkTiles;
constexpr int64_t kMaxSlab = (int64_t)1 << 20;   // queries per slab at most (24 MB of staging, as much again for the planes)
constexpr int64_t kMaxPartialDoubles = (int64_t)1 << 24;  // the partials of a slab at most (128 MB), unless one tile of queries needs more
constexpr int64_t kMaxChunks = 65535;            // gridDim.y

struct Plan {
    int64_t P = 0, M = 0;  // M = 0: no sum (the rigid and affine kinds)
    int64_t chunks = 0, chunk_length = kChunkLength, slab_length = 0, slabs = 0;

    int64_t chunk_begin(int64_t c) const { return c * chunk_length; }
    int64_t chunk_end(int64_t c) const { return (c + 1) * chunk_length < M ? (c + 1) * chunk_length : M; }
    int64_t slab_begin(int64_t s) const { return s * slab_length; }
    int64_t slab_count(int64_t s) const { return (s + 1) * slab_length < P ? slab_length : P - s * slab_length; }
    int64_t grid_x(int64_t s) const { return ceil_div(slab_count(s), kTile); }
    int64_t grid_y() const { return chunks; }
    int64_t partial_doubles() const { return chunks * 3 * slab_length; }
    int64_t cloud_doubles() const { return 3 * slab_length; }  // the staging buffer, and the planes of the slab
    int64_t workspace_bytes() const { return (partial_doubles() + 2 * cloud_doubles()) * (int64_t)sizeof(double); }
};

inline Plan make_plan(int64_t P, int64_t M) {
    Plan p;
    p.P = P;
    p.M = M;
    p.chunks = ceil_div(M, kChunkLength);
    int64_t cap = kMaxSlab;
    if (p.chunks > 0) {
        const int64_t fit = kMaxPartialDoubles / (3 * p.chunks) / kTile * kTile;  // whole tiles of queries
        if (fit < cap) cap = fit;
        if (cap < kTile) cap = kTile;
    }
    p.slab_length = P < cap ? P : cap;  // one slab holds all of a small call; otherwise whole tiles
    p.slabs = P > 0 ? ceil_div(P, p.slab_length) : 0;
    return p;
}

}  // namespace kernel_warp_plan
