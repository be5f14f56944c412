// Planning of the surface-distance metrics (surface_metrics.hip): the seed triangle of every vertex, the cut of the query sets into
// column blocks, of the meshes into launch chunks and of the queries into slabs, and the layout of the partials the batched scan leaves.
// Plain C++ (compiled for the host alone by tests/test_surface_metrics_host.py).
//
// Pairs.  A launch covers a block of at most kMaxBlockCols query sets (the column block of model_metrics_plan.h) and a chunk of at most
// kMeshChunk meshes.  pairing 0 (all): every set of the block against every mesh of the chunk, pair = set * meshes + mesh; pairing 1
// (cyclic): set c of the whole call against mesh c % n_meshes, one pair per set, one chunk that holds every mesh.
// Queries.  The points of a set are cut into slabs of whole kGroupQueries-query groups; a workgroup takes one (slab, pair), walks the
// slab's groups in ascending order and leaves ONE (sum, max) partial: partial[(slab * pairs + pair) * 2 + {0, 1}].  The finish adds the
// slabs in ascending order, so the sums depend on the number of points, sets and meshes alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "model_metrics_plan.h"

namespace surface_metrics_plan {

constexpr int64_t kGroupQueries = 16;                     // queries a workgroup holds at a time (64 lanes / 4 copies of each query)
constexpr int64_t kMeshChunk = 4096;                      // meshes of a launch (grid z)
constexpr int64_t kPairTarget = 8192;                     // workgroups a launch aims at
constexpr int64_t kMaxPartialDoubles = (int64_t)1 << 24;  // the partials of a launch at most (128 MB)
constexpr int64_t kMaxTriangles = (int64_t)1 << 26;       // a queue entry keeps the triangle's position in 26 bits (WaveQueue)

// seed[v] = the lowest-numbered triangle that has vertex v as a corner, -1 for a vertex of no triangle.  triangles: [3 T], ids in
// [0, n_vertices).
inline void seed_triangles(int64_t n_vertices, int64_t n_triangles, const int32_t *triangles, std::vector<int32_t> &seed) {
    seed.assign((size_t)n_vertices, -1);
    for (int64_t t = n_triangles - 1; t >= 0; --t)
        for (int k = 0; k < 3; ++k) seed[(size_t)triangles[3 * t + k]] = (int32_t)t;
}

// meshes in chunks of at most kMeshChunk (pairing 0); pairing 1 keeps every mesh in one chunk -- the grid does not run over meshes
struct MeshChunks {
    int64_t n = 0, count = 0, size = 0;
    int64_t begin(int64_t c) const { return c * size; }
    int64_t length(int64_t c) const { return (c + 1) * size < n ? size : n - c * size; }
};
inline MeshChunks mesh_chunks(int64_t n_meshes, int pairing) {
    MeshChunks c;
    c.n = n_meshes;
    c.size = pairing == 0 ? kMeshChunk : (n_meshes > 0 ? n_meshes : 1);
    c.count = n_meshes > 0 ? ceil_div(n_meshes, c.size) : 0;
    return c;
}

// one launch: `sets` query sets of `points` points against `meshes` meshes of a chunk
struct PairPlan {
    int64_t points = 0, sets = 0, meshes = 0;
    int pairing = 0;
    int64_t pairs = 0, per_slab = 0, slabs = 0;
    int64_t slab_begin(int64_t s) const { return s * per_slab; }
    int64_t slab_end(int64_t s) const { return (s + 1) * per_slab < points ? (s + 1) * per_slab : points; }
    int64_t pair(int64_t set, int64_t mesh) const { return pairing == 0 ? set * meshes + mesh : set; }
    int64_t partial_index(int64_t slab, int64_t pr, int which) const { return (slab * pairs + pr) * 2 + which; }
    int64_t partial_doubles() const { return slabs * pairs * 2; }
    int64_t workgroups() const { return slabs * pairs; }
};
// the mesh (index in the whole call) that set `set_global` meets under pairing 1
inline int64_t cyclic_mesh(int64_t set_global, int64_t n_meshes) { return set_global % n_meshes; }

inline PairPlan make_pair_plan(int64_t points, int64_t sets, int64_t meshes, int pairing) {
    PairPlan p;
    p.points = points, p.sets = sets, p.meshes = meshes, p.pairing = pairing;
    p.pairs = pairing == 0 ? sets * meshes : sets;
    const int64_t pairs = p.pairs > 0 ? p.pairs : 1;
    int64_t want = ceil_div(kPairTarget, pairs);
    const int64_t fit = kMaxPartialDoubles / (2 * pairs);
    if (want > fit) want = fit;
    const int64_t most = ceil_div(points, kGroupQueries);
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.per_slab = round_up(ceil_div(points, want), kGroupQueries);
    p.slabs = ceil_div(points, p.per_slab);
    return p;
}

// bytes on the device of a call's working set: every mesh as three planes with its tile and quarter boxes, a block of query sets as
// planes, the block of instance columns they are transposed from (model routes: model_rows = 3 M + 48, else 0), the partials
inline int64_t working_set_bytes(int64_t n_points, int64_t block_sets, int64_t n_vertices, int64_t n_meshes, int64_t n_triangles,
                                 int64_t model_rows) {
    const int64_t tiles = ceil_div(n_triangles, 256);
    int64_t doubles = n_meshes * (3 * n_vertices + 30 * tiles) + block_sets * 3 * n_points + kMaxPartialDoubles;
    doubles += model_rows * model_metrics_plan::padded_cols(block_sets);
    return doubles * 8 + (3 * n_triangles + n_points) * 4;
}

}  // namespace surface_metrics_plan
