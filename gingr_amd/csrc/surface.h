// Internal header of the surface family -- surface.hip (closest point), surface_line.hip, surface_self_intersect.hip,
// surface_mesh.hip (normals, boxes, distance statistics), surface_reversal.hip, surface_grid.hip (the target's triangle grid, host side)
// -- and of their callers in the fitter family: the grids' descriptions and the launchers (all async unless noted).
#pragma once
#include <type_traits>

#include "common.h"
#include "tri_grid_plan.h"

constexpr int kTriTile = 256;  // triangles per bounding box of the tile scans (four 64-triangle quarters)
#ifndef GINGR_TRI_GRID_CELLS
#define GINGR_TRI_GRID_CELLS 64
#endif
constexpr int kTriGridMaxCells = GINGR_TRI_GRID_CELLS;  // rows of cells (+ the short list) a grid query's ball may cover; more: the tile scan

// tri: [3*T] vertex POSITIONS in the cloud `v`, in a spatial triangle order; boxes: one {lo, hi} per 256 triangles
void launch_cell_normals(gingr_ctx *ctx, Cloud v, const int32_t *tri, int64_t T, double *cn_soa);
void launch_vertex_normals(gingr_ctx *ctx, const int32_t *adj_ptr, const int32_t *adj_tri, const double *cn_soa, int64_t T,
                           int64_t n, double *vn_soa);
void launch_tri_tile_bbox(gingr_ctx *ctx, Cloud v, const int32_t *tri, int64_t T, double *boxes, double *tribox = nullptr, double *cell_normals = nullptr);
// closest point of the triangle soup to every query (SoA out); exact ties: lowest tri_orig
// mask / nmask (nullable, device): only queries with mask[i] != 0 are answered and the launch is a no-op when *nmask == 0 (what
// launch_surface_cp_grid leaves behind: TriGrid::flag, TriGrid::cur_nflag())
void launch_surface_closest_point(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri, const int32_t *tri_orig, int64_t T,
                                  const double *boxes, double *cp_soa, double *d2, int32_t *tri_out = nullptr, int32_t *warm = nullptr,
                                  bool warm_valid = false, const double *tribox = nullptr, const uint8_t *mask = nullptr,
                                  const int32_t *nmask = nullptr);
// uniform grid over the (fixed) triangles of a mesh: cell -> triangles whose box overlaps it (tri_grid_plan.h, surface_grid.hip)
struct TriGridDev {
    double lo[3];
    double h, inv_h;
    int32_t g[3];
    int32_t span[3];            // largest extent (in cell steps) of a listed triangle's box per axis
    int32_t n_listed, n_big;    // entries [0, n_listed) are listed by cell, [n_listed, n_listed + n_big) is the short list of wide triangles
    const int32_t *cell_start;  // [g0 g1 g2 + 1], x fastest: a triangle is listed in the cell of its box's lower corner
    const double *boxes;        // [entries][6]: box lo / hi of every entry
    const double *recs;         // [entries][10]: corners A, B, C, {position | original index << 32} (tri_grid_plan.h: kTriRec)
};
struct TriGrid {
    TriGridDev v{};
    int32_t *cell_start = nullptr;
    double *boxes = nullptr, *recs = nullptr;
    uint8_t *flag = nullptr;   // [max_queries]: queries the grid search could not certify
    int32_t *nflag = nullptr;  // two counters used alternately (as NNGrid)
    int parity = 0;
    int64_t max_queries = 0, list_entries = 0;
    bool ready = false;
    const int32_t *cur_nflag() const { return nflag + parity; }
};
// The same grid for a MOVING mesh (the template), rebuilt on the device in front of every use (round 5): the description lives in
// device memory (params: the TriGridDev the kernels read, + validity), geometry and lists are recomputed from the per-triangle boxes
// the iteration has computed anyway (tri_tile_bbox_kernel).  Four short launches: set-up (bounding box of the tile boxes, grid
// dimensions at the fixed cell edge h, counters zeroed), count (cell of every triangle's lower corner, wide triangles to the short
// list), scan (128 workgroups with a look-back over their totals, up to 2^20 cells), fill (entries, boxes and corner records in cell order).  Entry order inside a cell
// is whatever the atomics give: the queries' results do not depend on it (self-intersection is an OR; closest points break ties by
// original triangle id).
struct MovGridParams {
    TriGridDev v;
    int32_t valid, pad;
};
struct MovGrid {
    MovGridParams *params = nullptr;  // device
    int32_t *cell_cnt = nullptr, *cell_start = nullptr, *tri_cell = nullptr, *big = nullptr;
    double *boxes = nullptr, *recs = nullptr;
    uint8_t *flag = nullptr;          // [max_queries]: queries the grid could not certify
    int32_t *nflag = nullptr;         // two counters used alternately (as TriGrid)
    unsigned long long *scan_agg = nullptr;  // per scan workgroup: (epoch << 32 | total) of the build in flight
    unsigned epoch = 0;
    int parity = 0;
    int32_t ncap = 0;                 // cells allocated
    int64_t T = 0, max_queries = 0;
    double h = 0.0;                   // cell edge (mean extent of a triangle's box when the grid was set up; any value is correct)
    bool ready = false;
    const int32_t *cur_nflag() const { return nflag + parity; }
};
int mov_grid_alloc(gingr_ctx *ctx, int64_t T, int64_t max_queries, MovGrid *g);
void mov_grid_free(MovGrid *g);
// (re)build for the current vertex positions; tribox [T][6] and tile_boxes [ceil(T / 256)][6] as tri_tile_bbox_kernel left them
void launch_mov_grid_build(gingr_ctx *ctx, MovGrid &g, Cloud v, const int32_t *tri, const int32_t *tri_orig, const double *tribox,
                           const double *tile_boxes);
// self-intersection flags (see launch_self_intersect) over the moving grid: certified queries get their flag, the others are marked
// in g.flag / counted in g.cur_nflag() for the masked launch_self_intersect that must follow
void launch_self_intersect_grid(gingr_ctx *ctx, Cloud fit, const double *cp_soa, MovGrid &g, const int32_t *skip, int32_t *flag);
int tri_grid_build(gingr_ctx *ctx, const double *vsoa_host, int64_t n, const int32_t *tri_host, const int32_t *tri_orig_host, int64_t T,
                   int64_t max_queries, TriGrid *g);
void tri_grid_free(TriGrid *g);
void launch_surface_cp_grid(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri, const int32_t *tri_orig, int64_t T, TriGrid &g,
                            double *cp_soa, double *d2, int32_t *tri_out, int32_t *warm);
// bary[3 i + k] = weight of corner k of triangle tri_id[i] at the closest point of that triangle to query i; tri_by_orig [3 T]:
// corner positions in the cloud v, indexed by ORIGINAL triangle number
void launch_barycentric(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri_by_orig, const int32_t *tri_id, double *bary);
// out4 = {sum of sqrt(d2), max, count, sum of log N(sqrt(d2); 0, sdev)} over the counted points (surface_mesh.hip)
int distance_stats_ws_doubles();
void launch_distance_stats(gingr_ctx *ctx, int64_t n, const double *d2, const int32_t *orig, int64_t orig_limit, const int32_t *nn,
                           const int32_t *boundary, double sdev, double *partial, double *out4);
// What the self-intersection launch can take over from the launches around it (both are one value per query, computed where the query
// is held anyway):  nn_vertex != nullptr -- the first two rejection tests of launch_surface_prereject are made in the prologue (pre_out
// is written, `skip` is not read);  w01 != nullptr -- launch_surface_weight's outputs are written in the epilogue.
struct SelfIntersectFuse {
    const int32_t *nn_vertex = nullptr, *boundary = nullptr, *found = nullptr;
    const double *q_vn = nullptr, *t_vn = nullptr;  // vertex normals of the queries' mesh [3][n] and of the other mesh [3][Nt]
    int64_t Nt = 0;
    int32_t *pre_out = nullptr;
    const double *sigma2 = nullptr;
    double *w01 = nullptr, *weight_in = nullptr;
};
// mesh (nullable): the cloud the triangles index when it is not the query cloud itself (row shard: the gathered fit of all shards)
// only / nonly (nullable, device): only queries with only[i] != 0 are processed and written, and the launch is a no-op when *nonly == 0
void launch_self_intersect(gingr_ctx *ctx, Cloud fit, const double *cp_soa, const int32_t *tri, int64_t T, const double *boxes,
                           const int32_t *skip, int32_t *flag, const double *tribox = nullptr, const Cloud *mesh = nullptr,
                           const uint8_t *only = nullptr, const int32_t *nonly = nullptr, const SelfIntersectFuse *fuse = nullptr);
// found (nullable): along-normal flavour, 0 = no intersection (rejected)
void launch_surface_prereject(gingr_ctx *ctx, int64_t M, const int32_t *nn_vertex, const int32_t *tgt_boundary,
                              const double *fit_vn, const double *tgt_vn, int64_t N, const int32_t *found, int32_t *pre);
// nearest intersection (!= the vertex) of the line through every fit vertex along dirs with the mesh; cp = the vertex, found = 0 if none
void launch_line_nearest(gingr_ctx *ctx, Cloud fit, const double *dirs_soa, Cloud v, const int32_t *tri, const int32_t *tri_orig,
                         int64_t T, double *boxes, double *cp_soa, int32_t *found);
// the same over the triangle grid of the mesh (static meshes: the target of the forward direction)
void launch_line_nearest_grid(gingr_ctx *ctx, Cloud fit, const double *dirs_soa, const TriGrid &g, double *cp_soa, int32_t *found);
void launch_surface_weight(gingr_ctx *ctx, int64_t M, const int32_t *pre, const int32_t *hit, const double *sigma2_dev, double *w01,
                           double *weight_in);

// reversed correspondence direction: from (nearest template vertex, rejection flags) per TARGET vertex to one observation per
// template vertex (mean of the accepted targets that map to it, weight = count / sigma2); w01_targets (nullable) gets 0 / 1 per target
size_t reversal_sort_temp_bytes(int64_t N);
void launch_reversal_observations(gingr_ctx *ctx, int64_t M, Cloud tgt, const int32_t *nn_vertex, const int32_t *pre,
                                  const int32_t *hit, const double *sigma2_dev, int32_t *keys, int32_t *vals, int32_t *skeys,
                                  int32_t *svals, void *sort_temp, size_t sort_temp_bytes, double *w01_targets, double *obs_soa,
                                  double *weight_in);

// the same for a RANGE of the target queries (tgt = that range), left as sums: sums4 [4][M] = {sum x, sum y, sum z, count} per
// template vertex (a row shard's contribution to the all-reduce of the reversed direction); tgt.n may be 0
void launch_reversal_sums(gingr_ctx *ctx, int64_t M, Cloud tgt, const int32_t *nn_vertex, const int32_t *pre, const int32_t *hit,
                          int32_t *keys, int32_t *vals, int32_t *skeys, int32_t *svals, void *sort_temp, size_t sort_temp_bytes,
                          double *w01_targets, double *sums4);

// spatial (k-d leaf) orders of a stateless mesh query on the host (fitter_surface.hip): queries and vertices (device position ->
// original index; vinv: original -> position), triangles by centroid (torder), and `tri` [3 T]: their vertex POSITIONS in that order
void mesh_orders(int64_t n_points, const double *points, int64_t n_vertices, const double *vertices, int64_t n_triangles,
                 const int32_t *triangles, std::vector<int32_t> &qorder, std::vector<int32_t> &vorder, std::vector<int32_t> &torder,
                 std::vector<int32_t> &vinv, std::vector<int32_t> &tri);

// copies of every query held per workgroup of the tile scans (surface_cp_queue_kernel, self_intersect_queue_kernel), from the number of queries
inline int surface_h(int64_t nq) {
    // measured (femur chain, 1 622 queries x 3 240 triangles: 1 007 / 1 151 / 1 237 / 1 257 steps per second at H = 2 / 4 / 8 / 16;
    // 41k queries x 82k triangles: 1 452 / 1 470 / 1 441 / 1 275 iterations per second): small meshes want many short workgroups
    return nq <= 4096 ? 16 : (nq <= 16384 ? 8 : 4);
}
// go(std::integral_constant<int, H>{}) for the H the tile-scan kernels are instantiated at: 8, 16, and 4 for every other value
template <typename F>
inline void with_surface_h(int h, F &&go) {
    if (h == 8) return go(std::integral_constant<int, 8>{});
    if (h == 16) return go(std::integral_constant<int, 16>{});
    go(std::integral_constant<int, 4>{});
}
