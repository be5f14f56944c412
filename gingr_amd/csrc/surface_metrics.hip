// Surface-distance model metrics (C ABI in include/gingr_hip.h: gingr_mesh_set_distances, gingr_model_generalization_surface,
// gingr_model_specificity_surface): the mean and the largest distance from every point of many query sets to the closest point on the
// surface of many meshes that share ONE triangulation, in one batched pass.
//   topology   the k-d leaf order of the FIRST mesh's vertices and triangle centroids (mesh_orders), the triangles as vertex positions in
//              that order, and one seed triangle per query (the lowest-numbered triangle at the query's own vertex): built once on the
//              host from first-mesh coordinates, used for every mesh and every set.  Exactness never depends on the other meshes being
//              similar: the boxes below are each mesh's own.
//   V          [n_meshes][3][nv]  every mesh resident as planes;  boxes [n_meshes][30 tiles]: tile and quarter boxes of every mesh from
//              one launch (mesh_tile_bbox_kernel: tri_tile_bbox_kernel of surface_mesh.hip with a mesh index)
//   Q          [sets][3][nq]      a block of at most 512 query sets as planes: host sets through launch_aos_to_soa, instances of a model
//              (launch_instances, model_metrics.hip) through columns_to_planes_kernel
//   scan       set_distance_kernel, grid (query slab, set, mesh): the seed triangle's exact distance as the first bound, tiles and
//              quarters pruned by box gap, survivors compacted through the wave queue into closest_on_triangle, the minimum squared
//              distance kept -- no point, no triangle id, no tie rule: the minimum distance is unique.  The routines are those of
//              surface_device.h and the squared distance is the separately rounded sum of surface_cp_queue_kernel (surface.hip), so a
//              query's squared distance has the bits gingr_mesh_closest_points returns.  The epilogue takes the square root and leaves
//              one (sum, max) partial per workgroup
//   finish     the slabs added in ascending order, / nq; for the specificity the smallest mean over the meshes, lowest index on a tie
// Every sum is taken in a fixed order (a lane's queries ascending, the 16 lanes ascending, the slabs ascending; no float atomics -- the
// atomics of the scan are integer minima): two calls with the same input give the same bits, and the seed never changes a bit.
#include "gp.h"
#include "model_metrics.h"
#include "surface_device.h"
#include "surface_metrics_plan.h"

#include <algorithm>
#include <cmath>

namespace mp = model_metrics_plan;
namespace sp = surface_metrics_plan;

namespace {

constexpr int kSetCopies = 4;                 // lanes that hold a copy of every query and take alternate triangles of a quarter
constexpr int kSetQueries = 64 / kSetCopies;  // queries a workgroup holds at a time
static_assert(kSetQueries == sp::kGroupQueries, "a slab is cut into the groups the kernel walks");
static_assert(kTriTile == 256 && kCpThreads == 256, "one thread stages one triangle box of a tile");

// boxes + mesh * 30 tiles: {lo[3], hi[3]} of every 256-triangle tile of mesh blockIdx.y, then of its four 64-triangle quarters -- the
// reductions of tri_tile_bbox_kernel (surface_mesh.hip) over the mesh's own coordinates.  V: [meshes][3][nv].
__global__ __launch_bounds__(256) void mesh_tile_bbox_kernel(const double *__restrict__ V, int64_t nv, const int32_t *__restrict__ tri, int64_t T,
                                                             double *__restrict__ boxes) {
    __shared__ double sh[6][256];
    const double *vp = V + (int64_t)blockIdx.y * 3 * nv;
    double *out = boxes + (int64_t)blockIdx.y * 30 * gridDim.x;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
    double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    if (t < T)
        for (int c = 0; c < 3; ++c) {
            const int32_t a = tri[3 * t + c];
            for (int d = 0; d < 3; ++d) {
                const double p = vp[(int64_t)d * nv + a];
                lo[d] = fmin(lo[d], p);
                hi[d] = fmax(hi[d], p);
            }
        }
    for (int d = 0; d < 3; ++d) {
        sh[d][threadIdx.x] = lo[d];
        sh[3 + d][threadIdx.x] = hi[d];
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int d = 0; d < 3; ++d) {
                sh[d][threadIdx.x] = fmin(sh[d][threadIdx.x], sh[d][threadIdx.x + off]);
                sh[3 + d][threadIdx.x] = fmax(sh[3 + d][threadIdx.x], sh[3 + d][threadIdx.x + off]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[(int64_t)blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
        }
    if ((threadIdx.x & 63) == 0) {
        double *sub = out + (int64_t)gridDim.x * 6 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 6;
        for (int d = 0; d < 3; ++d) {
            sub[d] = lo[d];
            sub[3 + d] = hi[d];
        }
    }
}

// Qp[(c * 3 + d) * M + s] = P[(3 s + d) * ldt + c] for the columns c < cnt: a block of instance columns [3 M + 48][ldt] (rows in the
// model's order) as one set of query planes per column.  Block (b, d): rows [64 b, 64 b + 64), 64 columns at a time through LDS: the
// reads run along a row of P, the writes along a plane.
__global__ __launch_bounds__(256) void columns_to_planes_kernel(const double *__restrict__ P, int ldt, int64_t M, int cnt, double *__restrict__ Qp) {
    __shared__ double tile[64][65];
    const int d = blockIdx.y, tid = threadIdx.x, low = tid & 63;
    const int64_t s0 = (int64_t)blockIdx.x * 64;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        __syncthreads();
        for (int vv = tid >> 6; vv < 64; vv += 4) tile[vv][low] = (s0 + vv < M && j0 + low < cnt) ? P[(3 * (s0 + vv) + d) * ldt + j0 + low] : 0.0;
        __syncthreads();
        for (int jj = tid >> 6; jj < 64; jj += 4)
            if (s0 + low < M && j0 + jj < cnt) Qp[((int64_t)(j0 + jj) * 3 + d) * M + s0 + low] = tile[low][jj];
    }
}

struct SetScan {
    const double *Q;      // [sets][3][nq]
    const double *V;      // [n_meshes][3][nv]
    const double *boxes;  // [n_meshes][30 nt]
    const int32_t *tri;   // [3 T] vertex positions, triangles in k-d order
    const int32_t *seed;  // [nq] position in `tri` of the triangle a query starts from, -1: none; nullptr: every query starts cold
    int64_t nq, nv, T, per_slab;
    int32_t nt, pairing, set0, mesh0, n_meshes;
};

// Workgroup (slab, set, mesh): the slab's queries in groups of 16, every group the scan of surface_cp_queue_kernel (surface.hip) at four
// copies per query, reduced to the distance: the four waves hold the same 16 queries and take one 64-triangle quarter of a tile each;
// sweep 0 visits the tiles nearest to the group's box, the waves share the bound, sweep 1 visits what that bound leaves.  The seed
// triangle's distance stands in every lane's `best` before the first tile, so with a seed at the query's own vertex the scan visits the
// few quarters round it; a NaN or missing seed is a cold start.  Exactness is the pruning's alone: a quarter or triangle is skipped only
// when its box gap exceeds the bound (with the 1e-12 slack of the existing scan), never because of the seed.
// partial[(slab * pairs + pair) * 2] = the sum of sqrt(d2) over the slab's queries, [.. + 1] = the largest.
__global__ __launch_bounds__(kCpThreads) void set_distance_kernel(SetScan a, double *__restrict__ partial) {
    constexpr int H = kSetCopies, QPB = kSetQueries;
    __shared__ double tbox[kTriTile][6];
    __shared__ unsigned long long qbest[4][QPB];  // per wave and query: bits of the best squared distance so far
    __shared__ double sq[3][QPB];                 // the queries
    __shared__ unsigned int wqueue[4][128];
    __shared__ double sbound[4][QPB];
    __shared__ double red[2][QPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ql = lane & (QPB - 1), half = lane / QPB;
    const int set = blockIdx.y;
    const int mesh = a.pairing == 0 ? a.mesh0 + (int)blockIdx.z : (int)(((int64_t)a.set0 + set) % a.n_meshes);
    const int64_t pairs = a.pairing == 0 ? (int64_t)gridDim.y * gridDim.z : gridDim.y;
    const int64_t pair = a.pairing == 0 ? (int64_t)set * gridDim.z + blockIdx.z : set;
    const double *qp = a.Q + (int64_t)set * 3 * a.nq;
    const double *vp = a.V + (int64_t)mesh * 3 * a.nv;
    const Cloud v{vp, vp + a.nv, vp + 2 * a.nv, a.nv};
    const int64_t T = a.T;
    const int nt = a.nt;
    const double *boxes = a.boxes + (int64_t)mesh * 30 * nt, *qboxes = boxes + (int64_t)nt * 6;
    const int64_t s0 = (int64_t)blockIdx.x * a.per_slab, s1 = min(a.nq, s0 + a.per_slab);
    const unsigned long long kInfBits = 0x7FF0000000000000ull;
    if (wave == 0 && half == 0) red[0][ql] = 0.0, red[1][ql] = 0.0;  // the running sum and maximum of lane ql's queries (this lane's alone)
    for (int64_t g0 = s0; g0 < s1; g0 += QPB) {
        const int64_t i = g0 + ql;
        const bool ok = i < s1;
        const double qx = ok ? qp[i] : 0.0, qy = ok ? qp[a.nq + i] : 0.0, qz = ok ? qp[2 * a.nq + i] : 0.0;
        unsigned long long wbits = kInfBits;
        if (a.seed && ok) {
            const int32_t tg = a.seed[i];
            if (tg >= 0 && tg < T) {
                const Corners w = gather_corners(v, a.tri, tg);
                const V3 pq{qx, qy, qz};
                const V3 dd = sub(closest_on_triangle(pq, w.A, w.B, w.C), pq);
                const double dist = (dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z;
                if (dist == dist) wbits = __builtin_bit_cast(unsigned long long, dist);  // NaN: cold start
            }
        }
        __syncthreads();  // the last group's answers have been read
        if (half == 0) {
            qbest[wave][ql] = wbits;
            if (wave == 0) sq[0][ql] = qx, sq[1][ql] = qy, sq[2][ql] = qz;
        }
        __syncthreads();
        double best = __builtin_bit_cast(double, wbits), bound = __builtin_huge_val();
        WaveQueue wq{wqueue[wave], lane, 0};
        const Box wb = wave_box(ok, qx, qy, qz);
        auto each = [&](bool mine, int tq, int64_t tg) {
            const V3 pp{sq[0][tq], sq[1][tq], sq[2][tq]};
            const Corners c3 = gather_corners(v, a.tri, tg);
            const V3 dd = sub(closest_on_triangle(pp, c3.A, c3.B, c3.C), pp);
            const double dist = (dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z;
            const unsigned long long db = __builtin_bit_cast(unsigned long long, dist);  // (a NaN's bits lie above infinity's: never taken)
            if (mine && db < qbest[wave][tq]) atomicMin(&qbest[wave][tq], db);
            __builtin_amdgcn_wave_barrier();
            best = __builtin_bit_cast(double, qbest[wave][ql]);  // every copy of the query prunes against the shared best
        };
        double gmin = __builtin_huge_val();
        for (int t = lane; t < nt; t += 64) gmin = fmin(gmin, box_gap2(wb, boxes + (int64_t)t * 6));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gmin = fmin(gmin, __shfl_xor(gmin, off));
        gmin = uniform_d(gmin);
        for (int phase = 0; phase < 2; ++phase) {
            double bmax = ok ? bound : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, off));
            bmax = uniform_d(bmax) * (1.0 + 1e-12);
            for (int tc = 0; tc < nt; tc += 64) {
                const int tl = tc + lane;
                const double g = tl < nt ? box_gap2(wb, boxes + (int64_t)tl * 6) : __builtin_huge_val();
                unsigned long long cand = __ballot(tl < nt && (phase == 0 ? !(g > gmin) : (g > gmin && !(g > bmax))));
                while (cand) {  // workgroup-uniform (same queries, same bound in every wave)
                    const int t = tc + __builtin_ctzll(cand);
                    cand &= cand - 1;
                    const int64_t tb = (int64_t)t * kTriTile, q0 = tb + 64 * wave;
                    const double pd = point_box_gap2(qx, qy, qz, qboxes + ((int64_t)t * 4 + wave) * 6);
                    const bool need = ok && q0 < T && !(pd > fmin(best, bound) * (1.0 + 1e-12));
                    const bool wave_needs = __any(need);
                    if (!__syncthreads_or(wave_needs)) continue;
                    {
                        const int64_t tt = tb + threadIdx.x;
                        if (tt < T) stage_tri_box(tbox[threadIdx.x], tt, nullptr, a.tri, v);
                    }
                    __syncthreads();
                    if (wave_needs) {
                        const int cnt = (int)min((int64_t)64, T - q0);
                        for (int j0 = 0; j0 < cnt; j0 += H) {
                            const int jj = j0 + half;
                            const bool live = jj < cnt;
                            const double gap = point_box_gap2(qx, qy, qz, tbox[64 * wave + (live ? jj : cnt - 1)]);
                            const bool pass = need && live && !(gap > fmin(best, bound) * (1.0 + 1e-12));
                            if (wq.push(pass, ql, (unsigned)(q0 + jj))) wq.flush(64, each);
                        }
                    }
                    __syncthreads();
                }
            }
            if (wq.tail > 0) wq.flush(wq.tail, each);  // drain: the sweep's results feed the bound / the answer
            if (phase == 0) {  // share the distance bound of sweep 0 between the waves
                if (half == 0) sbound[wave][ql] = __builtin_bit_cast(double, qbest[wave][ql]);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 4; ++k) bound = fmin(bound, sbound[k][ql]);
                __syncthreads();
            }
        }
        __syncthreads();
        if (wave == 0 && half == 0 && ok) {  // the smallest of the four waves' minima; a lane adds its queries in ascending order
            unsigned long long b = qbest[0][ql];
            for (int k = 1; k < 4; ++k) b = qbest[k][ql] < b ? qbest[k][ql] : b;
            const double d = sqrt(__builtin_bit_cast(double, b));
            red[0][ql] += d;
            red[1][ql] = fmax(red[1][ql], d);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0][0], m = red[1][0];
        for (int k = 1; k < QPB; ++k) {
            s += red[0][k];
            m = fmax(m, red[1][k]);
        }
        double *out = partial + ((int64_t)blockIdx.x * pairs + pair) * 2;
        out[0] = s;
        out[1] = m;
    }
}

// pair e of a launch: the slab partials in ascending order, / nq; pairing 0 writes [set][out_stride] at column out_off + mesh
__global__ __launch_bounds__(256) void set_finish_kernel(const double *__restrict__ partial, int slabs, int64_t pairs, int meshes, int pairing, int64_t nq,
                                                         int64_t out_stride, int64_t out_off, double *__restrict__ avg, double *__restrict__ mx) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pairs) return;
    double s = 0.0, m = 0.0;
    for (int b = 0; b < slabs; ++b) {
        s += partial[((int64_t)b * pairs + e) * 2];
        m = fmax(m, partial[((int64_t)b * pairs + e) * 2 + 1]);
    }
    const int64_t set = pairing == 0 ? e / meshes : e, mesh = pairing == 0 ? e - set * meshes : 0;
    const int64_t o = pairing == 0 ? set * out_stride + out_off + mesh : set;
    avg[o] = s / (double)nq;
    mx[o] = m;
}

// Thread c, set c < sets (pairing 0): for the meshes j in ascending order the slab partials in ascending order, / nq; the smallest mean and
// its index, the lowest index on an exact tie (pair_finish_kernel, model_metrics.hip)
__global__ __launch_bounds__(256) void set_finish_min_kernel(const double *__restrict__ partial, int slabs, int sets, int meshes, int64_t nq,
                                                             double *__restrict__ min_avg, int32_t *__restrict__ argmin) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= sets) return;
    const int64_t pairs = (int64_t)sets * meshes;
    double best = 0.0;
    int32_t bi = 0;
    for (int j = 0; j < meshes; ++j) {
        double s = 0.0;
        for (int b = 0; b < slabs; ++b) s += partial[((int64_t)b * pairs + (int64_t)c * meshes + j) * 2];
        const double m = s / (double)nq;
        if (j == 0 || m < best) {
            best = m;
            bi = j;
        }
    }
    min_avg[c] = best;
    argmin[c] = bi;
}

// ---- host side
// What every pair of a call shares, on the device: the triangles, the seeds, every mesh with its boxes.
struct SharedMeshes {
    DevBuf tri, seed, order, V, boxes;
    int64_t nv = 0, T = 0, nt = 0;
    int32_t n_meshes = 0;
    bool seeded = false;
};

int check_triangles(gingr_ctx *ctx, const char *who, int64_t n_vertices, int64_t n_triangles, const int32_t *triangles) {
    if (n_triangles < 1 || n_triangles > sp::kMaxTriangles)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %lld triangles, need 1 <= n_triangles <= %lld", who, (long long)n_triangles,
                               (long long)sp::kMaxTriangles);
    for (int64_t k = 0; k < 3 * n_triangles; ++k)
        if (triangles[k] < 0 || triangles[k] >= n_vertices)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: triangle %lld has vertex id %d outside 0..%lld", who, (long long)(k / 3),
                                   (int)triangles[k], (long long)(n_vertices - 1));
    return GINGR_OK;
}

// A call that would not fit is refused with its size, before anything is allocated.
int check_working_set(gingr_ctx *ctx, const char *who, int64_t n_points, int64_t block_sets, int64_t n_vertices, int64_t n_meshes, int64_t n_triangles,
                      int64_t model_rows) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const int64_t need = sp::working_set_bytes(n_points, block_sets, n_vertices, n_meshes, n_triangles, model_rows);
    if (need < 0 || (uint64_t)need > (uint64_t)free_b)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT,
                               "%s: the working set (%lld meshes of %lld vertices, %lld sets of %lld points at a time) needs %lld bytes on the device, %lld are free",
                               who, (long long)n_meshes, (long long)n_vertices, (long long)block_sets, (long long)n_points, (long long)need,
                               (long long)free_b);
    return GINGR_OK;
}

// cnt host point lists of n points each (interleaved xyz) as planes [cnt][3][n] in the order `order` (device: position -> input index),
// a few lists per transfer through one staging buffer of at most 64 MB.  Synchronises.
int upload_planes(gingr_ctx *ctx, const double *xyz, int64_t n, int64_t cnt, const int32_t *order, double *planes) {
    DevBuf stage;
    const int64_t per_stage = std::max<int64_t>(1, std::min<int64_t>(cnt, ((int64_t)8 << 20) / (3 * n)));
    HIP_TRY(ctx, stage.alloc((size_t)per_stage * 3 * n * sizeof(double)));
    for (int64_t i0 = 0; i0 < cnt; i0 += per_stage) {
        const int64_t part = std::min(per_stage, cnt - i0);
        HIP_TRY(ctx, hipMemcpyAsync(stage.p, xyz + (size_t)i0 * 3 * n, (size_t)part * 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        for (int64_t j = 0; j < part; ++j) launch_aos_to_soa(ctx, stage.as<double>() + (size_t)j * 3 * n, n, planes + (size_t)(i0 + j) * 3 * n, order);
        GINGR_TRY(check_launch(ctx));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffer is written again
    }
    return GINGR_OK;
}

// The shared topology from the first mesh, every mesh and its boxes on the device.  query_vertex (nullable, n_queries entries): the
// mesh vertex (caller's numbering) query position s lies near -- its seed is that vertex's lowest-numbered triangle.
int upload_meshes(gingr_ctx *ctx, int64_t nv, int32_t n_meshes, const double *meshes_xyz, int64_t T, const int32_t *triangles,
                  const std::vector<int32_t> &vorder, const std::vector<int32_t> &torder, const std::vector<int32_t> &tri, const int32_t *query_vertex,
                  int64_t n_queries, SharedMeshes &sm) {
    sm.nv = nv, sm.T = T, sm.nt = ceil_div(T, kTriTile), sm.n_meshes = n_meshes, sm.seeded = query_vertex != nullptr;
    HIP_TRY(ctx, sm.tri.alloc(tri.size() * sizeof(int32_t)));
    HIP_TRY(ctx, sm.order.alloc(vorder.size() * sizeof(int32_t)));
    HIP_TRY(ctx, sm.V.alloc((size_t)n_meshes * 3 * nv * sizeof(double)));
    HIP_TRY(ctx, sm.boxes.alloc((size_t)n_meshes * 30 * sm.nt * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(sm.tri.p, tri.data(), tri.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sm.order.p, vorder.data(), vorder.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> seed;
    if (query_vertex) {
        std::vector<int32_t> by_vertex, tinv((size_t)T);
        sp::seed_triangles(nv, T, triangles, by_vertex);
        for (int64_t s = 0; s < T; ++s) tinv[(size_t)torder[(size_t)s]] = (int32_t)s;
        seed.resize((size_t)n_queries);
        for (int64_t s = 0; s < n_queries; ++s) {
            const int32_t t = by_vertex[(size_t)query_vertex[s]];
            seed[(size_t)s] = t < 0 ? -1 : tinv[(size_t)t];
        }
        HIP_TRY(ctx, sm.seed.alloc(seed.size() * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(sm.seed.p, seed.data(), seed.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    GINGR_TRY(upload_planes(ctx, meshes_xyz, nv, n_meshes, sm.order.as<int32_t>(), sm.V.as<double>()));  // (synchronises: `seed` may go)
    for (int32_t m0 = 0; m0 < n_meshes; m0 += 32768) {
        const int32_t cnt = std::min<int32_t>(32768, n_meshes - m0);
        hipLaunchKernelGGL(mesh_tile_bbox_kernel, dim3((unsigned)sm.nt, (unsigned)cnt), dim3(256), 0, ctx->stream, sm.V.as<double>() + (size_t)m0 * 3 * nv, nv,
                           sm.tri.as<int32_t>(), T, sm.boxes.as<double>() + (size_t)m0 * 30 * sm.nt);
    }
    return check_launch(ctx);
}

// One launch of the scan on ctx->stream: `sets` query sets (planes Q, nq points each; set 0 is set `set0` of the call) against the
// meshes [mesh0, mesh0 + meshes) (pairing 0) or against mesh (set0 + c) % n_meshes each (pairing 1).  Timing hook 23: the scan alone.
int launch_set_scan(gingr_ctx *ctx, const SharedMeshes &sm, const double *Q, int64_t nq, int sets, int64_t set0, int pairing, int mesh0, int meshes,
                    const sp::PairPlan &plan, DevBuf &partial) {
    if ((size_t)plan.partial_doubles() * sizeof(double) > partial.bytes) HIP_TRY(ctx, partial.alloc((size_t)plan.partial_doubles() * sizeof(double)));
    SetScan a;
    a.Q = Q, a.V = sm.V.as<double>(), a.boxes = sm.boxes.as<double>(), a.tri = sm.tri.as<int32_t>(), a.seed = sm.seeded ? sm.seed.as<int32_t>() : nullptr;
    a.nq = nq, a.nv = sm.nv, a.T = sm.T, a.per_slab = plan.per_slab;
    a.nt = (int32_t)sm.nt, a.pairing = pairing, a.set0 = (int32_t)(set0 % sm.n_meshes), a.mesh0 = mesh0, a.n_meshes = sm.n_meshes;
    TimerScope ts(ctx, 23);
    hipLaunchKernelGGL(set_distance_kernel, dim3((unsigned)plan.slabs, (unsigned)sets, (unsigned)(pairing == 0 ? meshes : 1)), dim3(kCpThreads), 0,
                       ctx->stream, a, partial.as<double>());
    return GINGR_OK;
}

// Every set of a block against every mesh (pairing 0) or its own mesh (pairing 1): avg / max (device) as [sets][n_meshes] or [sets]
int run_set_block(gingr_ctx *ctx, const SharedMeshes &sm, const double *Q, int64_t nq, int sets, int64_t set0, int pairing, DevBuf &partial, double *avg,
                  double *mx) {
    const sp::MeshChunks chunks = sp::mesh_chunks(sm.n_meshes, pairing);
    for (int64_t c = 0; c < chunks.count; ++c) {
        const int meshes = (int)chunks.length(c), mesh0 = (int)chunks.begin(c);
        const sp::PairPlan plan = sp::make_pair_plan(nq, sets, meshes, pairing);
        GINGR_TRY(launch_set_scan(ctx, sm, Q, nq, sets, set0, pairing, mesh0, meshes, plan, partial));
        hipLaunchKernelGGL(set_finish_kernel, dim3((unsigned)ceil_div(plan.pairs, 256)), dim3(256), 0, ctx->stream, partial.as<double>(), (int)plan.slabs,
                           plan.pairs, meshes, pairing, nq, (int64_t)sm.n_meshes, (int64_t)mesh0, avg, mx);
        GINGR_TRY(check_launch(ctx));
    }
    return GINGR_OK;
}

// the shared topology of a model route: the shapes are in correspondence with the model's reference, so query s (row s of the model's
// order) lies near vertex hperm[s] of every shape
int upload_model_meshes(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, int64_t T, const int32_t *triangles, SharedMeshes &sm) {
    const int64_t M = model->M;
    std::vector<int32_t> qorder, vorder, torder, vinv, tri;
    mesh_orders(M, shapes_xyz, M, shapes_xyz, T, triangles, qorder, vorder, torder, vinv, tri);
    std::vector<int32_t> rows((size_t)M);  // the model's row order: device row -> vertex
    HIP_TRY(ctx, hipMemcpyAsync(rows.data(), model->perm, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return upload_meshes(ctx, M, n, shapes_xyz, T, triangles, vorder, torder, tri, rows.data(), M, sm);
}

}  // namespace

extern "C" {

int gingr_mesh_set_distances(gingr_ctx *ctx, int64_t n_points, int64_t n_sets, const double *sets_xyz, int64_t n_vertices, int64_t n_meshes,
                             const double *meshes_xyz, int64_t n_triangles, const int32_t *triangles, int32_t pairing, int32_t corresponding, double *avg,
                             double *max_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "mesh_set_distances";
    if (!sets_xyz || !meshes_xyz || !triangles || !avg || !max_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (n_points < 1 || n_sets < 1 || n_vertices < 1 || n_meshes < 1 || n_points > INT32_MAX || n_vertices > INT32_MAX || n_meshes > INT32_MAX ||
        n_sets > INT32_MAX)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %lld sets of %lld points, %lld meshes of %lld vertices: every count must be >= 1 (and < 2^31)",
                               who, (long long)n_sets, (long long)n_points, (long long)n_meshes, (long long)n_vertices);
    if (pairing != 0 && pairing != 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: pairing = %d, need 0 (all) or 1 (cyclic)", who, (int)pairing);
    if (corresponding && n_points != n_vertices)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: corresponding sets need n_points == n_vertices (%lld points, %lld vertices)", who,
                               (long long)n_points, (long long)n_vertices);
    GINGR_TRY(check_triangles(ctx, who, n_vertices, n_triangles, triangles));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const mp::ColumnBlocks blocks = mp::column_blocks(n_sets);
    const int64_t block_sets = blocks.length(0), out_cols = pairing == 0 ? n_meshes : 1;
    GINGR_TRY(check_working_set(ctx, who, n_points, block_sets, n_vertices, n_meshes, n_triangles, 0));  // (before the arrays are read)
    GINGR_TRY(check_finite(ctx, sets_xyz, 3 * n_points, n_sets, who, "set"));
    GINGR_TRY(check_finite(ctx, meshes_xyz, 3 * n_vertices, n_meshes, who, "mesh"));

    std::vector<int32_t> qorder, vorder, torder, vinv, tri;
    mesh_orders(n_points, sets_xyz, n_vertices, meshes_xyz, n_triangles, triangles, qorder, vorder, torder, vinv, tri);
    SharedMeshes sm;
    GINGR_TRY(upload_meshes(ctx, n_vertices, (int32_t)n_meshes, meshes_xyz, n_triangles, triangles, vorder, torder, tri, corresponding ? qorder.data() : nullptr,
                            n_points, sm));
    DevBuf qord, Q, partial, res;
    HIP_TRY(ctx, qord.alloc(qorder.size() * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(qord.p, qorder.data(), qorder.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, Q.alloc((size_t)block_sets * 3 * n_points * sizeof(double)));
    HIP_TRY(ctx, res.alloc((size_t)2 * block_sets * out_cols * sizeof(double)));
    for (int64_t b = 0; b < blocks.count; ++b) {
        const int cnt = (int)blocks.length(b);
        const int64_t c0 = blocks.begin(b);
        GINGR_TRY(upload_planes(ctx, sets_xyz + (size_t)c0 * 3 * n_points, n_points, cnt, qord.as<int32_t>(), Q.as<double>()));
        double *ravg = res.as<double>(), *rmax = ravg + (size_t)block_sets * out_cols;
        GINGR_TRY(run_set_block(ctx, sm, Q.as<double>(), n_points, cnt, c0, pairing, partial, ravg, rmax));
        HIP_TRY(ctx, hipMemcpyAsync(avg + (size_t)c0 * out_cols, ravg, (size_t)cnt * out_cols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(max_out + (size_t)c0 * out_cols, rmax, (size_t)cnt * out_cols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GINGR_OK;
}

int gingr_model_generalization_surface(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, int64_t n_triangles,
                                       const int32_t *triangles, int32_t n_ranks, const int32_t *ranks, double *coeffs, double *avg, double *max_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_generalization_surface";
    if (!model || !shapes_xyz || !triangles || !avg || !max_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    GINGR_TRY(metrics_check_model(ctx, model, who));
    if (n < 1 || n > mp::kMaxShapes)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d shapes, need 1 <= n <= %d per call", who, (int)n, (int)mp::kMaxShapes);
    RankList rl;
    GINGR_TRY(metrics_check_ranks(ctx, model, n_ranks, ranks, who, &rl));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    GINGR_TRY(check_triangles(ctx, who, M, n_triangles, triangles));
    GINGR_TRY(check_finite(ctx, shapes_xyz, 3 * M, n, who, "shape"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int np = (int)mp::padded_cols(n), ldt = n_ranks * np;
    GINGR_TRY(check_working_set(ctx, who, M, n, M, n, n_triangles, mp::block_rows(M)));

    // ---- the coefficient columns of the vertex route (the same launches: the same bits), every shape as a mesh
    RankFactors f;
    GINGR_TRY(project_rank_factors(ctx, model, n, shapes_xyz, rl, coeffs != nullptr, f));
    SharedMeshes sm;
    GINGR_TRY(upload_model_meshes(ctx, model, n, shapes_xyz, n_triangles, triangles, sm));

    // ---- rank by rank: the projections stored (a block of np <= 512 columns), as query planes, projection i against shape i
    DevBuf Tq, P, Q, partial, res;
    HIP_TRY(ctx, Tq.alloc((size_t)rp * np * sizeof(double)));
    HIP_TRY(ctx, P.alloc((size_t)mp::block_rows(M) * np * sizeof(double)));
    HIP_TRY(ctx, Q.alloc((size_t)n * 3 * M * sizeof(double)));
    HIP_TRY(ctx, res.alloc((size_t)2 * n_ranks * n * sizeof(double)));
    for (int32_t q = 0; q < n_ranks; ++q) {
        HIP_TRY(ctx, hipMemcpy2DAsync(Tq.p, (size_t)np * sizeof(double), f.T.as<double>() + (size_t)q * np, (size_t)ldt * sizeof(double), (size_t)np * sizeof(double),
                                      (size_t)rp, hipMemcpyDeviceToDevice, ctx->stream));
        launch_instances(ctx, model, Tq.as<double>(), np, P.as<double>());
        hipLaunchKernelGGL(columns_to_planes_kernel, dim3((unsigned)ceil_div(M, 64), 3), dim3(256), 0, ctx->stream, P.as<double>(), np, M, (int)n, Q.as<double>());
        GINGR_TRY(check_launch(ctx));
        GINGR_TRY(run_set_block(ctx, sm, Q.as<double>(), M, (int)n, 0, 1, partial, res.as<double>() + (size_t)q * n,
                                res.as<double>() + (size_t)(n_ranks + q) * n));
    }
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, f.flag, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "%s: Q^T Q / 1e-5 + I is not positive definite", who);
    HIP_TRY(ctx, hipMemcpyAsync(avg, res.p, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(max_out, res.as<double>() + (size_t)n_ranks * n, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (coeffs) HIP_TRY(ctx, hipMemcpyAsync(coeffs, f.coef.p, (size_t)n_ranks * n * r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_model_specificity_surface(gingr_ctx *ctx, const gingr_model *model, int32_t n_train, const double *train_xyz, int64_t n_triangles,
                                    const int32_t *triangles, int64_t n_samples, const double *alphas, int32_t n_ranks, const int32_t *ranks, double *min_avg,
                                    int32_t *argmin) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_specificity_surface";
    if (!model || !train_xyz || !triangles || !alphas || !min_avg || !argmin) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    GINGR_TRY(metrics_check_model(ctx, model, who));
    if (n_train < 1 || n_train > mp::kMaxShapes)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d training shapes, need 1 <= n_train <= %d", who, (int)n_train, (int)mp::kMaxShapes);
    if (n_samples < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n_samples = %lld < 1", who, (long long)n_samples);
    RankList rl;
    GINGR_TRY(metrics_check_ranks(ctx, model, n_ranks, ranks, who, &rl));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    GINGR_TRY(check_triangles(ctx, who, M, n_triangles, triangles));
    GINGR_TRY(check_finite(ctx, train_xyz, 3 * M, n_train, who, "training shape"));
    GINGR_TRY(check_finite(ctx, alphas, r, n_samples, who, "coefficient vector"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const mp::ColumnBlocks blocks = mp::column_blocks(n_samples);
    const int ldmax = (int)blocks.padded(0);
    GINGR_TRY(check_working_set(ctx, who, M, blocks.length(0), M, n_train, n_triangles, mp::block_rows(M)));

    SharedMeshes sm;
    GINGR_TRY(upload_model_meshes(ctx, model, n_train, train_xyz, n_triangles, triangles, sm));
    DevBuf A, T, P, Q, partial, best, besti;
    HIP_TRY(ctx, A.alloc((size_t)ldmax * r * sizeof(double)));
    HIP_TRY(ctx, T.alloc((size_t)rp * ldmax * sizeof(double)));
    HIP_TRY(ctx, P.alloc((size_t)mp::block_rows(M) * ldmax * sizeof(double)));
    HIP_TRY(ctx, Q.alloc((size_t)blocks.length(0) * 3 * M * sizeof(double)));
    HIP_TRY(ctx, best.alloc((size_t)ldmax * sizeof(double)));
    HIP_TRY(ctx, besti.alloc((size_t)ldmax * sizeof(int32_t)));
    for (int64_t b = 0; b < blocks.count; ++b) {
        const int cnt = (int)blocks.length(b), ldt = (int)blocks.padded(b);
        const int64_t c0 = blocks.begin(b);
        const sp::PairPlan plan = sp::make_pair_plan(M, cnt, n_train, 0);
        HIP_TRY(ctx, hipMemcpyAsync(A.p, alphas + c0 * r, (size_t)cnt * r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        for (int32_t q = 0; q < n_ranks; ++q) {
            launch_sample_factor(ctx, A.as<double>(), cnt, (int)r, (int)rl.k[q], (int)rp, ldt, T.as<double>());
            launch_instances(ctx, model, T.as<double>(), ldt, P.as<double>());
            hipLaunchKernelGGL(columns_to_planes_kernel, dim3((unsigned)ceil_div(M, 64), 3), dim3(256), 0, ctx->stream, P.as<double>(), ldt, M, cnt, Q.as<double>());
            GINGR_TRY(launch_set_scan(ctx, sm, Q.as<double>(), M, cnt, c0, 0, 0, (int)n_train, plan, partial));
            hipLaunchKernelGGL(set_finish_min_kernel, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, ctx->stream, partial.as<double>(), (int)plan.slabs, cnt,
                               (int)n_train, M, best.as<double>(), besti.as<int32_t>());
            GINGR_TRY(check_launch(ctx));
            HIP_TRY(ctx, hipMemcpyAsync(min_avg + (size_t)q * n_samples + c0, best.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(argmin + (size_t)q * n_samples + c0, besti.p, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GINGR_OK;
}

}  // extern "C"
