// k nearest neighbours of a cloud within itself and the normals of those neighbourhoods (C ABI in include/gingr_hip.h: gingr_cloud_knn,
// gingr_cloud_normals; the fitter's gingr_fitter_estimate_target_normals runs the same passes on the target as it lies on the device).
//
// The grid.  Built on the device per call: bounding box (block partials, combined on the host, which also plans the grid:
// cloud_knn_plan.h), one cell key per point, a stable radix sort of (key, position), and one pass that writes the points in cell order
// (coordinates, original index, position) and the start of every cell.  No atomics; the order inside a cell is the order of the cloud.
//
// The search.  G = 16, 32 or 64 lanes serve one query (the smallest that holds k) and keep its k-best list ONE ENTRY PER LANE, sorted by
// (d2, original index): lane i of the group holds the i-th best.  The lanes read G consecutive points of a row of cells (a run along x)
// at a time; a point that beats the k-th entry is broadcast and inserted -- the lanes holding smaller entries keep theirs (they are a
// prefix, counted by a ballot), the lane behind them takes the point, the rest take their left neighbour's entry (one shuffle).  The list
// never leaves the registers and is never indexed by a run-time value.  The order the points arrive in does not matter: (d2, index) is a
// total order and every point of a pass is met once.
//
// Exactness, by the rule of nn_grid.hip: after the block of cells [c - R, c + R]^3 every point not met is farther than R h from the query,
// so the list is exact once its k-th distance is at most (R h)^2 (1 - 1e-9) -- or the block was the whole grid.  Otherwise the list is
// started again with the R that covers the k-th distance found (R + 1 when fewer than k points were met), up to kMaxR.  A query that
// needs more, or whose block has a row of more than kMaxRowPoints points, is FLAGGED and answered by the same kernel in its scan-all form
// over every point of the cloud (launched only when something was flagged; workgroups without a flagged query leave at once).
// d2 is norm2_exact (box_device.h): the bits of dx*dx + dy*dy + dz*dz on a CPU.  Integer atomics count the flagged queries; nothing that
// reaches a result is accumulated atomically: two calls give the same bits.
#include "common.h"
#include "box_device.h"
#include "cloud_knn_plan.h"
#include "sym_eig3.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace {

namespace plan = cloud_knn_plan;

constexpr int kBoxBlocks = 512;  // block partials of the bounding box: {lo[3], hi[3], non-finite points}

struct KnnGridDev {  // what the kernels need, by value
    double lo[3];
    double h, inv_h;
    int32_t g[3];
    const int32_t *cell_start;  // [g0 g1 g2 + 1], x fastest
    const GridPoint *pts;       // [N] in cell order: orig = the caller's index, pos = position in the cloud on the device
    const int32_t *cell;        // [N] the cell of pts[.]
};

__global__ __launch_bounds__(256) void cloud_box_kernel(Cloud c, double *__restrict__ part /* [gridDim.x][7] */) {
    double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
    double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    double bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < c.n; i += (int64_t)gridDim.x * 256) {
        const double v[3] = {c.x[i], c.y[i], c.z[i]};
        if (fabs(v[0]) <= kDblMax && fabs(v[1]) <= kDblMax && fabs(v[2]) <= kDblMax) {
#pragma unroll
            for (int d = 0; d < 3; ++d) lo[d] = fmin(lo[d], v[d]), hi[d] = fmax(hi[d], v[d]);
        } else {
            bad += 1.0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) lo[d] = fmin(lo[d], __shfl_xor(lo[d], off)), hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
        bad += __shfl_xor(bad, off);  // (a count: exact in any order)
    }
    __shared__ double sh[4][7];
    if ((threadIdx.x & 63) == 0) {
        double *s = sh[threadIdx.x >> 6];
        s[0] = lo[0], s[1] = lo[1], s[2] = lo[2], s[3] = hi[0], s[4] = hi[1], s[5] = hi[2], s[6] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int q = threadIdx.x;
        double v = sh[0][q];
        for (int w = 1; w < 4; ++w) v = q < 3 ? fmin(v, sh[w][q]) : (q < 6 ? fmax(v, sh[w][q]) : v + sh[w][q]);
        part[(int64_t)blockIdx.x * 7 + q] = v;
    }
}

__global__ __launch_bounds__(256) void cloud_cell_keys_kernel(Cloud c, KnnGridDev g, int32_t *__restrict__ keys, int32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const int32_t cx = plan::cell_of(c.x[i], g.lo[0], g.inv_h, g.g[0]), cy = plan::cell_of(c.y[i], g.lo[1], g.inv_h, g.g[1]),
                  cz = plan::cell_of(c.z[i], g.lo[2], g.inv_h, g.g[2]);
    keys[i] = (cz * g.g[1] + cy) * g.g[0] + cx;  // (< 2^30 cells: the planner)
    vals[i] = (int32_t)i;
}

// sorted position p: the point record in cell order, and the start of every cell between the previous point's cell and this one's
__global__ __launch_bounds__(256) void cloud_cell_fill_kernel(Cloud c, const int32_t *__restrict__ orig, const int32_t *__restrict__ skeys,
                                                              const int32_t *__restrict__ svals, int64_t ncells, GridPoint *__restrict__ pts,
                                                              int32_t *__restrict__ cell_start) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= c.n) return;
    const int32_t i = svals[p];
    pts[p] = GridPoint{c.x[i], c.y[i], c.z[i], orig ? orig[i] : i, i};
    const int64_t cur = skeys[p], prev = p > 0 ? (int64_t)skeys[p - 1] : -1;
    for (int64_t q = prev + 1; q <= cur; ++q) cell_start[q] = (int32_t)p;
    if (p == c.n - 1)
        for (int64_t q = cur + 1; q <= ncells; ++q) cell_start[q] = (int32_t)c.n;
}

__device__ __forceinline__ bool before(double ad, int32_t ao, double bd, int32_t bo) { return ad < bd || (ad == bd && ao < bo); }

// BRUTE: only the queries with flag != 0, against every point of the cloud.  Every shuffle and ballot sits in wave-uniform control flow:
// the loops run while ANY lane of the wave has work, lanes without work take part with empty ranges.
template <int G, bool BRUTE>
__global__ __launch_bounds__(256) void cloud_knn_kernel(KnnGridDev g, int64_t N, int k, uint8_t *__restrict__ flag, int32_t *__restrict__ nflag,
                                                        int32_t *__restrict__ idx, double *__restrict__ d2out, int32_t *__restrict__ posout) {
    const int lane = threadIdx.x & 63, li = lane % G, gbase = lane - li;
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << gbase;
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;  // the query: a position in cell order
    const bool mine = p < N && (!BRUTE || flag[p] != 0);
    if (!__any(mine)) return;
    const int64_t pc = p < N ? p : N - 1;
    const GridPoint q = g.pts[pc];
    double ed = __builtin_huge_val(), kd = __builtin_huge_val();  // this lane's entry of the list; the k-th entry
    int32_t eo = INT32_MAX, ep = -1, ko = INT32_MAX;              // (original index, position in cell order)

    auto scan_run = [&](int32_t s, int32_t e) {  // the points [s, e) of the cell-ordered cloud into the list
        for (int32_t base = s; __any(base < e); base += G) {
            const int32_t j = base + li;
            bool cand = j < e;
            const GridPoint c = g.pts[cand ? j : 0];
            const double cd = norm2_exact(c.x - q.x, c.y - q.y, c.z - q.z);
            cand = cand && before(cd, c.orig, kd, ko);
            unsigned long long bal;
            while ((bal = __ballot(cand)) != 0ull) {
                const unsigned long long gb = bal & gmask;
                const int src = gb ? __ffsll(gb) - 1 : lane;  // the group's first lane with a point to insert
                const double bd = __shfl(cd, src);
                const int32_t bo = __shfl(c.orig, src), bp = __shfl(j, src);
                const int at = __popcll(__ballot(before(ed, eo, bd, bo)) & gmask);  // entries in front of it: a prefix of the group
                const double ud = __shfl_up(ed, 1, G);
                const int32_t uo = __shfl_up(eo, 1, G), up = __shfl_up(ep, 1, G);
                if (gb) {
                    if (li == at)
                        ed = bd, eo = bo, ep = bp;
                    else if (li > at)
                        ed = ud, eo = uo, ep = up;
                }
                kd = __shfl(ed, gbase + k - 1);
                ko = __shfl(eo, gbase + k - 1);
                if (lane == src) cand = false;
                cand = cand && before(cd, c.orig, kd, ko);
            }
        }
    };

    bool flagged = false;
    if (BRUTE) {
        scan_run(0, mine ? (int32_t)N : 0);
    } else {
        const int32_t cell = g.cell[pc];
        const int g0 = g.g[0], g1 = g.g[1], g2 = g.g[2];
        const int cx = cell % g0, cy = (cell / g0) % g1, cz = cell / (g0 * g1);
        const double fy = (q.y - g.lo[1]) * g.inv_h, fz = (q.z - g.lo[2]) * g.inv_h, h2 = g.h * g.h;
        int R = 1;
        bool busy = mine;
        while (__any(busy)) {
            if (busy) ed = kd = __builtin_huge_val(), eo = ko = INT32_MAX, ep = -1;  // every pass starts an empty list
            const int x0 = max(cx - R, 0), x1 = min(cx + R, g0 - 1), y0 = max(cy - R, 0), y1 = min(cy + R, g1 - 1), z0 = max(cz - R, 0),
                      z1 = min(cz + R, g2 - 1);
            const int ny = y1 - y0 + 1, nrows = busy ? ny * (z1 - z0 + 1) : 0;
            bool crowded = false;
            for (int r = 0; __any(r < nrows); ++r) {
                int32_t s = 0, e = 0;
                if (r < nrows) {
                    const int ry = y0 + r % ny, rz = z0 + r / ny;
                    const double gy = fmax(fmax((double)ry - fy, fy - (double)(ry + 1)), 0.0);
                    const double gz = fmax(fmax((double)rz - fz, fz - (double)(rz + 1)), 0.0);
                    // a full list and a row whose nearest point is farther than its k-th entry: nothing in it can enter
                    if (!(ko != INT32_MAX && (gy * gy + gz * gz) * h2 * (1.0 - 1e-9) > kd)) {
                        const int64_t row = ((int64_t)rz * g1 + ry) * g0;
                        s = g.cell_start[row + x0], e = g.cell_start[row + x1 + 1];
                        if (e - s > plan::kMaxRowPoints) crowded = true, s = e = 0;
                    }
                }
                scan_run(s, e);
            }
            if (busy) {
                const bool whole = x0 == 0 && y0 == 0 && z0 == 0 && x1 == g0 - 1 && y1 == g1 - 1 && z1 == g2 - 1;
                const bool full = ko != INT32_MAX;
                const double reach = (double)R * g.h;
                if (crowded) {
                    flagged = true, busy = false;
                } else if (whole || (full && kd <= reach * reach * (1.0 - 1e-9))) {
                    busy = false;
                } else {
                    int next = R + 1;
                    if (full) {
                        const double need = ceil(sqrt(kd) * g.inv_h * (1.0 + 1e-9));
                        next = need > (double)plan::kMaxR ? plan::kMaxR + 1 : max(next, (int)need);
                    }
                    if (next > plan::kMaxR)
                        flagged = true, busy = false;
                    else
                        R = next;
                }
            }
        }
    }
    if (mine && !flagged && li < k) {
        const int64_t o = (int64_t)q.pos * k + li;
        if (idx) idx[o] = eo;
        if (d2out) d2out[o] = ed;
        if (posout) posout[o] = ep;
    }
    if (!BRUTE) {
        if (mine && li == 0) flag[p] = flagged ? 1 : 0;
        const unsigned long long fb = __ballot(flagged && li == 0);
        if (fb && lane == 0) atomicAdd(nflag, (int32_t)__popcll(fb));
    }
}

// Per point t of the cloud (device position), from its neighbour list in the list's order (positions in the cell-ordered records):
// q_i = x_i - x_t, m = sum q_i / k, C = sum (q_i - m)(q_i - m)^T / k, then sym_eig3::normal_of; with a viewpoint v the normal is turned so
// that n . (v - x_t) >= 0.  out[t * sp + axis * sa]: interleaved (sp 3, sa 1) or planes (sp 1, sa N).
__global__ __launch_bounds__(256) void cloud_normals_kernel(Cloud c, int k, const GridPoint *__restrict__ pts, const int32_t *__restrict__ nbr,
                                                            int has_view, double vx, double vy, double vz, double *__restrict__ out, int64_t sp,
                                                            int64_t sa, double *__restrict__ variation) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= c.n) return;
    const double x = c.x[t], y = c.y[t], z = c.z[t];
    const int32_t *list = nbr + t * k;
    const double kk = (double)k;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int i = 0; i < k; ++i) {
        const GridPoint p = pts[list[i]];
        mx += p.x - x, my += p.y - y, mz += p.z - z;
    }
    mx /= kk, my /= kk, mz /= kk;
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < k; ++i) {
        const GridPoint p = pts[list[i]];
        const double dx = (p.x - x) - mx, dy = (p.y - y) - my, dz = (p.z - z) - mz;
        c6[0] += dx * dx, c6[1] += dx * dy, c6[2] += dx * dz, c6[3] += dy * dy, c6[4] += dy * dz, c6[5] += dz * dz;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) c6[q] /= kk;
    double n[3], var;
    sym_eig3::normal_of(c6, n, &var);
    if (has_view && (n[0] * (vx - x) + n[1] * (vy - y)) + n[2] * (vz - z) < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    out[t * sp] = n[0];
    out[t * sp + sa] = n[1];
    out[t * sp + 2 * sa] = n[2];
    if (variation) variation[t] = var;
}

template <bool BRUTE>
void launch_knn(gingr_ctx *ctx, const KnnGridDev &g, int64_t N, int k, uint8_t *flag, int32_t *nflag, int32_t *idx, double *d2, int32_t *pos) {
    const int G = plan::group_lanes(k);
    const dim3 grid((unsigned)ceil_div(N * G, 256)), block(256);
    if (G == 16)
        hipLaunchKernelGGL((cloud_knn_kernel<16, BRUTE>), grid, block, 0, ctx->stream, g, N, k, flag, nflag, idx, d2, pos);
    else if (G == 32)
        hipLaunchKernelGGL((cloud_knn_kernel<32, BRUTE>), grid, block, 0, ctx->stream, g, N, k, flag, nflag, idx, d2, pos);
    else
        hipLaunchKernelGGL((cloud_knn_kernel<64, BRUTE>), grid, block, 0, ctx->stream, g, N, k, flag, nflag, idx, d2, pos);
}

struct KnnWork {  // everything a search allocates; freed when it goes out of scope
    DevBuf part, keys, vals, skeys, svals, sort, cell_start, pts, flag, nflag;
    KnnGridDev grid{};
};

int check_k(gingr_ctx *ctx, int64_t N, int32_t k, const char *who) {
    if (N < 1 || N > ((int64_t)1 << 27)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: need 1 <= N <= 2^27", who);
    if (k < plan::kMinK || k > plan::kMaxK || k > N)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: need %d <= k <= %d and k <= N", who, plan::kMinK, plan::kMaxK);
    return GINGR_OK;
}

// the neighbour lists of cloud `c` (SoA on the device; orig: position -> the caller's index, nullable) into idx / d2 / pos, each
// [N][k] on the device and nullable, row t the list of the point at device position t.  Synchronises.  w keeps the grid for the caller.
int knn_search(gingr_ctx *ctx, Cloud c, const int32_t *orig, int32_t k, int32_t *idx, double *d2, int32_t *pos, KnnWork &w,
               gingr_cloud_knn_info *info, const char *who) {
    const int64_t N = c.n;
    const int nb = (int)std::min<int64_t>(ceil_div(N, 256), kBoxBlocks);
    HIP_TRY(ctx, w.part.alloc((size_t)nb * 7 * sizeof(double)));
    hipLaunchKernelGGL(cloud_box_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, c, w.part.as<double>());
    std::vector<double> part((size_t)nb * 7);
    HIP_TRY(ctx, hipMemcpyAsync(part.data(), w.part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, bad = 0.0;
    for (int b = 0; b < nb; ++b) {
        for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], part[(size_t)b * 7 + d]), hi[d] = std::max(hi[d], part[(size_t)b * 7 + 3 + d]);
        bad += part[(size_t)b * 7 + 6];
    }
    if (bad != 0.0) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: %.0f points with a non-finite coordinate", who, bad);
    for (int d = 0; d < 3; ++d)  // (squared distances must stay finite)
        if (!(hi[d] - lo[d] < 1e150)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the cloud extends over more than 1e150", who);
    const plan::Plan pl = plan::make_plan(N, k, lo, hi);
    const int64_t ncells = pl.ncells();
    const size_t n = (size_t)N;
    HIP_TRY(ctx, w.keys.alloc(n * sizeof(int32_t)));
    HIP_TRY(ctx, w.vals.alloc(n * sizeof(int32_t)));
    HIP_TRY(ctx, w.skeys.alloc(n * sizeof(int32_t)));
    HIP_TRY(ctx, w.svals.alloc(n * sizeof(int32_t)));
    HIP_TRY(ctx, w.cell_start.alloc((size_t)(ncells + 1) * sizeof(int32_t)));
    HIP_TRY(ctx, w.pts.alloc(n * sizeof(GridPoint)));
    HIP_TRY(ctx, w.flag.alloc(n));
    HIP_TRY(ctx, w.nflag.alloc(sizeof(int32_t)));
    KnnGridDev &g = w.grid;
    for (int d = 0; d < 3; ++d) g.lo[d] = pl.lo[d], g.g[d] = pl.g[d];
    g.h = pl.h, g.inv_h = pl.inv_h;
    g.cell_start = w.cell_start.as<int32_t>();
    g.pts = w.pts.as<GridPoint>();
    g.cell = w.skeys.as<int32_t>();
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < ncells) ++bits;
    size_t sort_bytes = 0;
    HIP_TRY(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, w.keys.as<int32_t>(), w.skeys.as<int32_t>(), w.vals.as<int32_t>(),
                                                    w.svals.as<int32_t>(), (int)N, 0, bits, ctx->stream));
    HIP_TRY(ctx, w.sort.alloc(sort_bytes));
    const dim3 per_point((unsigned)ceil_div(N, 256)), block(256);
    hipLaunchKernelGGL(cloud_cell_keys_kernel, per_point, block, 0, ctx->stream, c, g, w.keys.as<int32_t>(), w.vals.as<int32_t>());
    HIP_TRY(ctx, hipcub::DeviceRadixSort::SortPairs(w.sort.p, sort_bytes, w.keys.as<int32_t>(), w.skeys.as<int32_t>(), w.vals.as<int32_t>(),
                                                    w.svals.as<int32_t>(), (int)N, 0, bits, ctx->stream));
    hipLaunchKernelGGL(cloud_cell_fill_kernel, per_point, block, 0, ctx->stream, c, orig, w.skeys.as<int32_t>(), w.svals.as<int32_t>(), ncells,
                       w.pts.as<GridPoint>(), w.cell_start.as<int32_t>());
    HIP_TRY(ctx, hipMemsetAsync(w.nflag.p, 0, sizeof(int32_t), ctx->stream));
    launch_knn<false>(ctx, g, N, k, w.flag.as<uint8_t>(), w.nflag.as<int32_t>(), idx, d2, pos);
    int32_t nflag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nflag, w.nflag.p, sizeof(nflag), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (nflag > 0) launch_knn<true>(ctx, g, N, k, w.flag.as<uint8_t>(), w.nflag.as<int32_t>(), idx, d2, pos);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        info->cell_size = pl.h;
        for (int d = 0; d < 3; ++d) info->grid[d] = pl.g[d];
        info->flagged = nflag;
    }
    return GINGR_OK;
}

}  // namespace

int cloud_normals_device(gingr_ctx *ctx, Cloud c, const int32_t *orig, int32_t k, const double *viewpoint, double *normals, int64_t point_stride,
                         int64_t axis_stride, double *variation, gingr_cloud_knn_info *info, const char *who) {
    GINGR_TRY(check_k(ctx, c.n, k, who));
    if (viewpoint && !(fabs(viewpoint[0]) <= kDblMax && fabs(viewpoint[1]) <= kDblMax && fabs(viewpoint[2]) <= kDblMax))
        return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite viewpoint", who);
    KnnWork w;
    DevBuf pos;
    HIP_TRY(ctx, pos.alloc((size_t)c.n * k * sizeof(int32_t)));
    GINGR_TRY(knn_search(ctx, c, orig, k, nullptr, nullptr, pos.as<int32_t>(), w, info, who));
    hipLaunchKernelGGL(cloud_normals_kernel, dim3((unsigned)ceil_div(c.n, 256)), dim3(256), 0, ctx->stream, c, (int)k, w.grid.pts, pos.as<int32_t>(),
                       viewpoint ? 1 : 0, viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0, viewpoint ? viewpoint[2] : 0.0, normals,
                       point_stride, axis_stride, variation);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the work buffers go out of scope)
    return GINGR_OK;
}

int cloud_knn_device(gingr_ctx *ctx, Cloud c, int32_t k, int32_t *idx, double *d2, gingr_cloud_knn_info *info, const char *who) {
    GINGR_TRY(check_k(ctx, c.n, k, who));
    KnnWork w;
    return knn_search(ctx, c, nullptr, k, idx, d2, nullptr, w, info, who);  // (synchronises: the work buffers go out of scope)
}

extern "C" {

int gingr_cloud_knn(gingr_ctx *ctx, int64_t N, const double *xyz, int32_t k, int32_t *idx, double *d2, gingr_cloud_knn_info *info) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!xyz || !idx) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_knn: null argument");
    GINGR_TRY(check_k(ctx, N, k, "cloud_knn"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, nk = n * (size_t)k;
    DevBuf stage, soa, didx, dd2;
    HIP_TRY(ctx, stage.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, soa.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, didx.alloc(nk * sizeof(int32_t)));
    if (d2) HIP_TRY(ctx, dd2.alloc(nk * sizeof(double)));
    GINGR_TRY(upload_cloud(ctx, stage.as<double>(), xyz, N, soa.as<double>()));
    KnnWork w;
    GINGR_TRY(knn_search(ctx, Cloud{soa.as<double>(), soa.as<double>() + N, soa.as<double>() + 2 * N, N}, nullptr, k, didx.as<int32_t>(),
                         d2 ? dd2.as<double>() : nullptr, nullptr, w, info, "cloud_knn"));
    HIP_TRY(ctx, hipMemcpyAsync(idx, didx.p, nk * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (d2) HIP_TRY(ctx, hipMemcpyAsync(d2, dd2.p, nk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_cloud_normals(gingr_ctx *ctx, int64_t N, const double *xyz, int32_t k, const double *viewpoint, double *normals, double *variation,
                        gingr_cloud_knn_info *info) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!xyz || !normals) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_normals: null argument");
    GINGR_TRY(check_k(ctx, N, k, "cloud_normals"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N;
    DevBuf stage, soa, dn, dv;
    HIP_TRY(ctx, stage.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, soa.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, dn.alloc(3 * n * sizeof(double)));
    if (variation) HIP_TRY(ctx, dv.alloc(n * sizeof(double)));
    GINGR_TRY(upload_cloud(ctx, stage.as<double>(), xyz, N, soa.as<double>()));
    GINGR_TRY(cloud_normals_device(ctx, Cloud{soa.as<double>(), soa.as<double>() + N, soa.as<double>() + 2 * N, N}, nullptr, k, viewpoint,
                                   dn.as<double>(), 3, 1, variation ? dv.as<double>() : nullptr, info, "cloud_normals"));
    HIP_TRY(ctx, hipMemcpyAsync(normals, dn.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (variation) HIP_TRY(ctx, hipMemcpyAsync(variation, dv.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

}  // extern "C"
