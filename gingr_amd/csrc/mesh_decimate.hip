// gingr_mesh_decimate: the vertex clustering of gingr_amd/simple.py: cluster_decimate on the device, bit for bit -- the same kept
// vertices and the same triangles.  Host arrays in and out, synchronises.  Stages (every kernel talks to the next one through memory
// across the launch boundary only; no grid barrier, no hand-over between workgroups inside a kernel):
//   1  bounding box (min / max partials, then one workgroup) -> the control block: lower corner, extent, the bisection's start
//   2  bisection of the cube size, the recurrence of decimate_bisect.h in the control block: per step  clear | count | step, where
//      `count` packs every vertex's cell into a 64-bit key and inserts it into an open-addressing table (compare-and-swap); a vertex
//      that claims an empty slot is a new cell, and every wave adds its new cells to the counter once.  The steps are enqueued blind,
//      GINGR_OPT_DECIMATE_BATCH of them per read-back of the control block; every launch behind the deciding step returns at once.
//   3  one more insertion at the chosen size, which also records every vertex's table slot (= its cluster)
//   4  representatives: stable radix sort of the vertex numbers by slot -> one thread per cluster adds its coordinates IN ASCENDING
//      VERTEX NUMBER (what np.bincount(weights=...) does; no floating-point atomics anywhere) -> mean -> d2 per vertex -> integer
//      atomicMin of d2's bit pattern per cluster -> integer atomicMin of the vertex number among those that attain it
//   5  compaction: flag | exclusive scan | scatter for the kept vertices (ascending number) and, after re-indexing, for the triangles;
//      triangles with the same corner set share a slot of a second table that ends up holding the lowest triangle number
// Every probe loop is bounded by its table's size; running out of it sets the control block's error word and the call fails.
#include "common.h"
#include "decimate_bisect.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 8;                           // consecutive flags per thread of the scan
constexpr int64_t kScanTile = kThreads * kScanItems;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int32_t kEmptyTri = INT32_MAX;                // triangle numbers are < INT32_MAX
constexpr uint32_t kNoSlot = 0xffffffffu;

struct DecimateCtl {
    DecimateBisect b;
    double lo[3];
    double extent;
    unsigned long long count;  // distinct cells of the insertion pass in flight
    int32_t error;             // a probe loop ran out of table
    int32_t n_kept, n_tri_out, pad;
};

__device__ inline unsigned long long hash64(unsigned long long k) { return k * 0x9E3779B97F4A7C15ull; }

// ------------------------------------------------------------------------------------------------ 1 bounding box
// part[block][6] = {min x, y, z, max x, y, z} of the block's share
__global__ __launch_bounds__(kThreads) void bbox_partial_kernel(const double *__restrict__ v, int64_t n, double *__restrict__ part) {
    __shared__ double s[6][kThreads];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        for (int d = 0; d < 3; ++d) {
            const double x = v[3 * i + d];
            lo[d] = fmin(lo[d], x);
            hi[d] = fmax(hi[d], x);
        }
    for (int d = 0; d < 3; ++d) {
        s[d][threadIdx.x] = lo[d];
        s[3 + d][threadIdx.x] = hi[d];
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int d = 0; d < 3; ++d) {
                s[d][threadIdx.x] = fmin(s[d][threadIdx.x], s[d][threadIdx.x + w]);
                s[3 + d][threadIdx.x] = fmax(s[3 + d][threadIdx.x], s[3 + d][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[(int64_t)blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kThreads) void bbox_final_kernel(const double *__restrict__ part, int nparts, DecimateCtl *ctl) {
    __shared__ double s[6][kThreads];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int p = threadIdx.x; p < nparts; p += kThreads)
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], part[(int64_t)p * 6 + d]);
            hi[d] = fmax(hi[d], part[(int64_t)p * 6 + 3 + d]);
        }
    for (int d = 0; d < 3; ++d) {
        s[d][threadIdx.x] = lo[d];
        s[3 + d][threadIdx.x] = hi[d];
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int d = 0; d < 3; ++d) {
                s[d][threadIdx.x] = fmin(s[d][threadIdx.x], s[d][threadIdx.x + w]);
                s[3 + d][threadIdx.x] = fmax(s[3 + d][threadIdx.x], s[3 + d][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int d = 0; d < 3; ++d) ctl->lo[d] = s[d][0];
        ctl->extent = decimate_extent(s[3][0] - s[0][0], s[4][0] - s[1][0], s[5][0] - s[2][0]);
        decimate_bisect_init(&ctl->b, ctl->extent);
        ctl->count = 0;
        ctl->error = 0;
        ctl->n_kept = 0;
        ctl->n_tri_out = 0;
        ctl->pad = 0;
    }
}

// ------------------------------------------------------------------------------------------------ 2 / 3 cells
// every slot empty (all ones).  mode 0: in front of a step of the bisection -- the counter to zero too, nothing to do once the
// bisection is decided;  1: unconditionally, with the counter;  2: the table alone (its second life as the per-cluster minimum)
__global__ __launch_bounds__(kThreads) void cells_clear_kernel(DecimateCtl *ctl, unsigned long long *__restrict__ table, uint64_t slots,
                                                               int mode) {
    if (mode == 0 && ctl->b.done) return;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < slots; p += (uint64_t)gridDim.x * kThreads) table[p] = kEmptyKey;
    if (mode != 2 && blockIdx.x == 0 && threadIdx.x == 0) ctl->count = 0;
}

// final == 0: count the distinct cells at the bisection's current size;  final != 0: at the chosen size, and record slot / number
__global__ __launch_bounds__(kThreads) void cells_insert_kernel(const double *__restrict__ v, int64_t n, DecimateCtl *ctl,
                                                                unsigned long long *table, int log2_slots, int final,
                                                                uint32_t *__restrict__ slot, uint32_t *__restrict__ number) {
    if (!final && ctl->b.done) return;
    const double h = final ? ctl->b.h : ctl->b.mid;
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const unsigned long long key = decimate_cell_key(v[3 * i], v[3 * i + 1], v[3 * i + 2], ctl->lo[0], ctl->lo[1], ctl->lo[2], h);
        uint64_t p = hash64(key) >> (64 - log2_slots);
        bool placed = false;
        for (uint64_t probe = 0; probe <= mask; ++probe) {
            unsigned long long cur = __atomic_load_n(&table[p], __ATOMIC_RELAXED);
            if (cur == kEmptyKey) {
                cur = atomicCAS(&table[p], kEmptyKey, key);
                if (cur == kEmptyKey) {
                    fresh = true;
                    placed = true;
                    break;
                }
            }
            if (cur == key) {
                placed = true;
                break;
            }
            p = (p + 1) & mask;
        }
        if (!placed) atomicExch(&ctl->error, 1);
        if (final) {
            slot[i] = (uint32_t)p;
            number[i] = (uint32_t)i;
        }
    }
    const unsigned long long m = __ballot(fresh);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl->count, (unsigned long long)__builtin_popcountll(m));
}

__global__ void bisect_step_kernel(DecimateCtl *ctl, int64_t n_target) {
    if (blockIdx.x == 0 && threadIdx.x == 0) decimate_bisect_step(&ctl->b, (int64_t)ctl->count, n_target);
}

// ------------------------------------------------------------------------------------------------ 4 representatives
// coordinates in sorted order (planes of stride n) and, per cluster, where its run of the sorted order ends
__global__ __launch_bounds__(kThreads) void sorted_gather_kernel(const double *__restrict__ v, int64_t n, const uint32_t *__restrict__ sslot,
                                                                 const uint32_t *__restrict__ snumber, double *__restrict__ sxyz,
                                                                 uint32_t *__restrict__ run_end) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const int64_t i = snumber[p];
    for (int d = 0; d < 3; ++d) sxyz[(int64_t)d * n + p] = v[3 * i + d];
    if (p == n - 1 || sslot[p + 1] != sslot[p]) run_end[sslot[p]] = (uint32_t)(p + 1);
}

// the first position of every run adds the run's coordinates one after the other (ascending vertex number: the sort is stable) and
// divides by the count.  The loads of a stretch of eight do not depend on the sums, so they are in flight together.
__global__ __launch_bounds__(kThreads) void cluster_mean_kernel(int64_t n, const uint32_t *__restrict__ sslot, const double *__restrict__ sxyz,
                                                                const uint32_t *__restrict__ run_end, double *__restrict__ mean,
                                                                uint64_t slots) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = sslot[p];
    if (p > 0 && sslot[p - 1] == s) return;
    const int64_t end = run_end[s];
    const double *X = sxyz, *Y = sxyz + n, *Z = sxyz + 2 * n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t q = p;
    for (; q + 8 <= end; q += 8) {
        double a[8], b[8], c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = X[q + k];
            b[k] = Y[q + k];
            c[k] = Z[q + k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sx += a[k];
            sy += b[k];
            sz += c[k];
        }
    }
    for (; q < end; ++q) {
        sx += X[q];
        sy += Y[q];
        sz += Z[q];
    }
    const double cnt = (double)(end - p);
    mean[s] = sx / cnt;
    mean[slots + s] = sy / cnt;
    mean[2 * slots + s] = sz / cnt;
}

// d2 = ((dx dx + dy dy) + dz dz) to the cluster's mean; non-negative, so its bit pattern orders like its value
__global__ __launch_bounds__(kThreads) void cluster_d2_kernel(const double *__restrict__ v, int64_t n, const uint32_t *__restrict__ slot,
                                                              const double *__restrict__ mean, uint64_t slots,
                                                              unsigned long long *__restrict__ d2bits, unsigned long long *min_bits) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot[i];
    const double dx = v[3 * i] - mean[s], dy = v[3 * i + 1] - mean[slots + s], dz = v[3 * i + 2] - mean[2 * slots + s];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
    d2bits[i] = bits;
    atomicMin(&min_bits[s], bits);
}

__global__ __launch_bounds__(kThreads) void cluster_argmin_kernel(int64_t n, const uint32_t *__restrict__ slot,
                                                                  const unsigned long long *__restrict__ d2bits,
                                                                  const unsigned long long *__restrict__ min_bits, uint32_t *min_number) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot[i];
    if (d2bits[i] == min_bits[s]) atomicMin(&min_number[s], (uint32_t)i);
}

__global__ __launch_bounds__(kThreads) void kept_flag_kernel(int64_t n, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ min_number,
                                                             int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) flag[i] = min_number[slot[i]] == (uint32_t)i ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void fill_u32_kernel(uint32_t *__restrict__ a, uint64_t count, uint32_t value) {
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < count; p += (uint64_t)gridDim.x * kThreads) a[p] = value;
}

// ------------------------------------------------------------------------------------------------ exclusive scan of 0 / 1 flags
__device__ inline int32_t block_exclusive_scan(int32_t mine, int32_t *s, int32_t *total) {  // s: kThreads ints of LDS
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 1; w < kThreads; w <<= 1) {
        const int32_t add = (int)threadIdx.x >= w ? s[threadIdx.x - w] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const int32_t incl = s[threadIdx.x];
    *total = s[kThreads - 1];
    __syncthreads();
    return incl - mine;
}

__global__ __launch_bounds__(kThreads) void scan_tile_sums_kernel(const int32_t *__restrict__ flag, int64_t n, int32_t *__restrict__ tile_sum) {
    __shared__ int32_t s[kThreads];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int32_t mine = 0;
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) mine += flag[base + k];
    int32_t total;
    (void)block_exclusive_scan(mine, s, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum -> its exclusive scan, in stretches of kThreads with a running carry; *total = the sum of all flags
__global__ __launch_bounds__(kThreads) void scan_tiles_kernel(int32_t *__restrict__ tile_sum, int64_t tiles, int32_t *total_out) {
    __shared__ int32_t s[kThreads];
    int32_t carry = 0;
    for (int64_t base = 0; base < tiles; base += kThreads) {
        const int64_t t = base + threadIdx.x;
        const int32_t mine = t < tiles ? tile_sum[t] : 0;
        int32_t total;
        const int32_t excl = block_exclusive_scan(mine, s, &total);
        if (t < tiles) tile_sum[t] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(const int32_t *__restrict__ flag, int64_t n, const int32_t *__restrict__ tile_sum,
                                                              int32_t *__restrict__ pos) {
    __shared__ int32_t s[kThreads];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int32_t f[kScanItems], mine = 0;
    for (int k = 0; k < kScanItems; ++k) {
        f[k] = base + k < n ? flag[base + k] : 0;
        mine += f[k];
    }
    int32_t total;
    int32_t run = tile_sum[blockIdx.x] + block_exclusive_scan(mine, s, &total);
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) {
            pos[base + k] = run;
            run += f[k];
        }
}

// ------------------------------------------------------------------------------------------------ 5 compaction
__global__ __launch_bounds__(kThreads) void kept_scatter_kernel(int64_t n, const uint32_t *__restrict__ slot, const int32_t *__restrict__ flag,
                                                                const int32_t *__restrict__ pos, int32_t *__restrict__ kept,
                                                                uint32_t *__restrict__ new_id) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !flag[i]) return;
    kept[pos[i]] = (int32_t)i;
    new_id[slot[i]] = (uint32_t)pos[i];
}

__global__ __launch_bounds__(kThreads) void tri_reindex_kernel(int64_t T, const int32_t *__restrict__ tri, const uint32_t *__restrict__ slot,
                                                               const uint32_t *__restrict__ new_id, int32_t *__restrict__ rtri) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < 3 * T) rtri[k] = (int32_t)new_id[slot[tri[k]]];
}

struct Triple {
    int32_t a, b, c;  // ascending
};
__device__ inline Triple sorted_triple(const int32_t *__restrict__ rtri, int64_t t) {
    int32_t a = rtri[3 * t], b = rtri[3 * t + 1], c = rtri[3 * t + 2], x;
    if (a > b) { x = a; a = b; b = x; }
    if (b > c) { x = b; b = c; c = x; }
    if (a > b) { x = a; a = b; b = x; }
    return Triple{a, b, c};
}

// A slot of the table holds a triangle NUMBER; its corner set is that triangle's.  The first triangle of a set claims an empty slot,
// every other one of the same set lowers the number with atomicMin -- the slot stays with the set, so the probe sequences of all
// others are unaffected.  tslot[t] = where the set of triangle t lives (kNoSlot: a collapsed triangle, which never enters).
__global__ __launch_bounds__(kThreads) void tri_insert_kernel(int64_t T, const int32_t *__restrict__ rtri, int32_t *table, int log2_slots,
                                                              uint32_t *__restrict__ tslot, DecimateCtl *ctl) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const Triple me = sorted_triple(rtri, t);
    if (me.a == me.b || me.b == me.c) {
        tslot[t] = kNoSlot;
        return;
    }
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    unsigned long long hk = hash64((unsigned long long)(uint32_t)me.a);
    hk = hash64(hk ^ (unsigned long long)(uint32_t)me.b);
    hk = hash64(hk ^ (unsigned long long)(uint32_t)me.c);
    uint64_t p = hk >> (64 - log2_slots);
    for (uint64_t probe = 0; probe <= mask; ++probe) {
        int32_t cur = __atomic_load_n(&table[p], __ATOMIC_RELAXED);
        if (cur == kEmptyTri) {
            cur = atomicCAS(&table[p], kEmptyTri, (int32_t)t);
            if (cur == kEmptyTri) {
                tslot[t] = (uint32_t)p;
                return;
            }
        }
        const Triple other = sorted_triple(rtri, cur);
        if (other.a == me.a && other.b == me.b && other.c == me.c) {
            atomicMin(&table[p], (int32_t)t);
            tslot[t] = (uint32_t)p;
            return;
        }
        p = (p + 1) & mask;
    }
    tslot[t] = kNoSlot;
    atomicExch(&ctl->error, 2);
}

__global__ __launch_bounds__(kThreads) void tri_flag_kernel(int64_t T, const uint32_t *__restrict__ tslot, const int32_t *__restrict__ table,
                                                            int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < T) flag[t] = (tslot[t] != kNoSlot && table[tslot[t]] == (int32_t)t) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void tri_scatter_kernel(int64_t T, const int32_t *__restrict__ rtri, const int32_t *__restrict__ flag,
                                                               const int32_t *__restrict__ pos, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T || !flag[t]) return;
    for (int d = 0; d < 3; ++d) out[3 * (int64_t)pos[t] + d] = rtri[3 * t + d];
}

// ------------------------------------------------------------------------------------------------ host side
unsigned blocks_for(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, kThreads); }
unsigned fill_blocks(uint64_t count) {
    const uint64_t b = (count + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
int log2_slots_for(int64_t n) {  // the smallest power of two >= 2 n, at least 64 slots
    int b = 6;
    while (((int64_t)1 << b) < 2 * n) ++b;
    return b;
}

// pos = exclusive scan of flag, *total = the number of set flags; tile_sum: ceil(n / kScanTile) ints
void launch_flag_scan(gingr_ctx *ctx, const int32_t *flag, int64_t n, int32_t *tile_sum, int32_t *pos, int32_t *total) {
    const int64_t tiles = ceil_div(n, kScanTile);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, flag, n, tile_sum);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, tile_sum, tiles, total);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, flag, n, tile_sum, pos);
}

}  // namespace

extern "C" int gingr_mesh_decimate(gingr_ctx *ctx, int64_t n_vertices, const double *vertices, int64_t n_triangles,
                                   const int32_t *triangles, int64_t n_target, int64_t *n_kept, int32_t *kept_ids,
                                   int64_t *n_out_triangles, int32_t *out_triangles, double *cube_size) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (n_target < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: n_target must be >= 1");
    if (n_vertices < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: n_vertices must be >= 1");
    if (n_vertices > INT32_MAX) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: n_vertices exceeds the int32 index range");
    if (!vertices || !n_kept || !kept_ids)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: vertices, n_kept and kept_ids must not be NULL");
    const int64_t n = n_vertices, T = triangles ? n_triangles : 0;
    if (triangles && (n_triangles < 0 || n_triangles >= INT32_MAX || !n_out_triangles || !out_triangles))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: bad triangle arguments");
    for (int64_t k = 0; k < 3 * T; ++k)
        if (triangles[k] < 0 || triangles[k] >= n)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: triangle %lld has a vertex id out of range (%d)",
                                   (long long)(k / 3), (int)triangles[k]);
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(vertices[k]))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: coordinate %d of vertex %lld is not finite", (int)(k % 3),
                                   (long long)(k / 3));
    if (n_out_triangles) *n_out_triangles = 0;
    if (cube_size) *cube_size = 0.0;
    if (n_target >= n) {  // the identity: every vertex, the triangles untouched (collapsed and repeated ones included)
        for (int64_t i = 0; i < n; ++i) kept_ids[i] = (int32_t)i;
        *n_kept = n;
        if (triangles) {
            memcpy(out_triangles, triangles, (size_t)(3 * T) * sizeof(int32_t));
            *n_out_triangles = T;
        }
        return GINGR_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int lg = log2_slots_for(n);
    const uint64_t slots = (uint64_t)1 << lg;
    const int nparts = (int)(blocks_for(n) < 256u ? blocks_for(n) : 256u);
    const int64_t scan_n = n > T ? n : T;
    DevBuf dv, dctl, dpart, dtable, dslot, dnumber, dsslot, dsnumber, dsort, dsxyz, drun, dmean, dd2, dminnum, dflag, dpos, dtiles, dkept, dnewid;
    HIP_TRY(ctx, dv.alloc((size_t)(3 * n) * sizeof(double)));
    HIP_TRY(ctx, dctl.alloc(sizeof(DecimateCtl)));
    HIP_TRY(ctx, dpart.alloc((size_t)nparts * 6 * sizeof(double)));
    HIP_TRY(ctx, dtable.alloc((size_t)slots * sizeof(unsigned long long)));
    HIP_TRY(ctx, dslot.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(ctx, dnumber.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(ctx, dflag.alloc((size_t)scan_n * sizeof(int32_t)));
    HIP_TRY(ctx, dpos.alloc((size_t)scan_n * sizeof(int32_t)));
    HIP_TRY(ctx, dtiles.alloc((size_t)ceil_div(scan_n, kScanTile) * sizeof(int32_t)));
    DecimateCtl *ctl = dctl.as<DecimateCtl>();
    const double *v = dv.as<double>();
    unsigned long long *table = dtable.as<unsigned long long>();
    HIP_TRY(ctx, hipMemcpyAsync(dv.p, vertices, (size_t)(3 * n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    DecimateCtl hc;
    {
        TimerScope ts(ctx, 13);
        hipLaunchKernelGGL(bbox_partial_kernel, dim3((unsigned)nparts), dim3(kThreads), 0, ctx->stream, v, n, dpart.as<double>());
        hipLaunchKernelGGL(bbox_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, dpart.as<double>(), nparts, ctl);
    }
    // ---- bisection: the recurrence lives in the control block; the host only learns whether it is decided
    const int batch = ctx->decimate_batch < 1 ? 1 : ctx->decimate_batch;
    for (int enqueued = 0;;) {
        {
            TimerScope ts(ctx, 14);
            for (int k = 0; k < batch && enqueued < GINGR_DECIMATE_MAX_STEPS; ++k, ++enqueued) {
                hipLaunchKernelGGL(cells_clear_kernel, dim3(fill_blocks(slots)), dim3(kThreads), 0, ctx->stream, ctl, table, slots, 0);
                hipLaunchKernelGGL(cells_insert_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, v, n, ctl, table, lg, 0,
                                   (uint32_t *)nullptr, (uint32_t *)nullptr);
                hipLaunchKernelGGL(bisect_step_kernel, dim3(1), dim3(1), 0, ctx->stream, ctl, n_target);
            }
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&hc, ctl, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (!std::isfinite(hc.extent))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_decimate: the extent of the vertices overflows");
        if (hc.error) return gingr_set_error(ctx, GINGR_ERR_STATE, "mesh_decimate: the cell table ran full (internal error %d)", hc.error);
        if (hc.b.done) break;
        if (enqueued >= GINGR_DECIMATE_MAX_STEPS)
            return gingr_set_error(ctx, GINGR_ERR_STATE, "mesh_decimate: the bisection did not end (internal error)");
    }
    // ---- clusters at the chosen size
    HIP_TRY(ctx, dsslot.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(ctx, dsnumber.alloc((size_t)n * sizeof(uint32_t)));
    size_t sort_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)n, 0, lg, ctx->stream);
    HIP_TRY(ctx, dsort.alloc(sort_bytes));
    HIP_TRY(ctx, dsxyz.alloc((size_t)(3 * n) * sizeof(double)));
    HIP_TRY(ctx, drun.alloc((size_t)slots * sizeof(uint32_t)));
    HIP_TRY(ctx, dmean.alloc((size_t)(3 * slots) * sizeof(double)));
    HIP_TRY(ctx, dd2.alloc((size_t)n * sizeof(unsigned long long)));
    HIP_TRY(ctx, dminnum.alloc((size_t)slots * sizeof(uint32_t)));
    HIP_TRY(ctx, dkept.alloc((size_t)n * sizeof(int32_t)));
    HIP_TRY(ctx, dnewid.alloc((size_t)slots * sizeof(uint32_t)));
    uint32_t *slot = dslot.as<uint32_t>();
    {
        TimerScope ts(ctx, 15);
        hipLaunchKernelGGL(cells_clear_kernel, dim3(fill_blocks(slots)), dim3(kThreads), 0, ctx->stream, ctl, table, slots, 1);
        hipLaunchKernelGGL(cells_insert_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, v, n, ctl, table, lg, 1, slot,
                           dnumber.as<uint32_t>());
        // stable LSD radix sort over the bits a slot can have: equal slots keep ascending vertex numbers
        if (hipcub::DeviceRadixSort::SortPairs(dsort.p, sort_bytes, (const uint32_t *)slot, dsslot.as<uint32_t>(),
                                               (const uint32_t *)dnumber.as<uint32_t>(), dsnumber.as<uint32_t>(), (int)n, 0, lg,
                                               ctx->stream) != hipSuccess)
            return gingr_set_error(ctx, GINGR_ERR_HIP, "mesh_decimate: the radix sort failed");
        hipLaunchKernelGGL(sorted_gather_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, v, n, dsslot.as<uint32_t>(),
                           dsnumber.as<uint32_t>(), dsxyz.as<double>(), drun.as<uint32_t>());
        hipLaunchKernelGGL(cluster_mean_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, dsslot.as<uint32_t>(),
                           dsxyz.as<double>(), drun.as<uint32_t>(), dmean.as<double>(), slots);
        // the cell table has done its work: its memory is the per-cluster minimum of d2's bit pattern from here on
        hipLaunchKernelGGL(cells_clear_kernel, dim3(fill_blocks(slots)), dim3(kThreads), 0, ctx->stream, ctl, table, slots, 2);
        hipLaunchKernelGGL(fill_u32_kernel, dim3(fill_blocks(slots)), dim3(kThreads), 0, ctx->stream, dminnum.as<uint32_t>(), slots, kNoSlot);
        hipLaunchKernelGGL(cluster_d2_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, v, n, slot, dmean.as<double>(), slots,
                           dd2.as<unsigned long long>(), table);
        hipLaunchKernelGGL(cluster_argmin_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, slot,
                           dd2.as<unsigned long long>(), table, dminnum.as<uint32_t>());
    }
    DevBuf drtri, dtri, dttable, dtslot, dout;
    int32_t *flag = dflag.as<int32_t>(), *pos = dpos.as<int32_t>();
    {
        TimerScope ts(ctx, 16);
        hipLaunchKernelGGL(kept_flag_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, slot, dminnum.as<uint32_t>(), flag);
        launch_flag_scan(ctx, flag, n, dtiles.as<int32_t>(), pos, &ctl->n_kept);
        hipLaunchKernelGGL(kept_scatter_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, slot, flag, pos, dkept.as<int32_t>(),
                           dnewid.as<uint32_t>());
        if (T > 0) {
            int lt = 6;
            while (((int64_t)1 << lt) < 2 * T) ++lt;
            const uint64_t tslots = (uint64_t)1 << lt;
            HIP_TRY(ctx, dtri.alloc((size_t)(3 * T) * sizeof(int32_t)));
            HIP_TRY(ctx, drtri.alloc((size_t)(3 * T) * sizeof(int32_t)));
            HIP_TRY(ctx, dttable.alloc((size_t)tslots * sizeof(int32_t)));
            HIP_TRY(ctx, dtslot.alloc((size_t)T * sizeof(uint32_t)));
            HIP_TRY(ctx, dout.alloc((size_t)(3 * T) * sizeof(int32_t)));
            HIP_TRY(ctx, hipMemcpyAsync(dtri.p, triangles, (size_t)(3 * T) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(tri_reindex_kernel, dim3(blocks_for(3 * T)), dim3(kThreads), 0, ctx->stream, T, dtri.as<int32_t>(), slot,
                               dnewid.as<uint32_t>(), drtri.as<int32_t>());
            hipLaunchKernelGGL(fill_u32_kernel, dim3(fill_blocks(tslots)), dim3(kThreads), 0, ctx->stream, dttable.as<uint32_t>(), tslots,
                               (uint32_t)kEmptyTri);
            hipLaunchKernelGGL(tri_insert_kernel, dim3(blocks_for(T)), dim3(kThreads), 0, ctx->stream, T, drtri.as<int32_t>(),
                               dttable.as<int32_t>(), lt, dtslot.as<uint32_t>(), ctl);
            hipLaunchKernelGGL(tri_flag_kernel, dim3(blocks_for(T)), dim3(kThreads), 0, ctx->stream, T, dtslot.as<uint32_t>(),
                               dttable.as<int32_t>(), flag);
            launch_flag_scan(ctx, flag, T, dtiles.as<int32_t>(), pos, &ctl->n_tri_out);
            hipLaunchKernelGGL(tri_scatter_kernel, dim3(blocks_for(T)), dim3(kThreads), 0, ctx->stream, T, drtri.as<int32_t>(), flag, pos,
                               dout.as<int32_t>());
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&hc, ctl, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hc.error) return gingr_set_error(ctx, GINGR_ERR_STATE, "mesh_decimate: a hash table ran full (internal error %d)", hc.error);
    if (hc.n_kept < 1 || hc.n_kept > n || (int64_t)hc.count != (int64_t)hc.n_kept || hc.n_tri_out < 0 || hc.n_tri_out > T)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "mesh_decimate: inconsistent counts (clusters %lld, kept %d, triangles %d)",
                               (long long)hc.count, hc.n_kept, hc.n_tri_out);
    HIP_TRY(ctx, hipMemcpyAsync(kept_ids, dkept.p, (size_t)hc.n_kept * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (hc.n_tri_out > 0)
        HIP_TRY(ctx, hipMemcpyAsync(out_triangles, dout.p, (size_t)(3 * (int64_t)hc.n_tri_out) * sizeof(int32_t), hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_kept = hc.n_kept;
    if (n_out_triangles) *n_out_triangles = hc.n_tri_out;
    if (cube_size) *cube_size = hc.b.h;
    return GINGR_OK;
}
