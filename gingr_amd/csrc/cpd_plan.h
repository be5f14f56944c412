// The host-side planners of the all-pairs launches: which kernel instance (points per thread) a CPD pass takes, how its streamed
// side is cut into chunks, and the chunking of the nearest-neighbour scans.  Every threshold in here was measured.  No HIP in here:
// cpd_pairs.hip / nn_scan.hip launch by these plans (the occupancy query that yields `resident` stays there),
// tests/c/cpd_plan_driver.cpp runs them on the host under the sanitizers.
#pragma once
#include <cstdint>

#include "host_device.h"

constexpr int kTile = 256;      // points of a streamed tile = of a k-d leaf = of a culling box (four 64-point quarters)
constexpr int kNNThreads = 64;  // queries per workgroup of the nearest-neighbour scan

// The streamed side of an all-pairs launch is cut into chunks (one workgroup per owned block and chunk): n_big chunks of len_big
// points, then chunks of len_tail points.  Long chunks first and short ones last shorten the tail of the launch (the last
// workgroups to be dispatched are the cheap ones) without multiplying the per-chunk partials; len_tail == len_big is the uniform cut.
struct ChunkPlan {
    int64_t len_big, len_tail;
    int32_t n_big;
    int32_t fair = 0;  // one launch round: waves lower their issue priority as they advance (fair_priority)
    GINGR_HD void range(int64_t y, int64_t n, int64_t *b, int64_t *e) const {
        const int64_t lo = y < n_big ? y * len_big : (int64_t)n_big * len_big + (y - n_big) * len_tail;
        const int64_t hi = lo + (y < n_big ? len_big : len_tail);
        *b = lo;
        *e = hi < n ? hi : n;
    }
    int chunks(int64_t n) const {
        const int64_t head = (int64_t)n_big * len_big;
        if (head >= n) return (int)((n + len_big - 1) / len_big);
        return n_big + (int)((n - head + len_tail - 1) / len_tail);
    }
};

#ifndef GINGR_PT
#define GINGR_PT 4
#endif
#define GINGR_PT_DEFAULT GINGR_PT
constexpr int kPT = GINGR_PT_DEFAULT;     // points per thread in both CPD passes
// Row statistics of a TINY shard: two points per thread halve the workgroup's rows (more workgroups along the row axis, a fourth
// workgroup per CU).  With round 2's work split (a workgroup owns 256 rows whatever PT is) four points per thread win from a few
// thousand rows on: 8-GPU shard of the 50k workload (6250 rows) 0.50 ms per iteration with PT = 2, 0.49 ms with PT = 4.
#ifndef GINGR_SMALL_COLSUM_COLS
#define GINGR_SMALL_COLSUM_COLS 16384
#endif
#ifndef GINGR_SMALL_SHARD_ROWS
#define GINGR_SMALL_SHARD_ROWS 2048
#endif
constexpr int64_t kSmallShardRows = GINGR_SMALL_SHARD_ROWS;
constexpr int64_t kSmallColsumCols = GINGR_SMALL_COLSUM_COLS;
constexpr int64_t kTinyCols = 2048;
// Build-time knobs of the chunk planner (the sweeps behind the defaults: tools/chunk_sweep.sh, tools/small_chunk_sweep.sh build the
// library with -DGINGR_...=v through tools/abn.sh; none of them is read from the environment):
//   GINGR_ROWSTATS_PT        2 or 4 points per thread in the row-statistics pass whatever the shard size (0: by shard size)
//   GINGR_COLSUM_QUARTERS / GINGR_ROWSTATS_QUARTERS   fixed chunk length in 64-point quarters (0: planner)
//   GINGR_COLSUM_CHUNKS / GINGR_ROWSTATS_CHUNKS       exactly n chunks balanced to a quarter (0: planner)
//   GINGR_FAIR_PRIORITY      0 never, 1 in one-round launches (default), 2 always: waves lower their issue priority as they advance
#ifndef GINGR_ROWSTATS_PT
#define GINGR_ROWSTATS_PT 0
#endif
#ifndef GINGR_COLSUM_QUARTERS
#define GINGR_COLSUM_QUARTERS 0
#endif
#ifndef GINGR_ROWSTATS_QUARTERS
#define GINGR_ROWSTATS_QUARTERS 0
#endif
#ifndef GINGR_COLSUM_CHUNKS
#define GINGR_COLSUM_CHUNKS 0
#endif
#ifndef GINGR_ROWSTATS_CHUNKS
#define GINGR_ROWSTATS_CHUNKS 0
#endif
#ifndef GINGR_FAIR_PRIORITY
#define GINGR_FAIR_PRIORITY 1
#endif
#ifndef GINGR_COLSUM_PT
#define GINGR_COLSUM_PT 0
#endif
// owned points (targets) per thread of the column-sum pass: small target clouds take 2, tiny ones 1 -- two / four times the
// workgroups of a launch that fills a fifth of the chip at femur size (GINGR_COLSUM_PT: build-time override for the sweep)
inline int colsum_pt(int64_t cols) {
    constexpr int forced = GINGR_COLSUM_PT;
    if (forced == 1 || forced == 2 || forced == kPT) return forced;
    if (kPT > 2 && cols <= kTinyCols) return 1;  // femur size: 0.0973 -> 0.0950 ms per iteration against 2
    return (kPT > 2 && cols <= kSmallColsumCols) ? 2 : kPT;
}
// owned points (rows) per thread of the row-statistics pass: 1 where both clouds are tiny (femur), 2 on short shards (few row blocks whatever the target count) and on
// problems that are small on BOTH sides (15k x 15k: 0.354 -> 0.348 ms; a 6 250-row shard of 50k targets is slower with 2: 0.421 -> 0.435)
inline int rowstats_pt(int64_t rows, int64_t cols) {
    constexpr int forced = GINGR_ROWSTATS_PT;
    if (forced == 1 || forced == 2 || forced == kPT) return forced;
    if (kPT > 2 && rows <= kTinyCols && cols <= kTinyCols) return 1;  // femur size: 0.0950 -> 0.0932 ms per iteration against 2
    return (kPT > 2 && (rows <= kSmallShardRows || (rows <= kSmallColsumCols && cols <= kSmallColsumCols))) ? 2 : kPT;
}
// Workgroups per all-pairs launch.  A CU holds 3-4 of them and one lives for (tiles per chunk) x ~30 us, so the launch ends with
// a tail of about one workgroup's life: many short workgroups beat few long ones until the per-chunk partials (written here,
// read by the reduce kernels) cost more than the tail.  Measured with GINGR_COLSUM_TILES / GINGR_ROWSTATS_TILES at 50k <-> 50k
// on shards of 1/1, 1/2, 1/4, 1/8 of the rows (profiles/r01_chunk_length_sweep.txt): two tiles per chunk (~4900 workgroups)
// is 5 % faster than five (~2000) on the whole cloud, one tile is best on the shards.
constexpr int kTargetBlocks = 5120;
#ifndef GINGR_MIN_CHUNK
#define GINGR_MIN_CHUNK 256
#endif
constexpr int kMinChunk = GINGR_MIN_CHUNK;  // shortest chunk the planner picks by itself (64, 128 or 256 points)

// split `stream_len` into chunks so that block_cols * nchunks ~ kTargetBlocks.  A chunk is a whole number of tiles, or -- when
// even one tile per chunk leaves too few workgroups (small shards) -- a half or a quarter of a tile: 64-point quarters are the
// unit of the culling boxes, and a chunk that divides a tile never straddles two tiles' boxes.
// `quarters_override` > 0 (build-time knob GINGR_COLSUM_QUARTERS / GINGR_ROWSTATS_QUARTERS) fixes the chunk length.
// `resident` = resident workgroups of the chip for the launch's kernel (compute units x workgroups per unit; 0: unknown).  Launches
// come in rounds of that many workgroups and the last, partly filled round costs almost a full one (measured at 50k x 50k:
// 4.79 -> 4.98 rounds of the column-sum pass is 2.7 % FASTER, 6.38 -> 5.87 rounds of the row-statistics pass 3 %), so the planner
// makes the number of workgroups come out just under a whole number of rounds.
inline ChunkPlan plan_chunks(int64_t owned, int owned_per_block, int64_t stream_len, int *nchunks, int quarters_override = 0,
                             int forced_chunks = 0, int resident = 0) {
    const int64_t bx = ceil_div(owned, owned_per_block);
    int64_t want = ceil_div(kTargetBlocks, bx > 0 ? bx : 1);
    if (want < 1) want = 1;
    const int64_t n = stream_len > 0 ? stream_len : 1;
    int64_t len = round_up(ceil_div(n, want), 64);
    if (quarters_override > 0) len = (int64_t)quarters_override * 64;
    if (len >= kTile)
        len = round_up(len, kTile);
    else if (len > 128)
        len = kTile;
    else if (len > 64)
        len = 128;
    else
        len = 64;
    if (quarters_override <= 0 && len < kMinChunk) len = kMinChunk;
    ChunkPlan p{len, len, (int32_t)ceil_div(n, len), 0};
    // build-time knobs GINGR_COLSUM_CHUNKS / GINGR_ROWSTATS_CHUNKS=<n>: exactly n chunks balanced to a 64-point quarter (lengths
    // differ by at most 64; the kernels handle chunks that start inside a tile).  Default (no knob, `resident` known): the
    // largest chunk count whose workgroups fill k whole launch rounds, k = kTargetBlocks / resident rounded, with the same
    // balanced lengths.
    int forced = forced_chunks;
    if (forced <= 0 && quarters_override <= 0 && resident > 0) {
        // rounds: as many as kTargetBlocks asks for (finer balancing when culling makes workgroup costs uneven), but not so many that
        // a chunk drops below ~1024 streamed points -- every workgroup pays ~3-4 us of prologue (table fill, owned points, boxes),
        // which short chunks do not amortise (8-GPU shard of the 50k workload: 0.52 -> 0.49 ms per iteration with one round)
        int64_t k = (kTargetBlocks + resident / 2) / resident;
        const int64_t kmax = (n / 1024) * (bx > 0 ? bx : 1) / resident;
        if (k > kmax) k = kmax;
        if (k < 1) k = 1;
        int64_t nc = k * resident / (bx > 0 ? bx : 1);
        const int64_t Qmax = ceil_div(n, 64);
        if (nc > Qmax) nc = Qmax;
        if (nc < 1) nc = 1;
        // Short chunks stay whole tiles: wave q works on quarter q of every tile part, so a chunk of 3 quarters leaves one wave
        // idle; only from ~16 quarters per chunk on is the unevenness (one quarter per wave at most) small against the round gain
        // (emulated 8-GPU shard: 0.517 ms with tile-aligned chunks, 0.530 ms with balanced 192/256-point chunks).
        if (Qmax / nc >= 16) forced = (int)nc;
    }
    if (forced > 0) {
        const int64_t Q = ceil_div(n, 64), q = Q / forced, rem = Q % forced;
        if (q >= 1) {
            p.len_big = (q + 1) * 64;
            p.len_tail = q * 64;
            p.n_big = (int32_t)rem;
            if (rem == 0) {
                p.len_big = p.len_tail;
                p.n_big = forced;
            }
        }
    }
    *nchunks = p.chunks(n);
    constexpr int fair_env = GINGR_FAIR_PRIORITY;
    p.fair = (fair_env == 2 || (fair_env == 1 && resident > 0 && (int64_t)*nchunks * bx <= resident)) ? 1 : 0;
    return p;
}

// What a launch of one of the two CPD passes over M fit points x N targets needs to know.  colsum_plan / rowstats_plan are the ONLY
// callers of plan_chunks for the passes: the workspace sizes and the launchers go through them, so a workspace sized here and a grid
// launched there cannot disagree.
struct PairPlan {
    ChunkPlan plan;
    int nch;  // chunks of the streamed side = gridDim.y = chunk partials left in the workspace
    int pt;   // owned points per thread: the kernel instance; a workgroup owns 64 * pt points
};
// column sums: the N targets are owned, the M fit points streamed.  forced_chunks > 0: exactly that many chunks (launch_cpd_colsum)
inline PairPlan colsum_plan(int64_t M, int64_t N, int forced_chunks, int resident) {
    PairPlan r;
    r.pt = colsum_pt(N);
    r.plan = plan_chunks(N, 64 * r.pt, M, &r.nch, GINGR_COLSUM_QUARTERS, forced_chunks > 0 ? forced_chunks : GINGR_COLSUM_CHUNKS, resident);
    return r;
}
// row statistics: the M fit points are owned, the N targets streamed.  `resident` is that of the instance rowstats_pt(M, N) picks.
inline PairPlan rowstats_plan(int64_t M, int64_t N, int resident) {
    PairPlan r;
    r.pt = rowstats_pt(M, N);
    r.plan = plan_chunks(M, 64 * r.pt, N, &r.nch, GINGR_ROWSTATS_QUARTERS, GINGR_ROWSTATS_CHUNKS, resident);
    return r;
}
// workspaces (in doubles) of the two passes at the planner's own chunk count: [chunk][N] column sums, [chunk][4][M] row statistics
inline int64_t colsum_ws_doubles(int64_t M, int64_t N, int resident) { return (int64_t)colsum_plan(M, N, 0, resident).nch * N; }
inline int64_t rowstats_ws_doubles(int64_t M, int64_t N, int resident) { return (int64_t)rowstats_plan(M, N, resident).nch * 4 * M; }

// chunks of the target cloud in the exact nearest-neighbour scan (nn_scan.hip: nn_kernel), a whole number of tiles each
inline void plan_nn(int64_t nq, int64_t nt_points, bool pruned, int *nchunks, int64_t *chunk_len) {
    const int64_t bx = ceil_div(nq, kNNThreads);
    // Splitting the targets into chunks weakens the pruning (a chunk far from the queries has no near tile to shrink the
    // bound), so with pruning chunks are only used when there are too few query waves to occupy the chip; the full scan
    // wants ~8 waves per CU.
    int64_t want = pruned ? (bx >= 256 ? 1 : ceil_div(512, bx > 0 ? bx : 1)) : ceil_div(2048, bx > 0 ? bx : 1);
    const int64_t max_chunks = ceil_div(nt_points, kTile);
    if (want > max_chunks) want = max_chunks;
    if (want < 1) want = 1;
    int64_t len = round_up(ceil_div(nt_points, want), kTile);
    if (len < kTile) len = kTile;
    *chunk_len = len;
    *nchunks = (int)ceil_div(nt_points > 0 ? nt_points : 1, len);
}

// target slices of the small all-pairs scan (nn_scan.hip: nn_small_kernel)
#ifndef GINGR_NN_SMALL_WGS
#define GINGR_NN_SMALL_WGS 768
#endif
inline int nn_small_slices(int64_t M, int64_t N) {
    const int64_t groups = ceil_div(M, 512);
    int64_t s = GINGR_NN_SMALL_WGS / (groups > 0 ? groups : 1);  // at most three workgroups (12 waves) per compute unit: no fourth round
    const int64_t max_s = ceil_div(N, 32);               // at least 32 targets per slice
    if (s > max_s) s = max_s;
    const int64_t min_s = ceil_div(N, 2048);             // at most 2 048 targets (48 KB of LDS) per slice
    if (s < min_s) s = min_s;
    return (int)(s < 1 ? 1 : s);
}
