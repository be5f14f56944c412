// Planning of the model metrics (model_metrics.hip): column blocks, column chunks and vertex slabs of the batched instance, projection
// and sample-against-shape passes.  Plain C++ (compiled for the host alone by tests/test_model_metrics_host.py).
//
// Columns.  A batch of shapes, coefficient vectors or (shape, rank) pairs is a block of columns in the basis layout [3 M + kRowSlack][cols],
// cols a multiple of 16 (one MFMA tile).  A workgroup of the MFMA passes takes a chunk of kChunkCols columns; what is stored goes through
// the device in blocks of at most kMaxBlockCols columns.
// Vertices.  Every pass cuts the M vertices into slabs and leaves one partial per slab and column (or pair), which a finish kernel adds in
// ascending slab order: the slab boundaries depend on M and on the number of columns (or pairs) alone.  Every slab holds vertices; the
// last may be shorter.
#pragma once

#include "host_device.h"

namespace model_metrics_plan {

constexpr int64_t kRowSlack = 48;        // zero rows behind a block of columns: the MFMA passes fetch whole 16-row steps past M
constexpr int64_t kTileCols = 16;        // columns of an MFMA tile
constexpr int64_t kChunkCols = 64;       // columns of a workgroup of the MFMA passes (four tiles)
constexpr int64_t kMaxBlockCols = 512;   // columns stored at a time
constexpr int64_t kMaxShapes = 512;      // shapes of a generalization call, training shapes of a specificity call
constexpr int64_t kMaxRanks = 16;
constexpr int64_t kGroupVerts = 128;     // vertices a workgroup of the measure pass takes per step: eight waves of 16
constexpr int64_t kMeasureTarget = 1024; // workgroups the measure pass aims at
constexpr int64_t kPairTile = 64;        // a workgroup of the pair pass: 64 sample columns x 64 training columns, 4 x 4 per lane
constexpr int64_t kPairVerts = 32;       // granularity of a slab of the pair pass
constexpr int64_t kPairTarget = 2048;    // workgroups the pair pass aims at
constexpr int64_t kMaxPartialDoubles = (int64_t)1 << 24;  // the slab partials of the pair pass at most (128 MB)

inline int64_t padded_cols(int64_t n) { return round_up(n, kTileCols); }
inline int64_t block_rows(int64_t M) { return 3 * M + kRowSlack; }

// n columns in blocks of at most kMaxBlockCols
struct ColumnBlocks {
    int64_t n = 0, count = 0;
    int64_t begin(int64_t b) const { return b * kMaxBlockCols; }
    int64_t length(int64_t b) const { return (b + 1) * kMaxBlockCols < n ? kMaxBlockCols : n - b * kMaxBlockCols; }
    int64_t padded(int64_t b) const { return padded_cols(length(b)); }
};
inline ColumnBlocks column_blocks(int64_t n) {
    ColumnBlocks c;
    c.n = n;
    c.count = n > 0 ? ceil_div(n, kMaxBlockCols) : 0;
    return c;
}

// the measure pass (reconstruct and measure): slabs of whole kGroupVerts-vertex groups x chunks of kChunkCols columns
struct MeasurePlan {
    int64_t M = 0, cols = 0;  // cols: padded
    int64_t chunks = 0, verts_per_slab = 0, slabs = 0;
    int64_t slab_begin(int64_t s) const { return s * verts_per_slab; }
    int64_t slab_end(int64_t s) const { return (s + 1) * verts_per_slab < M ? (s + 1) * verts_per_slab : M; }
    int64_t workgroups() const { return slabs * chunks; }
    int64_t partial_doubles() const { return slabs * 2 * cols; }  // per slab: the sums, then the maxima
};
inline MeasurePlan make_measure_plan(int64_t M, int64_t cols) {
    MeasurePlan p;
    p.M = M;
    p.cols = padded_cols(cols);
    p.chunks = ceil_div(p.cols, kChunkCols);
    const int64_t groups = ceil_div(M, kGroupVerts);
    int64_t want = ceil_div(kMeasureTarget, p.chunks > 0 ? p.chunks : 1);
    if (want > groups) want = groups;
    if (want < 1) want = 1;
    p.verts_per_slab = round_up(ceil_div(M, want), kGroupVerts);
    p.slabs = ceil_div(M, p.verts_per_slab);
    return p;
}

// the pair pass (samples against training shapes): slabs of vertices x tiles of kPairTile x kPairTile pairs
struct PairPlan {
    int64_t M = 0, sp = 0, tp = 0;  // padded sample and training columns
    int64_t tiles_s = 0, tiles_t = 0, verts_per_slab = 0, slabs = 0;
    int64_t slab_begin(int64_t s) const { return s * verts_per_slab; }
    int64_t slab_end(int64_t s) const { return (s + 1) * verts_per_slab < M ? (s + 1) * verts_per_slab : M; }
    int64_t tiles() const { return tiles_s * tiles_t; }
    int64_t partial_doubles() const { return slabs * sp * tp; }  // [slab][training column][sample column]
};
inline PairPlan make_pair_plan(int64_t M, int64_t samples, int64_t train) {
    PairPlan p;
    p.M = M;
    p.sp = padded_cols(samples);
    p.tp = padded_cols(train);
    p.tiles_s = ceil_div(p.sp, kPairTile);
    p.tiles_t = ceil_div(p.tp, kPairTile);
    int64_t want = ceil_div(kPairTarget, p.tiles() > 0 ? p.tiles() : 1);
    const int64_t fit = kMaxPartialDoubles / (p.sp * p.tp > 0 ? p.sp * p.tp : 1);
    if (want > fit) want = fit;
    const int64_t most = ceil_div(M, kPairVerts);
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.verts_per_slab = round_up(ceil_div(M, want), kPairVerts);
    p.slabs = ceil_div(M, p.verts_per_slab);
    return p;
}

}  // namespace model_metrics_plan
