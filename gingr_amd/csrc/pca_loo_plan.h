// Bookkeeping of the leave-one-out generalization (pca_leave_one_out.hip): the argument rules of the rank list, the index maps between
// the n shapes and the n - 1 rows of a fold, the layout of the weight columns, and the batches the folds are decomposed in.  Plain C++
// (compiled for the host alone by tests/test_pca_loo_host.py).
//
// Fold i leaves shape i out.  Its Gram matrix, eigenvectors and right-hand side are indexed by the local row r = 0 .. n - 2 of the shapes
// that stay: shape j sits at row j (j < i) or j - 1 (j > i).  The weight vector of (rank q, fold i) is column q np + i of W [np][n_ranks np],
// np = n padded to the 16 columns of an MFMA tile, indexed by the shape: every fold's error field is a combination of all n centred
// shapes.  The folds go through the eigen-solver in batches that keep the fold matrices, their eigenvectors and the solver's work area
// within kBatchBytes; a batch never holds fewer than three folds (the count the block kernel takes side by side).
#pragma once

#include "host_device.h"

namespace pca_loo_plan {

constexpr int64_t kMinShapes = 3;    // a fold needs two shapes
constexpr int64_t kMaxShapes = 512;
constexpr int64_t kMaxRanks = 16;
constexpr int64_t kTileCols = 16;
constexpr int64_t kBatchBytes = (int64_t)256 << 20;
constexpr int64_t kMinBatch = 3;

GINGR_HD inline int fold_row(int i, int j) { return j < i ? j : j - 1; }     // j != i
GINGR_HD inline int fold_shape(int i, int r) { return r < i ? r : r + 1; }

inline int64_t padded_shapes(int64_t n) { return round_up(n, kTileCols); }
inline int64_t weight_columns(int64_t n, int64_t n_ranks) { return n_ranks * padded_shapes(n); }

// 0: fine; 1: the count; 2: ranks[*at] outside 1 .. n - 2; 3: ranks[*at] not above ranks[*at - 1]
inline int check_ranks(int64_t n, int64_t n_ranks, const int32_t *ranks, int *at) {
    *at = 0;
    if (n_ranks < 1 || n_ranks > kMaxRanks) return 1;
    for (int q = 0; q < (int)n_ranks; ++q) {
        *at = q;
        if (ranks[q] < 1 || ranks[q] > n - 2) return 2;
        if (q > 0 && ranks[q] <= ranks[q - 1]) return 3;
    }
    return 0;
}

// work_doubles: what the eigen-solver needs per fold besides the matrix and the eigenvectors (0 past the register kernel)
struct FoldBatches {
    int64_t n = 0, per_batch = 0, count = 0;
    int64_t begin(int64_t b) const { return b * per_batch; }
    int64_t length(int64_t b) const { return (b + 1) * per_batch < n ? per_batch : n - b * per_batch; }
};
inline int64_t fold_bytes(int64_t n, int64_t work_doubles) {
    const int64_t nf = n - 1;
    return (2 * nf * nf + 2 * nf + work_doubles) * 8;  // matrix, eigenvectors, eigenvalues, right-hand side, work
}
inline FoldBatches fold_batches(int64_t n, int64_t work_doubles) {
    FoldBatches f;
    f.n = n;
    int64_t per = kBatchBytes / fold_bytes(n, work_doubles);
    if (per < kMinBatch) per = kMinBatch;
    if (per > n) per = n;
    f.per_batch = per;
    f.count = ceil_div(n, per);
    return f;
}

}  // namespace pca_loo_plan
