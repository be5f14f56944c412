// Planning of the low-rank non-rigid CPD step (classic_cpd_lowrank.hip): the blocked layout of the factor, the column-block pairs
// of the weighted Gram pass and its row slabs.  Plain C++ (compiled for the host alone by tests/test_lowrank_cpd_host.py).
//
// The factor L (M x k, G ~ L L^T) is held as nb = kp / 64 column blocks, block b an (Mpad x 64) row-major matrix: kp = k rounded up to
// 64 and Mpad = M rounded up to the staging chunk, both padded with zeros, so no loop of either pass branches on a ragged edge.
// The Gram pass S = L^T D L deals the nb (nb + 1) / 2 block pairs (bi <= bj) x nslabs row slabs to workgroups; every workgroup
// leaves one 64 x 64 partial, and the partials of a pair are summed over the slabs in index order.  nslabs depends on (M, k) alone:
// two runs of one problem add the same numbers in the same order.
#pragma once

#include "host_device.h"

namespace lowrank_plan {

constexpr int kBlock = 64;          // columns per block = the panel width of the dense solve that follows
constexpr int kChunk = 32;          // rows staged in LDS at a time
constexpr int kMaxColumns = 512;    // the ceiling of the factor (the pivoted Cholesky's swap log)
constexpr int kTargetGroups = 1024; // workgroups the Gram pass aims at (four per CU)
constexpr int kMaxSlabs = 256;
constexpr int kApplyRows = 16;      // rows per workgroup round of the apply pass (16 lanes each)
constexpr int kApplyGroups = 1024;  // workgroups of the apply pass at most

// the p-th pair (bi <= bj) in the order (0,0), (0,1), .., (0,nb-1), (1,1), ..
GINGR_HD inline void pair_of(int p, int nb, int &bi, int &bj) {
    bi = 0;
    while (p >= nb - bi) {
        p -= nb - bi;
        ++bi;
    }
    bj = bi + p;
}

struct Plan {
    int64_t M = 0, Mpad = 0;
    int32_t k = 0, kp = 0, nb = 0, npairs = 0, nslabs = 0, apply_groups = 0;
    int64_t rows_per_slab = 0;

    int64_t factor_doubles() const { return (int64_t)nb * Mpad * kBlock; }
    int64_t gram_partial_doubles() const { return (int64_t)nslabs * npairs * kBlock * kBlock; }
    int64_t rhs_partial_doubles() const { return (int64_t)nslabs * nb * 3 * kBlock; }
    // element (i, c) of the factor, i < Mpad, c < kp
    int64_t at(int64_t i, int32_t c) const { return ((int64_t)(c / kBlock) * Mpad + i) * kBlock + c % kBlock; }
};

inline Plan make_plan(int64_t M, int32_t k) {
    Plan p;
    p.M = M;
    p.k = k;
    p.Mpad = round_up(M, kChunk);
    p.kp = (int32_t)round_up(k, kBlock);
    p.nb = p.kp / kBlock;
    p.npairs = p.nb * (p.nb + 1) / 2;
    int64_t want = kTargetGroups / p.npairs;
    if (want > kMaxSlabs) want = kMaxSlabs;
    if (want < 1) want = 1;
    p.rows_per_slab = round_up(ceil_div(p.Mpad, want), kChunk);
    p.nslabs = (int32_t)ceil_div(p.Mpad, p.rows_per_slab);  // every slab has rows; the last may be shorter (whole chunks)
    const int64_t rounds = ceil_div(M, kApplyRows);
    p.apply_groups = (int32_t)(rounds < kApplyGroups ? rounds : kApplyGroups);
    return p;
}

}  // namespace lowrank_plan
