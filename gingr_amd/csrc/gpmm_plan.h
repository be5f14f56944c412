// Host-side bookkeeping of the GPMM construction (gpmm.hip): which coordinates share a factorisation and an eigen-decomposition, how
// many columns the generic factorisation has given the traces of the scalar one, how the coordinate spectra merge into the model's,
// and what gingr_gpmm_info says about the result.  Plain C++ (no HIP, no context): tests/c/gpmm_plan_driver.cpp pins it on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace gpmm_plan {

// Distinct groups among the three coordinates: group_of[d] = the group of coordinate d (-1 where skip(d)), first[g] = the first
// coordinate of group g; same(e, d): coordinate d goes with the earlier coordinate e.  Returns the number of groups.
template <typename Same, typename Skip>
inline int group3(Same same, Skip skip, int group_of[3], int first[3]) {
    int ng = 0;
    for (int d = 0; d < 3; ++d) {
        group_of[d] = -1;
        if (skip(d)) continue;
        for (int g = 0; g < ng; ++g)
            if (same(first[g], d)) group_of[d] = g;
        if (group_of[d] < 0) first[group_of[d] = ng++] = d;
    }
    return ng;
}

inline bool none(int) { return false; }  // group3(same_kernel, none, ...): coordinates with the same kernel share a factorisation

// coordinates with the same column count share an eigen-decomposition: block_of[d] (-1: no column), block_n[b] its columns
inline int group_blocks(const int32_t cnt[3], int block_of[3], int32_t block_n[3]) {
    int first[3];
    const int nb = group3([&](int e, int d) { return cnt[e] == cnt[d]; }, [&](int d) { return cnt[d] == 0; }, block_of, first);
    for (int b = 0; b < 3; ++b) block_n[b] = b < nb ? cnt[first[b]] : 0;
    return nb;
}

// the stopping rule of the pivoted Cholesky, in the form that also stops at a NaN trace
inline bool below_tolerance(double tr, double tr0, double rel_tol) { return !(tr >= rel_tol * tr0); }

// One kernel for all coordinates: the generic pivot sequence is (P0,x),(P0,y),(P0,z),(P1,x),... with P0,P1,.. the scalar pivots, so
// after n = 3j + e generic pivots the residual trace is (3 - e) tr_s(j) + e tr_s(j + 1) (tr_s = htr: the scalar factorisation's traces)
inline double generic_trace(const double *htr, int32_t n) {
    const int32_t j = n / 3, e = n % 3;
    return e == 0 ? 3.0 * htr[j] : (3 - e) * htr[j] + e * htr[j + 1];
}

struct Columns {
    int32_t n = 0;               // generic pivots = factor columns
    int32_t cnt[3] = {0, 0, 0};  // columns per coordinate
    bool reached = false;        // the residual trace fell below the tolerance (or nothing is left to pivot)
    double fraction = 0.0;       // residual trace / trace after the n pivots
};

// The columns of the generic factorisation of M points from the ks >= 1 scalar columns with traces htr[0 .. ks]: pivots are taken
// while the residual trace is at or above rel_tol * trace, at most `limit` of them (and no more than the scalar columns carry).
inline Columns count_columns(const double *htr, int32_t ks, int32_t limit, double rel_tol, int64_t M) {
    Columns c;
    const double tr0 = 3.0 * htr[0];
    const int32_t nmax = std::min<int32_t>(limit, 3 * ks);
    while (c.n < nmax) {
        if (below_tolerance(generic_trace(htr, c.n), tr0, rel_tol)) break;
        ++c.n;
    }
    for (int d = 0; d < 3; ++d) c.cnt[d] = c.n / 3 + (d < c.n % 3 ? 1 : 0);
    const double tr = generic_trace(htr, c.n);  // (the traces it needs exist: n <= 3 ks)
    c.reached = below_tolerance(tr, tr0, rel_tol) || (int64_t)c.n == 3 * M;
    c.fraction = tr / tr0;
    return c;
}

// The model's columns: the eigenpairs of the coordinate blocks merged, eigenvalue descending; equal eigenvalues by index within the
// block, then in coordinate order (x, y, z).
struct Merged {
    std::vector<double> variance;             // the eigenvalues, negative ones as 0
    std::vector<int32_t> qdim, qblock, qidx;  // column q: its coordinate, eigen block and index within the block
};

// ev[b]: eigenvalues of block b, descending; coordinate d takes the leading cnt[d] of block block_of[d]
inline Merged merge_spectra(const std::vector<double> ev[3], const int32_t cnt[3], const int block_of[3]) {
    struct Col { double lam; int32_t dim, idx; };
    std::vector<Col> cols;
    for (int d = 0; d < 3; ++d)
        for (int32_t i = 0; i < cnt[d]; ++i) cols.push_back(Col{ev[block_of[d]][(size_t)i], d, i});
    std::stable_sort(cols.begin(), cols.end(), [](const Col &x, const Col &y) {
        if (x.lam != y.lam) return x.lam > y.lam;
        if (x.idx != y.idx) return x.idx < y.idx;
        return x.dim < y.dim;
    });
    Merged m;
    for (const Col &c : cols) {
        m.variance.push_back(c.lam > 0.0 ? c.lam : 0.0);
        m.qdim.push_back(c.dim);
        m.qblock.push_back(block_of[c.dim]);
        m.qidx.push_back(c.idx);
    }
    return m;
}

// need[b] = eigenvectors of block b the leading `keep` columns use (the leading ones of every block)
inline void eigvecs_needed(const Merged &m, int32_t keep, int32_t need[3]) {
    need[0] = need[1] = need[2] = 0;
    for (int32_t q = 0; q < keep; ++q) need[m.qblock[(size_t)q]] = std::max(need[m.qblock[(size_t)q]], m.qidx[(size_t)q] + 1);
}

// CeilingBeforeTolerance: run to tolerance, and the ceiling of factor columns came first; AboveRankLimit: more columns than a model holds
enum class Refusal { None, CeilingBeforeTolerance, AboveRankLimit };
constexpr int32_t kModelRankLimit = 512;

struct Info {  // the values of gingr_gpmm_info
    int32_t columns = 0, rank = 0, tolerance_reached = 0;
    double residual_fraction = 0.0, kept_variance_fraction = 0.0;
};

// What is known before any eigen-decomposition, and refused there: a factorisation run to tolerance (`to_tolerance`) that stopped before it.
inline Refusal unfinished(bool to_tolerance, int32_t columns, bool reached, double fraction, Info &info) {
    if (!to_tolerance || reached) return Refusal::None;
    info = Info{columns, 0, 0, fraction, 1.0};
    return Refusal::CeilingBeforeTolerance;
}

// A finished factorisation of `columns` columns with the descending spectrum lam: `keep` = the columns of the model (`ex`: the entry
// that truncates to keep_rank and never shortens silently), info, and whether the entry refuses the result.
inline Refusal conclude(bool ex, int32_t keep_rank, int32_t columns, bool reached, double fraction, const std::vector<double> &lam,
                        int32_t &keep, Info &info) {
    keep = (ex && keep_rank > 0 && keep_rank < columns) ? keep_rank : columns;
    double all = 0.0, kept = 0.0;
    for (int32_t q = 0; q < columns; ++q) {
        all += lam[(size_t)q];
        if (q + 1 == keep) kept = all;
    }
    info = Info{columns, keep, reached ? 1 : 0, fraction, all > 0.0 ? kept / all : 1.0};
    return ex && keep > kModelRankLimit ? Refusal::AboveRankLimit : Refusal::None;
}

}  // namespace gpmm_plan
