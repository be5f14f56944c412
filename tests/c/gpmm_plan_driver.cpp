// Host driver of the GPMM construction's bookkeeping (gingr_amd/csrc/gpmm_plan.h) for tests/test_gpmm_plan_host.py.  Raw float64 on
// stdin until it ends, raw float64 on stdout (every integer travels as a double).  Records, by their first value:
//   1  {1, ks, limit, M, rel_tol, htr[ks + 1]}           -> {n, cnt[3], reached, fraction}                              count_columns
//   2  {2, cnt[3], ex, keep_rank, ev of block 0, 1, ..}  -> {nblocks, block_of[3], block_n[3], n, variance[n], qdim[n], qblock[n], qidx[n],
//      (block sizes: group_blocks of cnt)                    keep, need[3], kept_variance_fraction}      group_blocks, merge_spectra, conclude, eigvecs_needed
//   3  {3, ex, to_tolerance, keep_rank, columns, reached, fraction, lam[columns]}
//                                                        -> {refusal, keep, columns, rank, tolerance_reached, residual_fraction, kept_variance_fraction}   unfinished, conclude
//   4  {4, id[3]}  (kernels are the same when their ids are)  -> {nsets, set_of[3], first[3] (-1 past nsets)}           group3
// Plain C++ for the host compiler: the header carries no device code.
#include <cstdio>
#include <vector>

#include "gpmm_plan.h"

using namespace gpmm_plan;

static bool get(std::vector<double> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(double), n, stdin) == n;
}
static bool put(const std::vector<double> &v) { return v.empty() || fwrite(v.data(), sizeof(double), v.size(), stdout) == v.size(); }
template <typename T>
static void append(std::vector<double> &out, const T *p, size_t n) {
    for (size_t i = 0; i < n; ++i) out.push_back((double)p[i]);
}

int main() {
    double op;
    std::vector<double> h, v;
    while (fread(&op, sizeof(double), 1, stdin) == 1) {
        std::vector<double> out;
        if (op == 1.0) {
            if (!get(h, 4) || h[0] < 1 || !get(v, (size_t)h[0] + 1)) return 1;
            const Columns c = count_columns(v.data(), (int32_t)h[0], (int32_t)h[1], h[3], (int64_t)h[2]);
            out = {(double)c.n, (double)c.cnt[0], (double)c.cnt[1], (double)c.cnt[2], c.reached ? 1.0 : 0.0, c.fraction};
        } else if (op == 2.0) {
            if (!get(h, 5)) return 1;
            const int32_t cnt[3] = {(int32_t)h[0], (int32_t)h[1], (int32_t)h[2]};
            int block_of[3];
            int32_t block_n[3];
            const int nblocks = group_blocks(cnt, block_of, block_n);
            std::vector<double> ev[3];
            for (int b = 0; b < nblocks; ++b)
                if (!get(ev[b], (size_t)block_n[b])) return 1;
            const Merged m = merge_spectra(ev, cnt, block_of);
            const int32_t n = (int32_t)m.variance.size();
            int32_t keep = -1, need[3];
            Info info;
            conclude(h[3] != 0.0, (int32_t)h[4], n, true, 0.0, m.variance, keep, info);
            eigvecs_needed(m, keep, need);
            out = {(double)nblocks};
            append(out, block_of, 3);
            append(out, block_n, 3);
            out.push_back((double)n);
            append(out, m.variance.data(), (size_t)n);
            append(out, m.qdim.data(), (size_t)n);
            append(out, m.qblock.data(), (size_t)n);
            append(out, m.qidx.data(), (size_t)n);
            out.push_back((double)keep);
            append(out, need, 3);
            out.push_back(info.kept_variance_fraction);
        } else if (op == 3.0) {
            if (!get(h, 6) || h[3] < 0 || !get(v, (size_t)h[3])) return 1;
            int32_t keep = -1;
            Info info;
            Refusal r = unfinished(h[1] != 0.0, (int32_t)h[3], h[4] != 0.0, h[5], info);  // as the build does: before the spectrum exists
            if (r == Refusal::None) r = conclude(h[0] != 0.0, (int32_t)h[2], (int32_t)h[3], h[4] != 0.0, h[5], v, keep, info);
            out = {(double)(int)r, (double)keep, (double)info.columns, (double)info.rank, (double)info.tolerance_reached,
                   info.residual_fraction, info.kept_variance_fraction};
        } else if (op == 4.0) {
            if (!get(h, 3)) return 1;
            int set_of[3], first[3] = {-1, -1, -1};
            const int nsets = group3([&](int e, int d) { return h[(size_t)e] == h[(size_t)d]; }, none, set_of, first);
            out = {(double)nsets};
            append(out, set_of, 3);
            append(out, first, 3);
        } else {
            return 2;
        }
        if (!put(out)) return 1;
    }
    return 0;
}
