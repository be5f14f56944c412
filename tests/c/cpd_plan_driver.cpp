// Host driver of the all-pairs planners (gingr_amd/csrc/cpd_plan.h) for tests/test_cpd_plan_host.py.  Raw int64 records on stdin, raw
// int64 records on stdout, one output record per input record:
//   cpd_plan_driver chunks   : {owned, streamed, resident, pt, forced} -> {nch, chunks(streamed), len_big, len_tail, n_big, fair,
//                                                                          then nch x {begin, end}}     (plan_chunks itself)
//   cpd_plan_driver colsum   : {M, N, forced, resident} -> {pt, nch, chunks(M), fair, colsum_ws_doubles(M, N, resident)}
//   cpd_plan_driver rowstats : {M, N, resident}         -> {pt, nch, chunks(N), fair, rowstats_ws_doubles(M, N, resident)}
//   cpd_plan_driver nn       : {M, N}                   -> {chunks pruned, length pruned, chunks unpruned, length unpruned}
//   cpd_plan_driver small    : {M, N}                   -> {nn_small_slices(M, N)}
// Plain C++ for the host compiler: the header carries no device code of its own.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cpd_plan.h"

static bool get(int64_t *p, size_t n) { return fread(p, sizeof(int64_t), n, stdin) == n; }
static bool put(const std::vector<int64_t> &v) { return v.empty() || fwrite(v.data(), sizeof(int64_t), v.size(), stdout) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    int64_t r[5];
    if (!strcmp(argv[1], "chunks")) {
        while (get(r, 5)) {
            int nch = 0;
            const ChunkPlan p = plan_chunks(r[0], 64 * (int)r[3], r[1], &nch, 0, (int)r[4], (int)r[2]);
            std::vector<int64_t> out{nch, p.chunks(r[1]), p.len_big, p.len_tail, p.n_big, p.fair};
            for (int y = 0; y < nch; ++y) {
                int64_t b, e;
                p.range(y, r[1], &b, &e);
                out.push_back(b), out.push_back(e);
            }
            if (!put(out)) return 1;
        }
        return 0;
    }
    if (!strcmp(argv[1], "colsum")) {
        while (get(r, 4)) {
            const PairPlan p = colsum_plan(r[0], r[1], (int)r[2], (int)r[3]);
            if (!put({p.pt, p.nch, p.plan.chunks(r[0]), p.plan.fair, colsum_ws_doubles(r[0], r[1], (int)r[3])})) return 1;
        }
        return 0;
    }
    if (!strcmp(argv[1], "rowstats")) {
        while (get(r, 3)) {
            const PairPlan p = rowstats_plan(r[0], r[1], (int)r[2]);
            if (!put({p.pt, p.nch, p.plan.chunks(r[1]), p.plan.fair, rowstats_ws_doubles(r[0], r[1], (int)r[2])})) return 1;
        }
        return 0;
    }
    if (!strcmp(argv[1], "nn")) {
        while (get(r, 2)) {
            int nc[2];
            int64_t len[2];
            plan_nn(r[0], r[1], true, &nc[0], &len[0]);
            plan_nn(r[0], r[1], false, &nc[1], &len[1]);
            if (!put({nc[0], len[0], nc[1], len[1]})) return 1;
        }
        return 0;
    }
    if (!strcmp(argv[1], "small")) {
        while (get(r, 2))
            if (!put({nn_small_slices(r[0], r[1])})) return 1;
        return 0;
    }
    return 2;
}
