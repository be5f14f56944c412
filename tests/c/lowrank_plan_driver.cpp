// Host driver of gingr_amd/csrc/classic_cpd_lowrank_plan.h for tests/test_lowrank_cpd_host.py: reads (M, k) pairs as int64 from
// stdin and writes, per pair, the plan's head (10 values), its block pairs (2 npairs values) and the offsets at(i, c) of the four
// corner elements of the factor.
#include "classic_cpd_lowrank_plan.h"

#include <cstdio>
#include <vector>

int main() {
    std::vector<int64_t> in;
    int64_t v;
    while (fread(&v, sizeof(v), 1, stdin) == 1) in.push_back(v);
    std::vector<int64_t> out;
    for (size_t q = 0; q + 1 < in.size(); q += 2) {
        const int64_t M = in[q];
        const int32_t k = (int32_t)in[q + 1];
        const lowrank_plan::Plan p = lowrank_plan::make_plan(M, k);
        for (int64_t x : {p.Mpad, (int64_t)p.kp, (int64_t)p.nb, (int64_t)p.npairs, (int64_t)p.nslabs, p.rows_per_slab, (int64_t)p.apply_groups,
                          p.factor_doubles(), p.gram_partial_doubles(), p.rhs_partial_doubles()})
            out.push_back(x);
        for (int pr = 0; pr < p.npairs; ++pr) {
            int bi = -1, bj = -1;
            lowrank_plan::pair_of(pr, p.nb, bi, bj);
            out.push_back(bi);
            out.push_back(bj);
        }
        for (int64_t x : {p.at(0, 0), p.at(M - 1, 0), p.at(0, k - 1), p.at(p.Mpad - 1, p.kp - 1)}) out.push_back(x);
    }
    fwrite(out.data(), sizeof(int64_t), out.size(), stdout);
    return 0;
}
