// Host driver of gingr_amd/csrc/gram_cov_plan.h for tests/test_pairs_cov_gram_host.py: reads (M, rp) pairs as int64 from stdin and
// writes, per pair, the plan's head (10 values) and its slabs (begin, end).
#include "gram_cov_plan.h"

#include <cstdio>
#include <vector>

int main() {
    std::vector<int64_t> in;
    int64_t v;
    while (fread(&v, sizeof(v), 1, stdin) == 1) in.push_back(v);
    std::vector<int64_t> out;
    for (size_t q = 0; q + 1 < in.size(); q += 2) {
        const gram_cov_plan::Plan p = gram_cov_plan::make_plan(in[q], (int)in[q + 1]);
        for (int64_t x : {(int64_t)p.nbp, (int64_t)p.npatch, (int64_t)p.nslabs, p.verts_per_slab, p.partial_stride(), p.partial_doubles(),
                          p.factor_doubles(), p.workspace_doubles(), (int64_t)gram_cov_plan::kMaxSlabs, (int64_t)p.instance})
            out.push_back(x);
        for (int s = 0; s < p.nslabs; ++s) {
            out.push_back(p.slab_begin(s));
            out.push_back(p.slab_end(s));
        }
    }
    fwrite(out.data(), sizeof(int64_t), out.size(), stdout);
    return 0;
}
