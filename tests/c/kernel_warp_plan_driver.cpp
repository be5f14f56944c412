// Host driver of gingr_amd/csrc/kernel_warp_plan.h for tests/test_kernel_warp_host.py: reads (P, M) pairs as int64 from stdin and
// writes, per pair, the plan's head (8 values), its chunks (begin, end) and its slabs (begin, count, grid_x).
#include "kernel_warp_plan.h"

#include <cstdio>
#include <vector>

int main() {
    std::vector<int64_t> in;
    int64_t v;
    while (fread(&v, sizeof(v), 1, stdin) == 1) in.push_back(v);
    std::vector<int64_t> out;
    for (size_t q = 0; q + 1 < in.size(); q += 2) {
        const kernel_warp_plan::Plan p = kernel_warp_plan::make_plan(in[q], in[q + 1]);
        for (int64_t x : {p.chunks, p.chunk_length, p.slab_length, p.slabs, p.partial_doubles(), p.cloud_doubles(), p.workspace_bytes(), p.grid_y()})
            out.push_back(x);
        for (int64_t c = 0; c < p.chunks; ++c) {
            out.push_back(p.chunk_begin(c));
            out.push_back(p.chunk_end(c));
        }
        for (int64_t s = 0; s < p.slabs; ++s) {
            out.push_back(p.slab_begin(s));
            out.push_back(p.slab_count(s));
            out.push_back(p.grid_x(s));
        }
    }
    fwrite(out.data(), sizeof(int64_t), out.size(), stdout);
    return 0;
}
