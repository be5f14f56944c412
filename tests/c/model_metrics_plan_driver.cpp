// Stand-alone driver of gingr_amd/csrc/model_metrics_plan.h for tests/test_model_metrics_host.py.  Reads cases from the command line,
//   blocks n | measure M cols | pair M samples train
// and prints one line of integers per case, then one line per block or slab:
//   blocks:  count                                      then  begin length padded
//   measure: cols chunks verts_per_slab slabs partial_doubles   then  slab_begin slab_end
//   pair:    sp tp tiles_s tiles_t verts_per_slab slabs partial_doubles   then  slab_begin slab_end
#include "model_metrics_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mp = model_metrics_plan;

int main(int argc, char **argv) {
    int at = 1;
    auto next = [&]() -> long long { return at < argc ? atoll(argv[at++]) : -1; };
    while (at < argc) {
        const char *kind = argv[at++];
        if (!strcmp(kind, "blocks")) {
            const mp::ColumnBlocks c = mp::column_blocks(next());
            printf("%lld\n", (long long)c.count);
            for (int64_t b = 0; b < c.count; ++b) printf("%lld %lld %lld\n", (long long)c.begin(b), (long long)c.length(b), (long long)c.padded(b));
        } else if (!strcmp(kind, "measure")) {
            const long long M = next(), cols = next();
            const mp::MeasurePlan p = mp::make_measure_plan(M, cols);
            printf("%lld %lld %lld %lld %lld\n", (long long)p.cols, (long long)p.chunks, (long long)p.verts_per_slab, (long long)p.slabs,
                   (long long)p.partial_doubles());
            for (int64_t s = 0; s < p.slabs; ++s) printf("%lld %lld\n", (long long)p.slab_begin(s), (long long)p.slab_end(s));
        } else if (!strcmp(kind, "pair")) {
            const long long M = next(), S = next(), T = next();
            const mp::PairPlan p = mp::make_pair_plan(M, S, T);
            printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)p.sp, (long long)p.tp, (long long)p.tiles_s, (long long)p.tiles_t,
                   (long long)p.verts_per_slab, (long long)p.slabs, (long long)p.partial_doubles());
            for (int64_t s = 0; s < p.slabs; ++s) printf("%lld %lld\n", (long long)p.slab_begin(s), (long long)p.slab_end(s));
        } else {
            fprintf(stderr, "unknown case %s\n", kind);
            return 2;
        }
    }
    return 0;
}
