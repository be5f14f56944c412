// Stand-alone driver of gingr_amd/csrc/pca_loo_plan.h for tests/test_pca_loo_host.py.  Reads cases from the command line,
//   ranks n k0 k1 ... end | maps n i | batches n work_doubles
// and prints
//   ranks:   code at
//   maps:    one line "r shape row_of_shape" per local row r of fold i
//   batches: per_batch count padded_shapes fold_bytes   then  begin length per batch
#include "pca_loo_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace lp = pca_loo_plan;

int main(int argc, char **argv) {
    int at = 1;
    auto next = [&]() -> long long { return at < argc ? atoll(argv[at++]) : -1; };
    while (at < argc) {
        const char *kind = argv[at++];
        if (!strcmp(kind, "ranks")) {
            const long long n = next();
            std::vector<int32_t> k;
            while (at < argc && strcmp(argv[at], "end")) k.push_back((int32_t)next());
            ++at;
            int where = 0;
            const int code = lp::check_ranks(n, (int64_t)k.size(), k.data(), &where);
            printf("%d %d\n", code, where);
        } else if (!strcmp(kind, "maps")) {
            const int n = (int)next(), i = (int)next();
            for (int r = 0; r < n - 1; ++r) printf("%d %d %d\n", r, lp::fold_shape(i, r), lp::fold_row(i, lp::fold_shape(i, r)));
        } else if (!strcmp(kind, "batches")) {
            const long long n = next(), work = next();
            const lp::FoldBatches f = lp::fold_batches(n, work);
            printf("%lld %lld %lld %lld\n", (long long)f.per_batch, (long long)f.count, (long long)lp::padded_shapes(n), (long long)lp::fold_bytes(n, work));
            for (int64_t b = 0; b < f.count; ++b) printf("%lld %lld\n", (long long)f.begin(b), (long long)f.length(b));
        } else {
            fprintf(stderr, "unknown case %s\n", kind);
            return 2;
        }
    }
    return 0;
}
