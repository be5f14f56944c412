// Stand-alone driver of gingr_amd/csrc/surface_metrics_plan.h for tests/test_surface_metrics_host.py.  One case per run, from the command line:
//   cover n_sets n_meshes pairing points
//       for every (block of sets, chunk of meshes), i.e. every launch:
//         L set0 sets mesh0 meshes pairs per_slab slabs partial_doubles
//         S slab_begin slab_end                         one line per slab
//         P set mesh pair index_of_(slab 0, sum) index_of_(last slab, max)      one line per pair; set and mesh count through the whole call
//   seeds n_vertices n_triangles a b c a b c ...
//       one line: the seed triangle of every vertex
//   bytes n_points block_sets n_vertices n_meshes n_triangles model_rows
//       one line: working_set_bytes
#include "surface_metrics_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mp = model_metrics_plan;
namespace sp = surface_metrics_plan;

int main(int argc, char **argv) {
    int at = 1;
    auto next = [&]() -> long long { return at < argc ? atoll(argv[at++]) : -1; };
    if (argc < 2) return 2;
    const char *kind = argv[at++];
    if (!strcmp(kind, "cover")) {
        const long long n_sets = next(), n_meshes = next();
        const int pairing = (int)next();
        const long long points = next();
        const mp::ColumnBlocks blocks = mp::column_blocks(n_sets);
        const sp::MeshChunks chunks = sp::mesh_chunks(n_meshes, pairing);
        for (int64_t b = 0; b < blocks.count; ++b)
            for (int64_t c = 0; c < chunks.count; ++c) {
                const int64_t sets = blocks.length(b), set0 = blocks.begin(b), meshes = chunks.length(c), mesh0 = chunks.begin(c);
                const sp::PairPlan p = sp::make_pair_plan(points, sets, meshes, pairing);
                printf("L %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)set0, (long long)sets, (long long)mesh0, (long long)meshes, (long long)p.pairs,
                       (long long)p.per_slab, (long long)p.slabs, (long long)p.partial_doubles());
                for (int64_t s = 0; s < p.slabs; ++s) printf("S %lld %lld\n", (long long)p.slab_begin(s), (long long)p.slab_end(s));
                for (int64_t i = 0; i < sets; ++i)
                    for (int64_t j = 0; j < (pairing == 0 ? meshes : 1); ++j) {
                        const int64_t mesh = pairing == 0 ? mesh0 + j : sp::cyclic_mesh(set0 + i, n_meshes), pr = p.pair(i, j);
                        printf("P %lld %lld %lld %lld %lld\n", (long long)(set0 + i), (long long)mesh, (long long)pr, (long long)p.partial_index(0, pr, 0),
                               (long long)p.partial_index(p.slabs - 1, pr, 1));
                    }
            }
    } else if (!strcmp(kind, "seeds")) {
        const long long nv = next(), nt = next();
        std::vector<int32_t> tri((size_t)(3 * nt)), seed;
        for (auto &t : tri) t = (int32_t)next();
        sp::seed_triangles(nv, nt, tri.data(), seed);
        for (size_t v = 0; v < seed.size(); ++v) printf("%d%c", (int)seed[v], v + 1 < seed.size() ? ' ' : '\n');
    } else if (!strcmp(kind, "bytes")) {
        const long long a = next(), b = next(), c = next(), d = next(), e = next(), f = next();
        printf("%lld\n", (long long)sp::working_set_bytes(a, b, c, d, e, f));
    } else {
        fprintf(stderr, "unknown case %s\n", kind);
        return 2;
    }
    return 0;
}
