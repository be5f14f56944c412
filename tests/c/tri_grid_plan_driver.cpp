// Host driver of the target-triangle grid's binning (gingr_amd/csrc/tri_grid_plan.h) for tests/test_tri_grid_host.py.  Raw bytes on
// stdin, raw bytes on stdout:
//   tri_grid_plan_driver plan : int64 {n, T, has_orig}, float64 vsoa[3 n], int32 tri[3 T], int32 tri_orig[T] (when has_orig) ->
//       int64 {ready, kTriGridMaxSpan, kTriRec, g[3], span[3], n_listed, n_big, start size, list size}, float64 {lo[3], h, inv_h},
//       int32 start[], int32 list[], float64 boxes[], float64 recs[]
//   tri_grid_plan_driver cell : float64 records {x, lo, inv_h, gd} -> one int64, the clamped cell
// Plain C++ for the host compiler: the header carries no device code of its own.
#include <cstdio>
#include <cstring>
#include <vector>

#include "tri_grid_plan.h"

template <typename T>
static bool get(T *p, size_t n) {
    return n == 0 || fread(p, sizeof(T), n, stdin) == n;
}
template <typename T>
static bool put(const T *p, size_t n) {
    return n == 0 || fwrite(p, sizeof(T), n, stdout) == n;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "cell")) {
        double r[4];
        while (get(r, 4)) {
            const int64_t c = grid_cell_of(r[0], r[1], r[2], (int32_t)r[3]);
            if (!put(&c, 1)) return 1;
        }
        return 0;
    }
    if (strcmp(argv[1], "plan")) return 2;
    int64_t head[3];
    if (!get(head, 3) || head[0] < 0 || head[1] < 0) return 1;
    const size_t n = (size_t)head[0], T = (size_t)head[1];
    std::vector<double> vsoa(3 * n);
    std::vector<int32_t> tri(3 * T), orig(head[2] ? T : 0);
    if (!get(vsoa.data(), vsoa.size()) || !get(tri.data(), tri.size()) || !get(orig.data(), orig.size())) return 1;
    TriGridPlan p;
    tri_grid_plan(vsoa.data(), (int64_t)n, tri.data(), head[2] ? orig.data() : nullptr, (int64_t)T, &p);
    const int64_t ints[13] = {p.ready, kTriGridMaxSpan, kTriRec, p.g[0], p.g[1], p.g[2], p.span[0], p.span[1], p.span[2], p.n_listed, p.n_big,
                              p.ready ? (int64_t)p.start.size() : 0, p.ready ? (int64_t)p.list.size() : 0};
    const double reals[5] = {p.lo[0], p.lo[1], p.lo[2], p.h, p.inv_h};
    if (!put(ints, 13) || !put(reals, 5)) return 1;
    if (!p.ready) return 0;
    return put(p.start.data(), p.start.size()) && put(p.list.data(), p.list.size()) && put(p.boxes.data(), p.boxes.size()) &&
                   put(p.recs.data(), p.recs.size())
               ? 0
               : 1;
}
