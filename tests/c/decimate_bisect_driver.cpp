// Host driver of the decimation's scalar side (gingr_amd/csrc/decimate_bisect.h) for tests/test_mesh_decimate_host.py.  Raw float64 on
// stdin until it ends, raw bytes on stdout:
//   decimate_bisect_driver bisect : records {ex, ey, ez, n_target, m, count_0 .. count_(m-1)}; the recurrence is fed the counts one per
//       step (the last one again once they run out) -> 4 + 60 float64: extent, h, steps, accepted, then the cube size every count was
//       asked for (zeros behind the last step)
//   decimate_bisect_driver key    : records {x, y, z, lx, ly, lz, h} -> one uint64, the packed cell
// Plain C++ for the host compiler: the header carries no device code of its own.
#include <cstdio>
#include <cstring>
#include <vector>

#include "decimate_bisect.h"

static bool get(double *p, size_t n) { return fread(p, sizeof(double), n, stdin) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "key")) {
        double r[7];
        while (get(r, 7)) {
            const uint64_t k = decimate_cell_key(r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
            if (fwrite(&k, sizeof(k), 1, stdout) != 1) return 1;
        }
        return 0;
    }
    if (strcmp(argv[1], "bisect")) return 2;
    double head[5];
    while (get(head, 5)) {
        const int64_t n_target = (int64_t)head[3];
        std::vector<double> counts((size_t)head[4]);
        if (counts.empty() || !get(counts.data(), counts.size())) return 1;
        double out[4 + GINGR_DECIMATE_MAX_STEPS] = {0};
        DecimateBisect b;
        out[0] = decimate_extent(head[0], head[1], head[2]);
        decimate_bisect_init(&b, out[0]);
        for (size_t s = 0; !b.done && s < 2 * GINGR_DECIMATE_MAX_STEPS; ++s) {
            out[4 + b.steps] = b.mid;
            decimate_bisect_step(&b, (int64_t)counts[s < counts.size() ? s : counts.size() - 1], n_target);
        }
        decimate_bisect_step(&b, 0, n_target);  // a step behind the deciding one changes nothing
        out[1] = b.h;
        out[2] = (double)b.steps;
        out[3] = (double)b.accepted;
        if (!b.done || fwrite(out, sizeof(double), 4 + GINGR_DECIMATE_MAX_STEPS, stdout) != 4 + GINGR_DECIMATE_MAX_STEPS) return 1;
    }
    return 0;
}
