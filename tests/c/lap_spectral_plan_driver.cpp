// Host driver of the planning header of the sparse inverse-Laplacian model build (gingr_amd/csrc/lap_spectral_plan.h) for
// tests/test_laplacian_model_host.py.  Text commands on stdin, one answer line (or block) each on stdout, numbers as %.17g:
//     edges n n_cells c[3 n_cells]    ->  status bad_cell n_edges, then p1 p2 per edge
//     block k dim                     ->  m active
//     filter theta_max bound budget   ->  a c e sigma1 degree spread(degree) spread(degree + 1), then alpha beta gamma per step
//     stop tolerance wanted r[wanted] ->  0 | 1
//     dropped wanted theta[wanted]    ->  count
// Plain C++ for the host compiler: the header carries no device code.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lap_spectral_plan.h"

int main() {
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "edges")) {
            long long n, nc;
            if (scanf("%lld %lld", &n, &nc) != 2 || nc < 0) return 2;
            std::vector<int32_t> cells((size_t)(3 * nc));
            for (int32_t &v : cells)
                if (scanf("%d", &v) != 1) return 2;
            std::vector<int32_t> edges;
            int64_t bad = -1;
            const int status = lap_edges_from_cells(n, nc, cells.data(), &edges, &bad);
            printf("%d %lld %zu\n", status, (long long)bad, edges.size() / 2);
            for (size_t e = 0; e < edges.size(); e += 2) printf("%d %d\n", edges[e], edges[e + 1]);
        } else if (!strcmp(cmd, "block")) {
            int k;
            long long dim;
            if (scanf("%d %lld", &k, &dim) != 2) return 2;
            const LapBlock b = lap_block_plan(k, dim);
            printf("%d %d\n", b.m, b.active);
        } else if (!strcmp(cmd, "filter")) {
            double theta, bound;
            int budget;
            if (scanf("%lf %lf %d", &theta, &bound, &budget) != 3) return 2;
            const LapFilter f = lap_filter_plan(theta, bound, budget);
            printf("%.17g %.17g %.17g %.17g %d %.17g %.17g\n", f.a, f.c, f.e, f.sigma1, f.degree, lap_filter_spread(f, f.degree),
                   lap_filter_spread(f, f.degree + 1));
            double sigma = 0.0;
            for (int step = 1; step <= f.degree; ++step) {
                const LapStep s = lap_recurrence_step(f, step, &sigma);
                printf("%.17g %.17g %.17g\n", s.alpha, s.beta, s.gamma);
            }
        } else if (!strcmp(cmd, "stop") || !strcmp(cmd, "dropped")) {
            double tol = 0.0;
            int wanted;
            if (cmd[0] == 's' && scanf("%lf", &tol) != 1) return 2;
            if (scanf("%d", &wanted) != 1 || wanted < 0) return 2;
            std::vector<double> v((size_t)wanted);
            for (double &x : v)
                if (scanf("%lf", &x) != 1) return 2;
            printf("%d\n", cmd[0] == 's' ? (int)lap_converged(v.data(), wanted, tol) : lap_count_dropped(v.data(), wanted));
        } else {
            return 3;
        }
    }
    return 0;
}
