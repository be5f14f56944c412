// Stand-alone host driver of gingr_amd/csrc/cloud_knn_plan.h and sym_eig3.h (tests/test_cloud_normals_host.py compiles it with the
// address and undefined-behaviour sanitizers and runs it).  Prints one line per grid plan --
//   plan <name> <N> <k> <dims> <h> <g0> <g1> <g2> <lanes>
// -- and one per eigen case --
//   eig <name> <lam0> <lam1> <lam2> <nx> <ny> <nz> <variation> <residual> <orthogonality>
// where residual = max_j |C v_j - lam_j v_j| / max(|lam2|, tiny) and orthogonality = max |V^T V - I|.  The Python side judges the numbers.
#include "cloud_knn_plan.h"
#include "sym_eig3.h"

#include <cstdio>

static void plan_case(const char *name, long long N, int k, double ex, double ey, double ez) {
    const double lo[3] = {-1.0, 2.0, 3.0}, hi[3] = {-1.0 + ex, 2.0 + ey, 3.0 + ez};
    const cloud_knn_plan::Plan p = cloud_knn_plan::make_plan(N, k, lo, hi);
    // every point of the box falls into a cell of the grid, the corners included
    for (int d = 0; d < 3; ++d) {
        const int32_t a = cloud_knn_plan::cell_of(lo[d], p.lo[d], p.inv_h, p.g[d]), b = cloud_knn_plan::cell_of(hi[d], p.lo[d], p.inv_h, p.g[d]);
        if (a != 0 || b < 0 || b > p.g[d] - 1) {
            std::printf("FAIL %s axis %d: cells %d .. %d of %d\n", name, d, a, b, p.g[d]);
            return;
        }
    }
    std::printf("plan %s %lld %d %d %.17g %d %d %d %d\n", name, N, k, p.dims, p.h, p.g[0], p.g[1], p.g[2], cloud_knn_plan::group_lanes(k));
}

static double absd(double x) { return x < 0 ? -x : x; }

static void eig_case(const char *name, const double c6[6]) {
    double lam[3], V[3][3], n[3], var;
    sym_eig3::eigh(c6, lam, V);
    sym_eig3::normal_of(c6, n, &var);
    const double C[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    double res = 0.0, orth = 0.0;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
            double s = 0.0;
            for (int l = 0; l < 3; ++l) s += C[i][l] * V[l][j];
            const double r = absd(s - lam[j] * V[i][j]);
            if (r > res) res = r;
        }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int l = 0; l < 3; ++l) s += V[l][a] * V[l][b];
            const double r = absd(s - (a == b ? 1.0 : 0.0));
            if (r > orth) orth = r;
        }
    const double scale = absd(lam[2]) > 1e-300 ? absd(lam[2]) : 1.0;
    std::printf("eig %s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.3e %.3e\n", name, lam[0], lam[1], lam[2], n[0], n[1], n[2], var, res / scale, orth);
}

int main() {
    plan_case("three", 3, 3, 1.0, 2.0, 0.5);
    plan_case("thousand", 1000, 16, 40.0, 40.0, 400.0);
    plan_case("million", 1000000, 16, 1.0, 1.0, 1.0);
    plan_case("million64", 1000000, 64, 1.0, 1.0, 1.0);
    plan_case("flat", 5000, 12, 10.0, 7.0, 0.0);
    plan_case("line", 5000, 12, 0.0, 7.0, 0.0);
    plan_case("onecell", 2000, 8, 0.0, 0.0, 0.0);
    plan_case("sliver", 100000, 8, 1e6, 1e-2, 1.0);
    const double diag[6] = {3.0, 0, 0, 1.0, 0, 2.0}, repeated[6] = {2.0, 0, 0, 2.0, 0, 5.0}, top[6] = {1.0, 0, 0, 4.0, 0, 4.0};
    const double zero[6] = {0, 0, 0, 0, 0, 0}, iso[6] = {7.0, 0, 0, 7.0, 0, 7.0};
    const double v[3] = {1.0, -2.0, 2.0};  // rank one: v v^T, eigenvalues 0, 0, 9
    const double rank1[6] = {v[0] * v[0], v[0] * v[1], v[0] * v[2], v[1] * v[1], v[1] * v[2], v[2] * v[2]};
    // a plane with normal (1, 1, 1) / sqrt 3: u u^T + 4 w w^T with u = (1, -1, 0) / sqrt 2, w = (1, 1, -2) / sqrt 6 -> eigenvalues 0, 1, 4
    const double plane[6] = {0.5 + 4.0 / 6.0, -0.5 + 4.0 / 6.0, -8.0 / 6.0, 0.5 + 4.0 / 6.0, -8.0 / 6.0, 16.0 / 6.0};
    const double general[6] = {4.0, 1.0, -2.0, 3.0, 0.5, 6.0}, tiny[6] = {4e-300, 1e-300, -2e-300, 3e-300, 0.5e-300, 6e-300};
    const double huge[6] = {4e300, 1e300, -2e300, 3e300, 0.5e300, 6e300};
    eig_case("diag", diag);
    eig_case("repeated_low", repeated);
    eig_case("repeated_high", top);
    eig_case("zero", zero);
    eig_case("isotropic", iso);
    eig_case("rank_one", rank1);
    eig_case("plane111", plane);
    eig_case("general", general);
    eig_case("tiny", tiny);
    eig_case("huge", huge);
    return 0;
}
