// Stand-alone driver of gingr_amd/csrc/spectrum_plan.h for tests/test_spectrum_plan_host.py.  Reads one case from the command line
// (doubles as hex floats, "nan" and "inf" as strtod reads them),
//   cut shift available max_rank tol ev0 ev1 ... | ceiling available max_rank | leading kmax tol lam0 lam1 ... | unshift ev shift
// and prints
//   cut:      "k first_nonfinite", "kept total", then the un-shifted spectrum, one line each (doubles as hex floats)
//   ceiling:  the rank ceiling
//   leading:  the leading rank
//   unshift:  the un-shifted eigenvalue
#include "spectrum_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sp = spectrum_plan;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    int at = 2;
    auto real = [&]() -> double { return at < argc ? strtod(argv[at++], nullptr) : 0.0; };
    auto whole = [&]() -> int { return at < argc ? atoi(argv[at++]) : 0; };
    auto rest = [&]() {
        std::vector<double> v;
        while (at < argc) v.push_back(real());
        return v;
    };
    const char *kind = argv[1];
    if (!strcmp(kind, "cut")) {
        const double shift = real();
        const int available = whole(), max_rank = whole();
        const double tol = real();
        std::vector<double> ev = rest();
        const sp::Cut c = sp::cut(ev.data(), (int)ev.size(), shift, available, max_rank, tol);
        printf("%d %d\n%a %a\n", c.k, c.first_nonfinite, c.kept, c.total);
        for (double v : ev) printf("%a ", v);
        printf("\n");
    } else if (!strcmp(kind, "ceiling")) {
        const int available = whole(), max_rank = whole();
        printf("%d\n", sp::rank_ceiling(available, max_rank));
    } else if (!strcmp(kind, "leading")) {
        const int kmax = whole();
        const double tol = real();
        const std::vector<double> lam = rest();
        printf("%d\n", sp::leading_rank(lam.data(), kmax, tol));
    } else if (!strcmp(kind, "unshift")) {
        const double ev = real(), shift = real();
        printf("%a\n", sp::unshift(ev, shift));
    } else {
        fprintf(stderr, "unknown case %s\n", kind);
        return 2;
    }
    return 0;
}
