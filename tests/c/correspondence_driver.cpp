// Stand-alone driver of gingr_amd/csrc/correspondence.h for tests/test_correspondence_host.py (host compiler, sanitizers on).
//   correspondence_driver enum                      the four Flavour values
//   correspondence_driver facts                     one line per (kind, reversed, surface method, landmarks) with every derived fact
//   correspondence_driver validate < requests       per line "flavour cpd? w lambda icp? max_iterations" (pointers: 0 null, 1 given;
//                                                   numbers as strtod reads them) -> "error kind w lambda max_iterations"
#include "correspondence.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "enum")) {
        printf("%d %d %d %d\n", (int)Flavour::Cpd, (int)Flavour::IcpCloud, (int)Flavour::IcpSurface, (int)Flavour::Pairs);
        return 0;
    }
    if (!strcmp(argv[1], "facts")) {
        for (int kind = 0; kind < 4; ++kind)
            for (int reversed = 0; reversed < 2; ++reversed)
                for (int method = 0; method < 2; ++method)
                    for (int n_lm = 0; n_lm < 2; ++n_lm) {
                        const gingr_cpd_params cp{0.1, 2.0};
                        const gingr_icp_params ip{4.0, 1.0, 10};
                        Correspondence c;
                        if (make_correspondence(kind, &cp, &ip, &c) != CorrespondenceError::None) return 3;
                        printf("%d %d %d %d : %d %d %d %d %d %d %d %d %d %d\n", kind, reversed, method, n_lm, (int)is_icp_schedule(c),
                               (int)post_solve_sigma2_rule(c), (int)needs_meshes(c), (int)needs_gathered_fit(c, reversed != 0),
                               (int)exchanges_segment0(c), (int)exchanges_reversal_sums(c, reversed != 0),
                               (int)uniform_weights(c, reversed != 0, n_lm), (int)zero_one_weights(c, reversed != 0),
                               (int)reversed_icp(c, reversed != 0), memo_flavour_key(c, method, reversed != 0));
                    }
        return 0;
    }
    if (strcmp(argv[1], "validate")) return 2;
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        int flavour, has_cp, has_ip, max_it;
        char ws[64], ls[64];
        if (sscanf(line, "%d %d %63s %63s %d %d", &flavour, &has_cp, ws, ls, &has_ip, &max_it) != 6) return 4;
        const gingr_cpd_params cp{strtod(ws, nullptr), strtod(ls, nullptr)};
        const gingr_icp_params ip{4.0, 1.0, max_it};
        Correspondence c;
        const CorrespondenceError e = make_correspondence(flavour, has_cp ? &cp : nullptr, has_ip ? &ip : nullptr, &c);
        if (e != correspondence_error(c) || e != correspondence_error(abi_correspondence(flavour, has_cp ? &cp : nullptr, has_ip ? &ip : nullptr)))
            return 5;
        printf("%d %d %a %a %d\n", (int)e, (int)c.kind, c.cpd.w, c.cpd.lambda, (int)c.icp.max_iterations);
    }
    return 0;
}
