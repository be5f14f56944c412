// Stand-alone driver of gingr_amd/csrc/bcpd_math.h for tests/test_bcpd_host.py (built with the address and undefined-behaviour
// sanitizers).  stdin: doubles {mode, count, payload}; stdout: doubles.
//   mode 0  digamma: count arguments                                        -> count values
//   mode 1  similarity finish: count records {Sxu 9, Phi 9, Psi 9, tr_Suu, xbar 3, ubar 3}  -> count records {s, R 9, t 3}
//   mode 2  chunk planner: count records {owners, streamed}                 -> count records {chunks, length}
//   mode 3  alpha: {kappa, psi_total, M} then count values of nu           -> count values
#include <cstdio>
#include <vector>

#include "bcpd_math.h"

int main() {
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
    if (in.size() < 2) return 2;
    const int mode = (int)in[0];
    const size_t count = (size_t)in[1];
    const double *p = in.data() + 2;
    const size_t have = in.size() - 2;
    std::vector<double> out;
    if (mode == 0) {
        if (have != count) return 3;
        for (size_t i = 0; i < count; ++i) out.push_back(bcpd_digamma(p[i]));
    } else if (mode == 1) {
        if (have != count * 34) return 3;
        for (size_t i = 0; i < count; ++i) {
            const double *r = p + i * 34;
            double o[13];
            bcpd_similarity_finish(r, r + 9, r + 18, r[27], r + 28, r + 31, o);
            out.insert(out.end(), o, o + 13);
        }
    } else if (mode == 2) {
        if (have != count * 2) return 3;
        for (size_t i = 0; i < count; ++i) {
            const BcpdChunks c = bcpd_plan_chunks((int64_t)p[2 * i], (int64_t)p[2 * i + 1]);
            out.push_back((double)c.count);
            out.push_back((double)c.length);
        }
    } else if (mode == 3) {
        if (have != count + 3) return 3;
        for (size_t i = 0; i < count; ++i) out.push_back(bcpd_alpha(p[0], p[3 + i], p[1], p[2]));
    } else {
        return 4;
    }
    fwrite(out.data(), sizeof(double), out.size(), stdout);
    return 0;
}
