// Prints the workspace layout of the blocked SPD solve (gingr_amd/csrc/dense_spd.h: DenseSpdWork) for the padded ranks given on the
// command line, one line per rank and use: "<use> <rp> <name>=<offset in doubles> ...".  Host only: built with the plain C++ compiler by
// tests/test_dense_spd_layout_host.py.
#include "dense_spd.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const long long rp = std::atoll(argv[i]);
        const DenseSpdWork s(rp, DenseSpdWork::kRhsRows), f(rp, DenseSpdWork::kIdentity), b(rp, DenseSpdWork::kIdentity, true);
        std::printf("solve %lld Mp=%lld rows=%lld aw=%lld linv=%lld w=%lld flag=%lld doubles=%lld static=%lld\n", rp, (long long)s.Mp,
                    (long long)s.rows(), (long long)s.aw(), (long long)s.linv(), (long long)s.w(), (long long)s.flag(), (long long)s.doubles(),
                    (long long)DenseSpdWork::doubles(rp, DenseSpdWork::kRhsRows));
        std::printf("factor %lld Mp=%lld rows=%lld aw=%lld lt=%lld linv=%lld flag=%lld doubles=%lld static=%lld\n", rp, (long long)f.Mp,
                    (long long)f.rows(), (long long)f.aw(), (long long)f.lt(), (long long)f.linv(), (long long)f.flag(), (long long)f.doubles(),
                    (long long)DenseSpdWork::doubles(rp, DenseSpdWork::kIdentity));
        std::printf("binv %lld Mp=%lld rows=%lld aw=%lld lt=%lld c=%lld linv=%lld doubles=%lld static=%lld\n", rp, (long long)b.Mp,
                    (long long)b.rows(), (long long)b.aw(), (long long)b.lt(), (long long)b.c(), (long long)b.linv(), (long long)b.doubles(),
                    (long long)DenseSpdWork::doubles(rp, DenseSpdWork::kIdentity, true));
    }
    return 0;
}
