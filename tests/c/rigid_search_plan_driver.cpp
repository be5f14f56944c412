// Stand-alone driver of gingr_amd/csrc/rigid_search_plan.h for tests/test_rigid_search_host.py (compiled for the host with
// -fsanitize=address,undefined): the spiral's rotations as hexadecimal floats, keep_count at products that are integral and just off,
// the slabs (a function of M and N alone that covers S exactly) and the grid of the segmented sums.
#include "rigid_search_plan.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace rs = rigid_search_plan;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    // the spiral: "rot n i r0 .. r8", "quat n i x y z w"
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)7, (int64_t)64, (int64_t)1000}) {
        std::vector<double> R((size_t)9 * n);
        rs::rotation_samples(n, R.data());
        for (int64_t i = 0; i < n; ++i) {
            double q[4];
            rs::rotation_sample_quaternion(i, n, q);
            std::printf("quat %lld %lld %a %a %a %a\n", (long long)n, (long long)i, q[0], q[1], q[2], q[3]);
            std::printf("rot %lld %lld", (long long)n, (long long)i);
            for (int k = 0; k < 9; ++k) std::printf(" %a", R[(size_t)(9 * i + k)]);
            std::printf("\n");
        }
    }

    // keep = ceil(rho M): "keep M rho keep"
    for (int64_t M : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)10, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)406, (int64_t)478,
                      (int64_t)1000, (int64_t)1000003}) {
        std::vector<double> rhos = {1.0, 0.5, 0.85, 0.6, 1e-300, std::nextafter(1.0, 0.0)};
        for (int64_t k : {(int64_t)1, M / 2, M - 1, M})
            if (k >= 1) {
                const double r = (double)k / (double)M;
                rhos.push_back(r);
                rhos.push_back(std::nextafter(r, 0.0));
                if (r < 1.0) rhos.push_back(std::nextafter(r, 2.0));
            }
        for (double rho : rhos) {
            const int64_t keep = rs::keep_count(M, rho);
            CHECK(keep >= 1 && keep <= M);
            std::printf("keep %lld %a %lld\n", (long long)M, rho, (long long)keep);
        }
    }

    // slabs: "slab M N poses"; every S is covered exactly by consecutive ranges of at most that many poses
    for (int64_t M : {(int64_t)1, (int64_t)3, (int64_t)256, (int64_t)406, (int64_t)1000, (int64_t)2000, (int64_t)4097, (int64_t)300000, (int64_t)2147483647})
        for (int64_t N : {(int64_t)1, (int64_t)7, (int64_t)1622, (int64_t)5000, (int64_t)1000000, (int64_t)2147483647}) {
            const int64_t p = rs::slab_poses(M, N);
            CHECK(p >= 1 && p <= rs::kMaxSlabPoses);
            CHECK(p == 1 || p * M <= rs::kSlabQueries);
            std::printf("slab %lld %lld %lld\n", (long long)M, (long long)N, (long long)p);
            for (int64_t S : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)128, (int64_t)1000}) {
                int64_t next = 0;
                const int64_t nb = rs::slab_count(M, N, S);
                for (int64_t b = 0; b < nb; ++b) {
                    int64_t first, count;
                    rs::slab_range(M, N, S, b, &first, &count);
                    CHECK(first == next && count >= 1 && count <= p);
                    CHECK(b == nb - 1 || count == p);
                    next = first + count;
                }
                CHECK(next == S);
            }
        }
    for (int64_t M : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1000, (int64_t)8192, (int64_t)8193, (int64_t)2147483647}) {
        const int b = rs::sum_blocks(M);
        CHECK(b >= 1 && b <= rs::kMaxSumBlocks && (b == rs::kMaxSumBlocks || (int64_t)b * rs::kSumThreads >= M));
        std::printf("blocks %lld %d\n", (long long)M, b);
    }
    std::printf(failures ? "FAILED %d\n" : "ok %d\n", failures);
    return failures ? 1 : 0;
}
