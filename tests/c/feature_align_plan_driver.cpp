// Stand-alone driver of gingr_amd/csrc/feature_align_plan.h for tests/test_feature_alignment_host.py (compiled for the host with
// -fsanitize=address,undefined): the bins at and beside every edge as hexadecimal floats, the argument rules of the descriptor, the
// chunks of the match (whole tiles, no empty chunk, every row covered once) and the degenerate-triple test on given triangles.
#include "feature_align_plan.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace fap = feature_align_plan;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    // "bin c f bin" (alpha, phi) and "bin a f bin" (theta): every edge, its two neighbours, the ends and beyond
    for (int b = 0; b <= fap::kBins; ++b) {
        const double ec = -1.0 + 2.0 * b / fap::kBins, ea = -fap::kPi + 2.0 * fap::kPi * b / fap::kBins;
        for (double f : {std::nextafter(ec, -2.0), ec, std::nextafter(ec, 2.0)}) std::printf("bin c %a %d\n", f, fap::bin_of_cosine(f));
        for (double f : {std::nextafter(ea, -4.0), ea, std::nextafter(ea, 4.0)}) std::printf("bin a %a %d\n", f, fap::bin_of_angle(f));
    }
    for (double f : {0.0, -0.0, 0.3, -0.7, 1.5, -1.5, 1e300, -1e300}) {
        std::printf("bin c %a %d\n", f, fap::bin_of_cosine(f));
        std::printf("bin a %a %d\n", f, fap::bin_of_angle(f));
    }
    CHECK(fap::bin_of_cosine(std::numeric_limits<double>::quiet_NaN()) == 0);
    CHECK(fap::bin_of_cosine(0.0) == 5 && fap::bin_of_angle(0.0) == 5);  // the centre bins of a plane
    CHECK(fap::kWords == 33);

    // "fpfh N k radius code"
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (long long N : {0LL, 1LL, 2LL, 3LL, 64LL, 65LL, 1622LL})
        for (int k : {0, 2, 3, 4, 63, 64, 65})
            for (double r : {25.0, 1e-300, 0.0, -1.0, nan, inf})
                std::printf("fpfh %lld %d %a %d\n", N, k, r, fap::check_fpfh(N, k, r));
    for (int D : {0, 1, 16, 17, 33, 40, 41, 64, 65}) std::printf("match %d %d %d\n", D, (int)fap::check_match(1, 1, D), fap::match_width(D));
    CHECK(!fap::check_match(0, 1, 3) && !fap::check_match(1, 0, 3));

    // "chunks M N chunks rows"
    for (int64_t M : {(int64_t)1, (int64_t)3, (int64_t)64, (int64_t)65, (int64_t)300, (int64_t)2000, (int64_t)50000, (int64_t)2147483647})
        for (int64_t N : {(int64_t)1, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)64, (int64_t)257, (int64_t)1025, (int64_t)1622, (int64_t)50000,
                          (int64_t)2147483647}) {
            const int64_t c = fap::match_chunks(M, N), rows = fap::match_chunk_rows(M, N);
            CHECK(c >= 1 && c <= fap::kMatchGroups && rows >= fap::kMatchTile && rows % fap::kMatchTile == 0);
            CHECK(c * rows >= N);        // every row is in a chunk
            CHECK((c - 1) * rows < N);   // and no chunk is empty
            std::printf("chunks %lld %lld %lld %lld\n", (long long)M, (long long)N, (long long)c, (long long)rows);
        }

    // "tri x0 .. z2 degenerate" and the repeated index
    const double tris[][9] = {
        {0, 0, 0, 1, 0, 0, 0, 1, 0},              // a right triangle
        {0, 0, 0, 1, 0, 0, 2, 0, 0},              // collinear
        {0, 0, 0, 1, 0, 0, 2, 1e-7, 0},           // area^2 / edge^4 = 1e-14 / 64: below 2^-40
        {0, 0, 0, 1, 0, 0, 2, 1e-5, 0},           // 1e-10 / 64 = 1.6e-12: above 2^-40 = 9.1e-13
        {5, 5, 5, 5, 5, 5, 5, 5, 5},              // one point three times
        {1e150, 0, 0, 0, 1e150, 0, 0, 0, 1e150},  // the fourth power overflows: not comparable, degenerate
        {100.5, -3.25, 7, 130, 12.5, -40, 90, 60, 33},
    };
    for (const auto &t : tris) {
        std::printf("tri");
        for (double v : t) std::printf(" %a", v);
        std::printf(" %d\n", (int)fap::triangle_degenerate(t, t + 3, t + 6));
    }
    const int32_t r0[3] = {1, 2, 3}, r1[3] = {1, 1, 3}, r2[3] = {1, 2, 1}, r3[3] = {0, 2, 2};
    CHECK(!fap::triple_repeats(r0) && fap::triple_repeats(r1) && fap::triple_repeats(r2) && fap::triple_repeats(r3));
    std::printf(failures ? "FAILED %d\n" : "ok %d\n", failures);
    return failures ? 1 : 0;
}
