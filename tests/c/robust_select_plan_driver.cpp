// Stand-alone driver of gingr_amd/csrc/robust_select_plan.h for tests/test_plane_robust_host.py (compiled for the host with
// -fsanitize=address,undefined): the digits cover the 64 bits of a key exactly once, the grid at the sizes the GPU tests use, the key
// order on zeros, denormals and +inf, and the selection itself -- the passes of robust_select.hip replayed on the host with the header's
// digit_of / prefix_of, group by group, against a sort.
#include "robust_select_plan.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

namespace rsp = robust_select_plan;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                            \
        }                                                          \
    } while (0)

// the device's passes: per group a histogram of digit p over the keys that carry the chosen prefix, the bucket from the summed counts
static uint64_t select_key(const std::vector<uint64_t> &keys, int64_t k) {
    const int64_t n = (int64_t)keys.size();
    const int G = rsp::groups(n);
    std::vector<uint32_t> counts((size_t)rsp::count_words(n), 0u);
    uint64_t prefix = 0, rank = (uint64_t)k;
    for (int p = 0; p < rsp::kPasses; ++p) {
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < rsp::kThreads; ++t)
                for (int64_t i = (int64_t)g * rsp::kThreads + t; i < n; i += (int64_t)G * rsp::kThreads)
                    if (rsp::prefix_of(keys[(size_t)i], p) == prefix) ++counts[((size_t)p * G + g) * rsp::kBins + rsp::digit_of(keys[(size_t)i], p)];
        uint64_t below = 0;
        int bucket = rsp::kBins - 1;
        for (int b = 0; b < rsp::kBins; ++b) {
            uint64_t total = 0;
            for (int g = 0; g < G; ++g) total += counts[((size_t)p * G + g) * rsp::kBins + b];
            if (below <= rank && rank < below + total) {
                bucket = b;
                break;
            }
            below += total;
        }
        prefix = (prefix << rsp::kDigitBits) | (uint64_t)bucket;
        rank -= below;
    }
    return prefix;
}

int main() {
    // digits: every bit of the key in exactly one digit
    uint64_t covered = 0;
    for (int p = 0; p < rsp::kPasses; ++p) {
        const uint64_t mask = (uint64_t)(rsp::kBins - 1) << rsp::shift_of(p);
        CHECK((covered & mask) == 0);
        covered |= mask;
        CHECK(rsp::shift_of(p) >= 0 && rsp::shift_of(p) + rsp::kDigitBits <= 64);
    }
    CHECK(covered == ~(uint64_t)0);
    std::printf("digits %d bits x %d passes, %d bins, %d threads, covered %016llx\n", rsp::kDigitBits, rsp::kPasses, rsp::kBins, rsp::kThreads,
                (unsigned long long)covered);
    const uint64_t probe = 0x0123456789ABCDEFull;
    uint64_t rebuilt = 0;
    for (int p = 0; p < rsp::kPasses; ++p) {
        CHECK(rsp::prefix_of(probe, p) == rebuilt);
        rebuilt = (rebuilt << rsp::kDigitBits) | rsp::digit_of(probe, p);
    }
    CHECK(rebuilt == probe);

    // grid
    const int64_t sizes[] = {1, 2, 255, 256, 257, 1000, 2048, 2049, 65537, 50000, 1000000, rsp::kMaxKeys};
    for (int64_t n : sizes) {
        const int g = rsp::groups(n);
        CHECK(g >= 1 && g <= rsp::kMaxGroups);
        CHECK(g == rsp::kMaxGroups || (int64_t)g * rsp::kThreads * rsp::kItemsPerThread >= n);
        CHECK(rsp::count_words(n) == (int64_t)rsp::kPasses * g * rsp::kBins);
        std::printf("groups %lld %d %lld\n", (long long)n, g, (long long)rsp::count_words(n));
    }
    CHECK(rsp::groups(0) == 1);
    CHECK(rsp::lower_median_rank(1) == 0 && rsp::lower_median_rank(2) == 0 && rsp::lower_median_rank(3) == 1 && rsp::lower_median_rank(4) == 1);

    // key order
    const double inf = std::numeric_limits<double>::infinity();
    const double ladder[] = {0.0, 4.9406564584124654e-324, 9.8813129168249309e-324, DBL_MIN / 2, DBL_MIN, 1e-300, 1.0, 1.0 + DBL_EPSILON, 2.0, 1e300,
                             DBL_MAX, inf};
    for (size_t i = 0; i + 1 < sizeof ladder / sizeof *ladder; ++i) CHECK(rsp::key_of(ladder[i]) < rsp::key_of(ladder[i + 1]));
    CHECK(rsp::key_of(0.0) == 0 && rsp::key_of(inf) == 0x7FF0000000000000ull && rsp::key_of(inf) < rsp::kSentinel);
    CHECK(rsp::key_of(-0.0 + 0.0) == 0);
    for (double v : ladder) CHECK(rsp::key_of(rsp::value_of(rsp::key_of(v))) == rsp::key_of(v));
    std::printf("keys zero %016llx denormal %016llx inf %016llx sentinel %016llx\n", (unsigned long long)rsp::key_of(0.0),
                (unsigned long long)rsp::key_of(ladder[1]), (unsigned long long)rsp::key_of(inf), (unsigned long long)rsp::kSentinel);

    // the selection against a sort
    std::mt19937_64 rng(5);
    int checked = 0;
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1000, (int64_t)5000}) {
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<uint64_t> keys((size_t)n);
            for (auto &key : keys) {
                const double x = std::ldexp((double)(rng() >> 11), -53);
                switch (kind) {
                    case 0: key = rsp::key_of(x * 100.0); break;
                    case 1: key = rsp::key_of(3.5); break;
                    case 2: key = rsp::key_of((double)(rng() % 4)); break;
                    case 3: key = rng() % 3 ? (rng() % 7) : 0; break;                          // zeros among denormals
                    default: key = rng() % 5 ? rsp::key_of(x) : rsp::kSentinel; break;         // rows that take no part
                }
            }
            if (kind == 0 && n > 2) keys[(size_t)(n / 2)] = rsp::key_of(inf);
            std::vector<uint64_t> sorted = keys;
            std::sort(sorted.begin(), sorted.end());
            for (int64_t k : {(int64_t)0, (n - 1) / 2, n - 1}) {
                CHECK(select_key(keys, k) == sorted[(size_t)k]);
                ++checked;
            }
        }
    }
    std::printf("selections %d\n", checked);
    std::printf(failures ? "FAILED %d\n" : "ok %d\n", failures);
    return failures ? 1 : 0;
}
