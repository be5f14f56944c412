// Planning of the exact order statistic over non-negative doubles (robust_select.hip): the selection key, the radix digits and the grid.
// Plain C++ (compiled for the host alone by tests/test_plane_robust_host.py); key_of / digit_of are also what the device evaluates.
//
// The key.  A non-negative IEEE double orders as its bit pattern read as an unsigned 64-bit integer: +0 is 0, the denormals follow,
// then the normal numbers, +inf = 0x7FF0000000000000 above every finite value.  A row that takes no part (not observed) gets kSentinel,
// all ones, which no non-negative double has (a pattern above +inf with the sign bit clear is a NaN; all ones has the sign bit set).
// The selection.  kPasses digits of kDigitBits bits, most significant first.  Pass p counts, per workgroup in LDS, the digit p of the
// keys whose digits 0 .. p - 1 are the ones chosen so far, and writes its 2^kDigitBits counts; the bucket that holds rank k is the
// first whose running total exceeds k, and k loses the total below it.  After the last pass the chosen digits ARE the key of rank k.
// 8 bits x 8 passes: a workgroup of 256 threads owns one bin per thread when it sums the partial counts, the histogram is 1 KiB of
// LDS, and a pass's partials are 1 KiB per workgroup -- with at most kMaxGroups workgroups every workgroup of the next pass reads at most
// 64 KiB to re-derive the bucket.  Wider digits (11 bits x 6 passes) would save two launches and read eight times as much per workgroup.
#pragma once

#include "host_device.h"

#include <cstring>

namespace robust_select_plan {

constexpr int kDigitBits = 8;
constexpr int kBins = 1 << kDigitBits;
constexpr int kPasses = 64 / kDigitBits;  // every bit of the key belongs to exactly one digit
constexpr int kThreads = 256;             // == kBins: one bin per thread
constexpr int kItemsPerThread = 8;        // keys a thread counts before the grid is grown
constexpr int kMaxGroups = 64;            // workgroups of a pass: beyond, each strides over the keys
constexpr int64_t kMaxKeys = 2147483647;  // counts are 32-bit
constexpr uint64_t kSentinel = ~(uint64_t)0;

static_assert(kPasses * kDigitBits == 64, "the digits cover the key");
static_assert(kThreads == kBins, "one bin per thread");

// bits of a double that is >= 0 (the caller's business; -0 is made +0 by adding 0 first)
GINGR_HD inline uint64_t key_of(double s) {
    uint64_t k;
#if defined(__HIP_DEVICE_COMPILE__)
    k = (uint64_t)__double_as_longlong(s);
#else
    std::memcpy(&k, &s, sizeof k);
#endif
    return k;
}

GINGR_HD inline double value_of(uint64_t k) {
    double s;
#if defined(__HIP_DEVICE_COMPILE__)
    s = __longlong_as_double((long long)k);
#else
    std::memcpy(&s, &k, sizeof s);
#endif
    return s;
}

// bits to the right of digit p (p = 0: the most significant)
GINGR_HD inline int shift_of(int p) { return 64 - kDigitBits * (p + 1); }
GINGR_HD inline unsigned digit_of(uint64_t key, int p) { return (unsigned)(key >> shift_of(p)) & (unsigned)(kBins - 1); }
// digits 0 .. p - 1 of the key, right-aligned (p = 0: nothing, 0)
GINGR_HD inline uint64_t prefix_of(uint64_t key, int p) { return p == 0 ? 0 : key >> (64 - kDigitBits * p); }

// workgroups of one counting pass over n keys
inline int groups(int64_t n) {
    const int64_t per = (int64_t)kThreads * kItemsPerThread;
    int64_t g = n > 0 ? ceil_div(n, per) : 1;
    if (g > kMaxGroups) g = kMaxGroups;
    return (int)g;
}

// 32-bit words of the partial counts of all passes: [kPasses][groups][kBins]
inline int64_t count_words(int64_t n) { return (int64_t)kPasses * groups(n) * kBins; }

// the lower median's rank among n > 0 values
GINGR_HD inline int64_t lower_median_rank(int64_t n) { return (n - 1) / 2; }

}  // namespace robust_select_plan
