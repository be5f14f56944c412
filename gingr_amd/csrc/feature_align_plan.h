// Planning and argument rules of the feature-based alignment (feature_align.hip; C ABI in include/gingr_hip.h: gingr_cloud_fpfh,
// gingr_feature_match, gingr_rigid_poses_from_triples): the bins of the descriptor, the test of a degenerate triple and the grid of the
// match.  Plain C++ (compiled for the host alone by tests/test_feature_alignment_host.py); nothing here touches the device.
//
// Bins.  Eleven per feature: a feature f in [-1, 1] (alpha, phi) goes to min(10, max(0, floor((f + 1) / 2 * 11))), the angle theta in
// [-pi, pi] to the same of (theta + pi) / (2 pi).  A descriptor row is 33 words: alpha bins, phi bins, theta bins.
// Triples.  A triple of pairs gives no pose when an index repeats in either triple or the squared area of either triangle is
// <= 2^-40 (longest edge)^4.
// Match.  A wave of kMatchThreads query rows scans kMatchTile rows of b at a time out of LDS; the rows of b are cut into
// match_chunks(M, N) chunks of whole tiles so that a small M still fills the device, and the chunks are combined in ascending order (a
// later chunk replaces only on a strictly smaller sum: the lowest index wins ties whatever the chunking).
#pragma once

#include "host_device.h"

#include <cmath>

namespace feature_align_plan {

constexpr int kBins = 11;            // per feature
constexpr int kWords = 3 * kBins;    // a descriptor row
constexpr int kMinK = 3, kMaxK = 64; // the neighbour list of a point is one wave
constexpr int kMaxD = 64;            // widest row of the match
constexpr double kSkip = 0x1p-40;    // |dn x u|^2 at or below: the pair is skipped; area^2 / edge^4 at or below: the triple is degenerate
constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr int kPointsPerBlock = 4;   // SPFH / FPFH kernels: a wave per point, four to a workgroup
constexpr int kMatchThreads = 64;    // query rows per workgroup of the match (a row per lane)
constexpr int kMatchTile = 32;       // rows of b staged in LDS at a time
constexpr int kMatchGroups = 2048;   // workgroups the match aims at
constexpr int kTripleThreads = 64;   // triples per workgroup (a triple per lane)

GINGR_HD inline int bin_of_unit(double f01) {
    const double b = std::floor(f01 * (double)kBins);
    return b >= (double)(kBins - 1) ? kBins - 1 : (b > 0.0 ? (int)b : 0);  // (a NaN: bin 0)
}
GINGR_HD inline int bin_of_cosine(double f) { return bin_of_unit((f + 1.0) / 2.0); }
GINGR_HD inline int bin_of_angle(double f) { return bin_of_unit((f + kPi) / (2.0 * kPi)); }

// 0: fine; 1: k outside [3, 64] or above N, or N < 1; 2: radius not above zero (a NaN included)
inline int check_fpfh(int64_t N, int k, double radius) {
    if (N < 1 || k < kMinK || k > kMaxK || (int64_t)k > N) return 1;
    if (!(radius > 0.0) || !(radius <= kDblMax)) return 2;
    return 0;
}

// padded row width of the match kernel's instantiation for D columns: 16, 40 or 64 (the padding is zeros, which add nothing)
inline int match_width(int D) { return D <= 16 ? 16 : (D <= 40 ? 40 : 64); }
inline bool check_match(int64_t M, int64_t N, int D) { return M >= 1 && N >= 1 && D >= 1 && D <= kMaxD; }

// chunks of the rows of b, and the rows of a chunk (a multiple of the tile)
inline int64_t match_chunks(int64_t M, int64_t N) {
    const int64_t groups = ceil_div(M > 0 ? M : 1, kMatchThreads), tiles = ceil_div(N > 0 ? N : 1, kMatchTile);
    int64_t c = ceil_div(kMatchGroups, groups);
    if (c > tiles) c = tiles;
    if (c < 1) c = 1;
    return ceil_div(tiles, ceil_div(tiles, c));  // (no empty chunk)
}
inline int64_t match_chunk_rows(int64_t M, int64_t N) {
    const int64_t tiles = ceil_div(N > 0 ? N : 1, kMatchTile);
    return ceil_div(tiles, match_chunks(M, N)) * kMatchTile;
}

GINGR_HD inline bool triple_repeats(const int32_t t[3]) { return t[0] == t[1] || t[0] == t[2] || t[1] == t[2]; }

// squared area <= 2^-40 (longest edge)^4, or not comparable (a NaN)
GINGR_HD inline bool triangle_degenerate(const double p0[3], const double p1[3], const double p2[3]) {
    const double e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]},
                 e2[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double c[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const double area2 = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) / 4.0;
    const double l0 = (e0[0] * e0[0] + e0[1] * e0[1]) + e0[2] * e0[2], l1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2],
                 l2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double longest = l0 > l1 ? (l0 > l2 ? l0 : l2) : (l1 > l2 ? l1 : l2);
    return !(area2 > kSkip * (longest * longest));
}

}  // namespace feature_align_plan
