// Planning of the batched multi-start trimmed rigid ICP (rigid_search.hip; C ABI in include/gingr_hip.h: gingr_rigid_search,
// gingr_rotation_samples): the start rotations, the size of the kept set, the slabs of poses and the grids of the segmented kernels.
// Plain C++ (compiled for the host alone by tests/test_rigid_search_host.py); nothing here touches the device.
//
// Start rotations.  The super-Fibonacci spiral (M. Alexa, "Super-Fibonacci Spirals: Fast, Low-Discrepancy Sampling of SO(3)", CVPR
// 2022): a closed form for any n, with phi = sqrt 2 and psi = 1.533751168755204288118041.  For s = i + 1/2, r = sqrt(s / n),
// R = sqrt(1 - s / n), alpha = 2 pi s / phi, beta = 2 pi s / psi the unit quaternion (x, y, z, w) = (r sin alpha, r cos alpha,
// R sin beta, R cos beta).
// The kept set.  keep = ceil(rho M), evaluated on the float64 product rho * M and clamped to [1, M]; the pairs kept are those whose
// squared distance is <= the order statistic of rank keep - 1, ties included.
// Slabs.  The poses advance in slabs of slab_poses(M, N) poses, so that the query cloud (poses x M points), its matches and the
// workspace of the search stay bounded whatever S is.  The slab depends on M and N alone -- never on S -- and no sum of a pose reaches
// across poses, so a pose's result does not depend on the slab it runs in or on its place there.
#pragma once

#include "host_device.h"

#include <cmath>

namespace rigid_search_plan {

constexpr double kPhi = 1.41421356237309504880168872420969808;  // sqrt 2
constexpr double kPsi = 1.533751168755204288118041;
constexpr double kTwoPi = 6.28318530717958647692528676655900577;

constexpr int kPoseWords = 12;                 // a pose: R row-major, then t
constexpr int kSums = 17;                      // count, sum p~ (3), sum y~ (3), sum y~ p~^T (9), sum d2 over the kept pairs
constexpr int kSumThreads = 256;               // threads of a workgroup of the segmented sums
constexpr int kMaxSumBlocks = 32;              // workgroups per pose of the segmented sums: beyond, each strides over the points
constexpr int kStepThreads = 64;               // poses per workgroup of the pose step (one lane each)
constexpr int kMaxSlabPoses = 64;              // poses per slab at most: one wave of the pose step
constexpr int64_t kSlabQueries = 1 << 18;      // query points per slab (unless one pose alone has more)
constexpr int64_t kSlabTargetWork = (int64_t)1 << 34;  // queries x targets per slab: bounds the masked tile scan of a slab of bad starts

// rotation matrix (row-major) of the unit quaternion (x, y, z, w)
inline void quaternion_to_rotation(double x, double y, double z, double w, double R[9]) {
    R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - z * w), R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w), R[7] = 2.0 * (y * z + x * w), R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// sample i of n of the spiral as a quaternion (x, y, z, w)
inline void rotation_sample_quaternion(int64_t i, int64_t n, double q[4]) {
    const double s = (double)i + 0.5;
    const double r = std::sqrt(s / (double)n), R = std::sqrt(1.0 - s / (double)n);
    const double alpha = kTwoPi * s / kPhi, beta = kTwoPi * s / kPsi;
    q[0] = r * std::sin(alpha), q[1] = r * std::cos(alpha), q[2] = R * std::sin(beta), q[3] = R * std::cos(beta);
}

// the n rotations of the spiral, row-major [n][9]
inline void rotation_samples(int64_t n, double *rotations9) {
    for (int64_t i = 0; i < n; ++i) {
        double q[4];
        rotation_sample_quaternion(i, n, q);
        quaternion_to_rotation(q[0], q[1], q[2], q[3], rotations9 + 9 * i);
    }
}

// ceil(rho M) of the float64 product, in [1, M] (M >= 1, 0 < rho <= 1)
inline int64_t keep_count(int64_t M, double rho) {
    const double c = std::ceil(rho * (double)M);
    int64_t k = c >= (double)M ? M : (int64_t)c;
    if (k < 1) k = 1;
    return k;
}

// poses per slab: a function of M and N alone
inline int64_t slab_poses(int64_t M, int64_t N) {
    int64_t p = kSlabQueries / (M > 0 ? M : 1);
    const int64_t per_pose = (M > 0 ? M : 1) * (N > 0 ? N : 1);
    const int64_t q = kSlabTargetWork / per_pose;
    if (q < p) p = q;
    if (p > kMaxSlabPoses) p = kMaxSlabPoses;
    if (p < 1) p = 1;
    return p;
}

inline int64_t slab_count(int64_t M, int64_t N, int64_t S) { return ceil_div(S, slab_poses(M, N)); }
// the poses [first, first + count) of slab b
inline void slab_range(int64_t M, int64_t N, int64_t S, int64_t b, int64_t *first, int64_t *count) {
    const int64_t p = slab_poses(M, N);
    *first = b * p;
    *count = S - *first < p ? S - *first : p;
}

// workgroups per pose of the segmented sums: a function of M alone
inline int sum_blocks(int64_t M) {
    int64_t b = ceil_div(M > 0 ? M : 1, kSumThreads);
    if (b > kMaxSumBlocks) b = kMaxSumBlocks;
    return (int)b;
}

}  // namespace rigid_search_plan
