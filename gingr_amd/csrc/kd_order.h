// Spatial order for the tile culling: recursive median split along the longest axis of the bounding box (a balanced k-d
// tree laid out in leaf order).  Leaves are 256-point tiles; the left half of a split takes the larger number of whole leaves, so
// every tile is one leaf -- a compact box, which is what the per-tile / per-workgroup bounding boxes of the CPD kernels need (a
// Z-curve order has seams whose chunks span the whole domain).  When the number of leaves is a power of two, every aligned run of
// 256 * 2^k points is one tree node as well; otherwise only the runs the cuts produce are (five leaves: the top cut is at 768).
// Deterministic: ties are broken by the original index.
// The points travel with their index (32-byte records, permuted in place): every pass is a contiguous sweep, and the two halves of
// the upper levels go to separate threads.  The result does not depend on either -- each split is the unique median cut of the total
// order (coordinate, original index), and the quarters are sorted by index at the end.
// Plain C++: cloud_ops.hip holds the library's one out-of-line kd_leaf_order, tests/c/kd_order_driver.cpp runs this on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <system_error>
#include <thread>
#include <vector>

struct KdPoint {
    double c[3];
    int64_t idx;
};

// How much of the work goes to threads of its own; the order that comes out is the same for every value.
struct KdParallel {
    int split_levels = 4;        // upper tree levels whose halves go to separate threads: up to sixteen
    int leaf_threads = 8;        // threads of the pass over the leaves
    int64_t min_points = 16384;  // (sub)clouds below this are not worth a thread
    static KdParallel serial() { return KdParallel{0, 1, 0}; }
};

inline void kd_split(KdPoint *p, int64_t n, int64_t leaf, int par_levels, int64_t par_min_points) {
    if (n <= leaf) return;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            const double v = p[i].c[d];
            if (v == v) {
                if (v < lo[d]) lo[d] = v;
                if (v > hi[d]) hi[d] = v;
            }
        }
    int ax = 0;
    for (int d = 1; d < 3; ++d)
        if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
    // left half gets a multiple of `leaf` points so that leaves stay aligned to 256-point tiles
    int64_t half = ((n / leaf + 1) / 2) * leaf;
    if (half >= n) half = n / 2;
    std::nth_element(p, p + half, p + n, [ax](const KdPoint &a, const KdPoint &b) {
        const double ka = a.c[ax] == a.c[ax] ? a.c[ax] : 1e300, kb = b.c[ax] == b.c[ax] ? b.c[ax] : 1e300;  // NaN coordinates sort last
        return ka < kb || (ka == kb && a.idx < b.idx);
    });
    if (par_levels > 0 && n >= par_min_points) {
        std::thread left;
        try {
            left = std::thread([=] { kd_split(p, half, leaf, par_levels - 1, par_min_points); });
        } catch (const std::system_error &) {  // no thread to be had: this half inline as well
            kd_split(p, half, leaf, 0, par_min_points);
        }
        kd_split(p + half, n - half, leaf, par_levels - 1, par_min_points);
        if (left.joinable()) left.join();
    } else {
        kd_split(p, half, leaf, 0, par_min_points);
        kd_split(p + half, n - half, leaf, 0, par_min_points);
    }
}

// perm[s] = original index of the point (of the n interleaved xyz) stored at position s of the k-d leaf order
inline void kd_leaf_order(const double *xyz, int64_t n, std::vector<int32_t> &perm, const KdParallel &par) {
    std::vector<KdPoint> pts((size_t)n);
    for (int64_t i = 0; i < n; ++i) pts[(size_t)i] = KdPoint{{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, i};
    kd_split(pts.data(), n, 256, par.split_levels, par.min_points);
    // every 256-point leaf is split further into four spatially compact 64-point quarters (the unit of the fine exact-zero
    // culling: one owned slot of a wave, one quarter of a streamed tile); original order inside a quarter (reproducible)
    perm.resize((size_t)n);
    auto leaves = [&](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; b += 256) {
            const int64_t m = b + 256 < n ? 256 : n - b;
            kd_split(pts.data() + b, m, 64, 0, 0);
            for (int64_t i = 0; i < m; ++i) perm[(size_t)(b + i)] = (int32_t)pts[(size_t)(b + i)].idx;
            for (int64_t q = 0; q < m; q += 64) std::sort(perm.begin() + b + q, perm.begin() + b + (q + 64 < m ? q + 64 : m));
        }
    };
    const int64_t nleaves = (n + 255) / 256;
    const int nt = par.leaf_threads;
    if (nt > 1 && n >= par.min_points) {
        std::vector<std::thread> th((size_t)(nt - 1));
        for (int t = 1; t < nt; ++t) {
            const int64_t b0 = nleaves * t / nt * 256, b1 = nleaves * (t + 1) / nt * 256;
            try {
                th[(size_t)(t - 1)] = std::thread(leaves, b0, b1);
            } catch (const std::system_error &) {
                leaves(b0, b1);
            }
        }
        leaves(0, nleaves / nt * 256);
        for (std::thread &t : th)
            if (t.joinable()) t.join();
    } else {
        leaves(0, nleaves * 256);
    }
}
