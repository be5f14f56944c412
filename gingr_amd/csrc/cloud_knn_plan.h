// Planning of the k-nearest-neighbour search of a cloud within itself (cloud_knn.hip): the uniform grid over the cloud's bounding box.
// Plain C++ (compiled for the host alone by tests/test_cloud_normals_host.py); cell_of is also what the device evaluates per point.
//
// The cell edge h.  A query first scans the cells [c - 1, c + 1]^3 around its own; its list is exact once the k-th distance is at most h
// (cloud_knn.hip), so h should be about the radius of a ball that holds k points with some to spare -- 2 k here.  What that radius is
// depends on how the cloud fills its box, which the box alone does not say.  Two models, N points each:
//   a volume   the box filled evenly:                  N (4 pi / 3) h^3 / (e0 e1 e2)                       points within h
//   a surface  a sheet of about the box's own area:    N pi h^2 / A,  A = 2 (e0 e1 + e0 e2 + e1 e2)        points within h
// (a box with one flat axis: the sheet e0 e1; with two: the line, N 2 h / e0).  The SMALLER of the two radii is taken: too small an h
// costs some queries a second pass over [c - R, c + R]^3 with the R their k-th distance asks for, too large an h costs every query a
// longer scan.  Scans, targets of this search, are surfaces: the surface model sets h there whenever the box is not much larger than the
// sheet in it.  The grid is then coarsened until it has at most 1024 cells per axis and 8 N + 4096 cells in all, as nn_grid.hip does.
#pragma once

#include "host_device.h"

#include <cmath>

namespace cloud_knn_plan {

constexpr int kMinK = 3, kMaxK = 64;
constexpr int kMaxR = 4;             // largest half-width (in cells) of the block a query scans: 9^3 cells
constexpr int kMaxRowPoints = 1024;  // a row of cells (a run along x) with more points is not scanned by the grid kernel: the query is flagged
constexpr int kMaxAxisCells = 1024;
constexpr double kSpare = 2.0;       // points wanted within h, in units of k
constexpr double kPi = 3.14159265358979323846;

struct Plan {
    double lo[3] = {0, 0, 0};
    double h = 1.0, inv_h = 1.0;
    int32_t g[3] = {1, 1, 1};
    int dims = 0;  // axes along which the cloud extends
    int64_t ncells() const { return (int64_t)g[0] * g[1] * g[2]; }
};

// lanes that serve one query: the list has one entry per lane, so the smallest of 16, 32, 64 that holds k
inline int group_lanes(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }

// floor(f) clamped to [0, g - 1]; the expression the grid is filled by and every query is located by
GINGR_HD inline int32_t cell_of(double x, double lo, double inv_h, int32_t g) {
    const double c = floor((x - lo) * inv_h);
    return c >= (double)(g - 1) ? g - 1 : (c > 0.0 ? (int32_t)c : 0);
}

// lo / hi: the bounding box of the N >= 1 finite points
inline Plan make_plan(int64_t N, int k, const double lo[3], const double hi[3]) {
    Plan p;
    double e[3], maxext = 0.0;
    for (int d = 0; d < 3; ++d) {
        p.lo[d] = lo[d];
        e[d] = hi[d] - lo[d];
        if (e[d] > maxext) maxext = e[d];
    }
    double h = 1.0;
    if (maxext > 0.0) {
        double ext[3];
        int dims = 0;
        for (int d = 0; d < 3; ++d)
            if (e[d] > 1e-9 * maxext) ext[dims++] = e[d];
        p.dims = dims;
        const double want = kSpare * (double)k / (double)N;  // the fraction of the cloud wanted within h
        if (dims == 3) {
            const double hv = std::cbrt(want * ext[0] * ext[1] * ext[2] * 3.0 / (4.0 * kPi));
            const double hs = std::sqrt(want * 2.0 * (ext[0] * ext[1] + ext[0] * ext[2] + ext[1] * ext[2]) / kPi);
            h = hv < hs ? hv : hs;
        } else if (dims == 2) {
            h = std::sqrt(want * ext[0] * ext[1] / kPi);
        } else {
            h = 0.5 * want * ext[0];
        }
        if (!(h > 1e-12 * maxext)) h = 1e-12 * maxext;
    }
    for (;;) {
        double cells = 1.0;
        bool fine = true;
        for (int d = 0; d < 3; ++d) {
            const double c = std::floor(e[d] / h) + 1.0;
            if (c > (double)kMaxAxisCells) fine = false;
            p.g[d] = (int32_t)(c < (double)kMaxAxisCells ? c : (double)kMaxAxisCells);
            cells *= c < 1e9 ? c : 1e9;
        }
        const double most = 8.0 * (double)N + 4096.0;
        if (fine && cells <= (most < 1073741824.0 ? most : 1073741824.0)) break;  // (cell indices are 32-bit on the device)
        h *= 1.25;
    }
    p.h = h;
    p.inv_h = 1.0 / h;
    return p;
}

}  // namespace cloud_knn_plan
