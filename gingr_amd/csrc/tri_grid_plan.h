// The host side of the uniform grid over the (fixed) triangles of a mesh: the clamped cell index every grid user evaluates -- host
// binning and device searches alike -- and the binning itself, as plain vectors.  No HIP in here: tri_grid_build (surface_grid.hip)
// uploads the plan, tests/c/tri_grid_plan_driver.cpp runs it on the host under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_device.h"

constexpr int kTriRec = 10;          // doubles per grid entry behind its box: corners A, B, C, {position | original index << 32}
constexpr int kTriGridMaxSpan = 3;   // a listed triangle's box spans at most this many cell steps per axis (wider ones: the short list)
constexpr int kTriGridMaxBig = 256;  // entries of the short list of a fixed mesh; more: no grid

// The cell of grid coordinate f = (x - lo) * inv_h on an axis of gd cells: floor, clamped to [0, gd - 1] (NaN: cell 0).  The grid
// searches are exact because the binning and every query evaluate THIS expression, which is monotone in x.
GINGR_HD inline int32_t grid_clamp_cell(double f, int32_t gd) {
    const double c = floor(f);
    return c >= (double)(gd - 1) ? gd - 1 : (c > 0.0 ? (int32_t)c : 0);
}
GINGR_HD inline int32_t grid_cell_of(double x, double lo, double inv_h, int32_t gd) { return grid_clamp_cell((x - lo) * inv_h, gd); }

struct TriGridPlan {
    double lo[3] = {0.0, 0.0, 0.0}, h = 0.0, inv_h = 0.0;
    int32_t g[3] = {1, 1, 1}, span[3] = {0, 0, 0};  // span: largest extent (in cell steps) of a listed triangle's box per axis
    std::vector<int32_t> start;        // [g0 g1 g2 + 1], x fastest
    std::vector<int32_t> list;         // triangle (position in `tri`) of every entry: by cell, then the wide ones
    std::vector<double> boxes, recs;   // per entry: [6] box, [kTriRec] corners + {position | original index << 32}
    int64_t n_listed = 0, n_big = 0;
    bool ready = false;  // false: no grid (no finite triangle, zero or infinite extent, too many wide triangles); nothing else is valid
};

// vsoa: the mesh vertices as SoA planes [3][n]; tri: [3 T] vertex positions, in the triangle order the entries refer to; tri_orig
// (nullable): original number of every triangle.
inline void tri_grid_plan(const double *vsoa, int64_t n, const int32_t *tri, const int32_t *tri_orig, int64_t T, TriGridPlan *p) {
    *p = TriGridPlan{};
    if (T < 1 || T > INT32_MAX || n < 1) return;
    double *lo = p->lo, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    lo[0] = lo[1] = lo[2] = HUGE_VAL;
    std::vector<double> tb((size_t)6 * T);
    std::vector<char> good((size_t)T, 0);
    double ext_sum = 0.0;
    int64_t ngood = 0;
    for (int64_t t = 0; t < T; ++t) {
        double bl[3], bh[3];
        bool fin = true;
        for (int d = 0; d < 3; ++d) {
            const double a = vsoa[(size_t)d * n + tri[3 * t]], b = vsoa[(size_t)d * n + tri[3 * t + 1]], c = vsoa[(size_t)d * n + tri[3 * t + 2]];
            fin = fin && std::isfinite(a) && std::isfinite(b) && std::isfinite(c);
            bl[d] = std::min(a, std::min(b, c));
            bh[d] = std::max(a, std::max(b, c));
        }
        if (!fin) continue;  // a triangle with a non-finite corner is never the closest one (its distance is NaN)
        good[(size_t)t] = 1;
        ++ngood;
        double ext = 0.0;
        for (int d = 0; d < 3; ++d) {
            tb[(size_t)6 * t + d] = bl[d];
            tb[(size_t)6 * t + 3 + d] = bh[d];
            lo[d] = std::min(lo[d], bl[d]);
            hi[d] = std::max(hi[d], bh[d]);
            ext = std::max(ext, bh[d] - bl[d]);
        }
        ext_sum += ext;
    }
    if (ngood == 0) return;
    double size[3], maxext = 0.0;
    for (int d = 0; d < 3; ++d) size[d] = hi[d] - lo[d], maxext = std::max(maxext, size[d]);
    if (!(maxext > 0.0) || !(maxext < 1e300)) return;
    // cell edge = the mean extent of a triangle's box
    double &h = p->h = ext_sum / (double)ngood;
    if (!(h > 1e-9 * maxext)) h = 1e-9 * maxext;
    int32_t *gd = p->g, *E = p->span;
    for (;;) {
        double cells = 1.0;
        for (int d = 0; d < 3; ++d) {
            const double c = std::floor(size[d] / h) + 1.0;
            gd[d] = (int32_t)std::min(c, 512.0);
            cells *= std::min(c, 1e9);
            if (c > 512.0) cells = 1e30;
        }
        if (cells <= std::min(16.0 * (double)T + 4096.0, 134217728.0)) break;
        h *= 1.25;
    }
    const double inv_h = p->inv_h = 1.0 / h;
    const int64_t ncells = (int64_t)gd[0] * gd[1] * gd[2];
    // Every triangle is listed ONCE, in the cell of its box's lower corner; a query then looks at the cells [c0 - E, c1] per axis,
    // E = the largest extent (in cells) of a listed triangle's box -- any triangle whose box reaches into the ball [c0, c1] has its
    // lower corner there.  Triangles spanning more than kTriGridMaxSpan cells of an axis go to a short list every query tests.
    std::vector<int32_t> &start = p->start, &list = p->list, hcell((size_t)T, -1), big;
    start.assign((size_t)ncells + 1, 0);
    for (int64_t t = 0; t < T; ++t) {
        if (!good[(size_t)t]) continue;
        int32_t a[3], ex[3];
        bool wide = false;
        for (int d = 0; d < 3; ++d) {
            a[d] = grid_cell_of(tb[(size_t)6 * t + d], lo[d], inv_h, gd[d]);
            ex[d] = grid_cell_of(tb[(size_t)6 * t + 3 + d], lo[d], inv_h, gd[d]) - a[d];
            wide = wide || ex[d] > kTriGridMaxSpan;
        }
        if (wide) {
            big.push_back((int32_t)t);
            continue;
        }
        for (int d = 0; d < 3; ++d) E[d] = std::max(E[d], ex[d]);
        hcell[(size_t)t] = (int32_t)(((int64_t)a[2] * gd[1] + a[1]) * gd[0] + a[0]);
        start[(size_t)hcell[(size_t)t] + 1]++;
    }
    if (big.size() > (size_t)kTriGridMaxBig) return;  // many huge triangles in a fine grid: keep the tile scan
    for (int64_t c = 0; c < ncells; ++c) start[(size_t)c + 1] += start[(size_t)c];
    const int64_t n_listed = start[(size_t)ncells], total = n_listed + (int64_t)big.size();
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    list.resize((size_t)(total > 0 ? total : 1));
    for (int64_t t = 0; t < T; ++t)  // ascending triangle position inside a cell
        if (hcell[(size_t)t] >= 0) list[(size_t)fill[(size_t)hcell[(size_t)t]]++] = (int32_t)t;
    for (size_t k = 0; k < big.size(); ++k) list[(size_t)n_listed + k] = big[k];
    // per ENTRY, contiguous in cell order: the box (48 bytes, all the first test reads) and, apart from it, corners + {device position |
    // original index} (80 bytes, read for the survivors).  The mesh is fixed (the target), so nothing is chased through vertex ids.
    std::vector<double> &boxes = p->boxes, &recs = p->recs;
    boxes.assign(list.size() * (size_t)6, 0.0), recs.assign(list.size() * (size_t)kTriRec, 0.0);
    for (size_t e2 = 0; e2 < (size_t)total; ++e2) {
        const int64_t t = list[e2];
        for (int d = 0; d < 6; ++d) boxes[e2 * 6 + d] = tb[(size_t)6 * t + d];
        double *rc = recs.data() + e2 * kTriRec;
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) rc[3 * c + d] = vsoa[(size_t)d * n + tri[3 * t + c]];
        const long long meta = (long long)(((unsigned long long)(uint32_t)(tri_orig ? tri_orig[t] : (int32_t)t) << 32) | (unsigned long long)(uint32_t)t);
        memcpy(rc + 9, &meta, sizeof(meta));
    }
    p->n_listed = n_listed;
    p->n_big = (int64_t)big.size();
    p->ready = true;
}
