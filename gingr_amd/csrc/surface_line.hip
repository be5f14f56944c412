// The along-normal flavour of the surface ICP: nearest intersection of a line through every fit vertex with a mesh, tile scan and grid.
#include "surface_device.h"

namespace {

constexpr int kSurfThreads = 64;

// ClosestPointAlongNormalTriangleMesh3D (ClosestPointRegistrator.scala:102-131): for every fit vertex the intersection of the
// line {p + t n} (n = its vertex normal, both directions) with the mesh (v, tri) that is closest to p and != p; found[i] = 0 and
// cp = p when there is none.  A 256-triangle tile is visited only if some lane's line passes through its (slightly inflated) box and
// the box is not farther from p than the lane's current hit; then the same test on its four 64-triangle quarters (boxes behind the
// tile boxes: tri_tile_bbox_kernel), and only a quarter some lane needs is staged.  Exact ties go to the lowest ORIGINAL triangle.
// Round 6 (1 067 -> see DESIGN.md at 41k x 82k, where it was 85 % of an iteration of this ICP flavour): the slab test multiplies by
// the line's reciprocal direction (six float64 divisions per box before), quarters instead of whole tiles, and a triangle whose
// barycentric numerators are clearly outside [0, det] is dropped before the division of the Moeller-Trumbore test -- the survivors go
// through the same expressions as before.
struct LineSlab {
    double p[3], inv[3];
    bool par[3];  // direction component exactly zero
    __device__ __forceinline__ bool hits(const double *bx) const {
        double tmin = -__builtin_huge_val(), tmax = __builtin_huge_val();
        bool miss = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double eps = 1e-9 * (fabs(bx[d]) + fabs(bx[3 + d]) + fabs(p[d]) + 1e-300);
            const double lo = bx[d] - eps, hi = bx[3 + d] + eps;
            if (par[d]) {
                if (p[d] < lo || p[d] > hi) miss = true;
            } else {
                const double t1 = (lo - p[d]) * inv[d], t2 = (hi - p[d]) * inv[d];
                tmin = fmax(tmin, fmin(t1, t2));
                tmax = fmin(tmax, fmax(t1, t2));
            }
        }
        return !(miss || tmin > tmax);
    }
};

constexpr int kLineGroup = 16;       // tiles per group box
#ifndef GINGR_LINE_COPIES
#define GINGR_LINE_COPIES 4
#endif
constexpr int kLineCopies = GINGR_LINE_COPIES;  // lanes per query: they take alternate triangles of a staged quarter and alternate group boxes
constexpr int kLineQueries = kSurfThreads / kLineCopies;

// boxes of the groups of 16 tiles (the triangle order is a k-d order: aligned runs are compact), behind the tile and quarter boxes
__global__ __launch_bounds__(64) void line_group_boxes_kernel(double *__restrict__ boxes, int nt) {
    const int idx = blockIdx.x * 64 + threadIdx.x, g = idx / 6, d = idx - 6 * g;
    if (g >= (nt + kLineGroup - 1) / kLineGroup) return;
    double vals[kLineGroup];
#pragma unroll
    for (int u = 0; u < kLineGroup; ++u) {
        const int t = min(g * kLineGroup + u, nt - 1);
        vals[u] = boxes[(int64_t)t * 6 + d];
    }
    double r = vals[0];
#pragma unroll
    for (int u = 1; u < kLineGroup; ++u) r = d < 3 ? fmin(r, vals[u]) : fmax(r, vals[u]);
    boxes[(int64_t)nt * 30 + (int64_t)g * 6 + d] = r;
}

// Four lanes per query (16 queries a wave): the union of the quarters the lines of a wave pierce is smaller, a staged quarter costs 16
// steps instead of 64, and there are four times the waves to hide each other's staging latency (one wave per SIMD otherwise).
__global__ __launch_bounds__(kSurfThreads) void line_nearest_kernel(Cloud fit, const double *__restrict__ dirs, Cloud v,
                                                                   const int32_t *__restrict__ tri,
                                                                   const int32_t *__restrict__ tri_orig, int64_t T,
                                                                   const double *__restrict__ boxes, double *__restrict__ cp,
                                                                   int32_t *__restrict__ found) {
    __shared__ Tri9 quarter[64];
    const int lane = threadIdx.x, copy = lane & (kLineCopies - 1);
    const int64_t i = (int64_t)blockIdx.x * kLineQueries + lane / kLineCopies;
    const bool ok = i < fit.n;
    const int64_t ic = ok ? i : 0;
    const V3 p{fit.x[ic], fit.y[ic], fit.z[ic]};
    const V3 dir{dirs[ic], dirs[fit.n + ic], dirs[2 * fit.n + ic]};
    LineSlab line;
    line.p[0] = p.x, line.p[1] = p.y, line.p[2] = p.z;
    {
        const double da[3] = {dir.x, dir.y, dir.z};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            line.par[d] = da[d] == 0.0;
            line.inv[d] = line.par[d] ? 0.0 : 1.0 / da[d];
        }
    }
    const int nt = (int)((T + kTriTile - 1) / kTriTile);
    const double *qboxes = boxes + (int64_t)nt * 6;
    const double *gboxes = boxes + (int64_t)nt * 30;  // line_group_boxes_kernel
    // Sweeps over shells round the workgroup's own points, the radius doubling: tiles come roughly nearest first, so a line's hit in
    // one shell culls (by distance) what it pierces in the later ones -- the far side of a closed mesh, the fat boxes of slanted
    // patches.  A tile belongs to the shell its box's gap from the points' centre falls into; the sweeps end when every line has a hit
    // nearer than the shell reached, or the farthest box corner is inside it.
    const int ngroups = (nt + kLineGroup - 1) / kLineGroup;
    const Box wb = wave_box(ok, p.x, p.y, p.z);
    const double cx = 0.5 * (wb.lo[0] + wb.hi[0]), cy = 0.5 * (wb.lo[1] + wb.hi[1]), cz = 0.5 * (wb.lo[2] + wb.hi[2]);
    const double ext = sqrt((wb.hi[0] - wb.lo[0]) * (wb.hi[0] - wb.lo[0]) + (wb.hi[1] - wb.lo[1]) * (wb.hi[1] - wb.lo[1]) + (wb.hi[2] - wb.lo[2]) * (wb.hi[2] - wb.lo[2]));
    double gmin2 = __builtin_huge_val(), gfar2 = 0.0;  // nearest gap / farthest corner of the group boxes from the centre
    for (int g = 0; g < ngroups; ++g) {
        const double *gb = gboxes + (int64_t)g * 6;
        gmin2 = fmin(gmin2, point_box_gap2(cx, cy, cz, gb));
        const double fx = fmax(fabs(cx - gb[0]), fabs(cx - gb[3])), fy = fmax(fabs(cy - gb[1]), fabs(cy - gb[4])),
                     fz = fmax(fabs(cz - gb[2]), fabs(cz - gb[5]));
        gfar2 = fmax(gfar2, fx * fx + fy * fy + fz * fz);
    }
    double radius = fmax(fmax(3.0 * ext, 1.5 * sqrt(gmin2)), sqrt(gfar2) * (1.0 / 64.0));
    double inner2 = -1.0;  // tiles with inner2 < gap2 <= radius^2 belong to the sweep
    double best = __builtin_huge_val(), bo = __builtin_huge_val();  // distance |p - ip| and the original triangle that holds it
    V3 bp = p;
    double bound = __builtin_huge_val();  // the smallest `best` of the query's four lanes (culling only)
    for (;;) {
        const double outer2 = radius * radius;
        for (int g0 = 0; g0 < nt; g0 += kLineGroup) {
            const int g = g0 / kLineGroup;
            {
                const double *gb = gboxes + (int64_t)g * 6;
                if (point_box_gap2(cx, cy, cz, gb) > outer2) continue;  // (uniform) the whole group lies in a later shell
                // one of the query's four lanes tests the group (the wave only needs the union)
                const bool need_group = ok && (g & (kLineCopies - 1)) == copy && line.hits(gb) &&
                                        !(point_box_gap2(p.x, p.y, p.z, gb) > bound * bound * (1.0 + 1e-12));
                if (!__any(need_group)) continue;
            }
            // the query's four lanes share the box tests of the group's 16 tiles (four each) and of a tile's four quarters (one each);
            // two shuffles give every lane the query's whole mask
            unsigned tmask = 0;
#pragma unroll
            for (int u = 0; u < (kLineGroup + kLineCopies - 1) / kLineCopies; ++u) {
                const int k = kLineCopies * u + copy, t = g0 + k;
                if (k < kLineGroup && t < nt) {
                    const double *bx = boxes + (int64_t)t * 6;
                    const double cg2 = point_box_gap2(cx, cy, cz, bx);
                    if (cg2 > inner2 && cg2 <= outer2 && ok && line.hits(bx) &&
                        !(point_box_gap2(p.x, p.y, p.z, bx) > bound * bound * (1.0 + 1e-12)))
                        tmask |= 1u << k;
                }
            }
#pragma unroll
            for (int off = 1; off < kLineCopies; off <<= 1) tmask |= __shfl_xor(tmask, off);
            for (int k = 0; k < kLineGroup && g0 + k < nt; ++k) {
                if (!__any((tmask >> k) & 1u)) continue;
                const int t = g0 + k;
                const bool need_tile = (tmask >> k) & 1u;
                unsigned qmask = 0;
#pragma unroll
                for (int u = 0; u < (kTriTile / 64 + kLineCopies - 1) / kLineCopies; ++u) {
                    const int q = kLineCopies * u + copy;
                    if (q < kTriTile / 64) {
                        const int64_t q0 = (int64_t)t * kTriTile + 64 * q;
                        const double *qb = qboxes + ((int64_t)t * 4 + q) * 6;
                        if (q0 < T && need_tile && line.hits(qb) && !(point_box_gap2(p.x, p.y, p.z, qb) > bound * bound * (1.0 + 1e-12)))
                            qmask |= 1u << q;
                    }
                }
#pragma unroll
                for (int off = 1; off < kLineCopies; off <<= 1) qmask |= __shfl_xor(qmask, off);
                for (int q = 0; q < kTriTile / 64; ++q) {
                    if (!__any((qmask >> q) & 1u)) continue;
                    const int64_t q0 = (int64_t)t * kTriTile + 64 * q;
                    // (the bound may have dropped since the mask was made)
                    const bool need = ((qmask >> q) & 1u) &&
                                      !(point_box_gap2(p.x, p.y, p.z, qboxes + ((int64_t)t * 4 + q) * 6) > bound * bound * (1.0 + 1e-12));
                    __syncthreads();
                    if (q0 + lane < T) {
                        const int64_t tq = q0 + lane;
                        const int32_t a = tri[3 * tq], b = tri[3 * tq + 1], c = tri[3 * tq + 2];
                        quarter[lane] = Tri9{v.x[a], v.y[a], v.z[a], v.x[b], v.y[b], v.z[b], v.x[c], v.y[c], v.z[c],
                                             (double)(tri_orig ? tri_orig[tq] : (int32_t)tq)};
                    }
                    __syncthreads();
                    const int cnt = (int)min((int64_t)64, T - q0);
                    if (need)
                        for (int jj = copy; jj < cnt; jj += kLineCopies) {
                            const Tri9 tr = quarter[jj];
                            line_hits_triangle<true>(p, dir, V3{tr.ax, tr.ay, tr.az}, V3{tr.bx, tr.by, tr.bz}, V3{tr.cx, tr.cy, tr.cz}, [&](V3 ip) {
                                const V3 dd = sub(ip, p);
                                const double dist = sqrt((dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z);
                                if (dist < best || (dist == best && tr.orig < bo)) {
                                    best = dist;
                                    bo = tr.orig;
                                    bp = ip;
                                }
                            });
                        }
                    bound = best;
#pragma unroll
                    for (int off = 1; off < kLineCopies; off <<= 1) bound = fmin(bound, __shfl_xor(bound, off));
                }
            }
        }
        if (outer2 >= gfar2) break;                                    // every tile has been in a shell
        if (__all(!ok || bound <= radius - ext)) break;                // what is left is farther than every line's hit
        inner2 = outer2;
        radius *= 2.0;
    }
    // the best of the four lanes: smallest distance, exact ties to the lowest original triangle
#pragma unroll
    for (int off = 1; off < kLineCopies; off <<= 1) take_better(best, bo, bp, off);
    if (ok && copy == 0) {
        cp[i] = bp.x;
        cp[fit.n + i] = bp.y;
        cp[2 * fit.n + i] = bp.z;
        found[i] = best < __builtin_huge_val() ? 1 : 0;
    }
}

// The same search over the target's triangle GRID (TriGridDev: a triangle is listed in the cell of its box's lower corner, its box
// reaches at most span[d] cells further; wide triangles sit in a short list): four lanes per line walk the listing slabs along the
// line's dominant axis outward from the vertex, nearest first.  A triangle listed in slab j can meet the line only over the axis
// interval [j, j + 1 + span] h, so the slab's share of the line -- clipped to the distance of the best hit so far -- bounds the cells of
// the other two axes; the lanes take those cells in turn and run the Moeller-Trumbore test (same expressions and early-outs as
// line_nearest_kernel) on their entries.  A direction is finished once the slab's nearest point of the line is farther than the best
// hit.  Every triangle whose box the line can reach within that distance is seen, so the result is the tile scan's, bit for bit
// (nearest intersection, exact ties to the lowest original triangle).
template <int kLanes>
__global__ __launch_bounds__(256) void line_grid_kernel(Cloud fit, const double *__restrict__ dirs, TriGridDev g, double *__restrict__ cp,
                                                        int32_t *__restrict__ found) {
    constexpr int QPB = 256 / kLanes;
    const int ql = threadIdx.x % kLanes, qi = threadIdx.x / kLanes;
    const int64_t i = (int64_t)blockIdx.x * QPB + qi;
    const bool ok = i < fit.n;
    const int64_t ic = ok ? i : 0;
    const V3 p{fit.x[ic], fit.y[ic], fit.z[ic]};
    const V3 dir{dirs[ic], dirs[fit.n + ic], dirs[2 * fit.n + ic]};
    const double pa[3] = {p.x, p.y, p.z}, da[3] = {dir.x, dir.y, dir.z};
    double best = __builtin_huge_val();
    unsigned bo = 0xFFFFFFFFu;
    V3 bp = p;
    auto test_entry = [&](int64_t e) {
        const double *rc = g.recs + e * kTriRec;
        line_hits_triangle<true>(p, dir, V3{rc[0], rc[1], rc[2]}, V3{rc[3], rc[4], rc[5]}, V3{rc[6], rc[7], rc[8]}, [&](V3 ip) {
            const V3 dd = sub(ip, p);
            const double dist = sqrt((dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z);
            const unsigned o = (unsigned)((unsigned long long)__builtin_bit_cast(long long, rc[9]) >> 32);
            if (dist < best || (dist == best && o < bo)) {
                best = dist;
                bo = o;
                bp = ip;
            }
        });
    };
    // dominant axis (the same in the kLanes lanes of a line)
    int a = 0;
    if (fabs(da[1]) > fabs(da[a])) a = 1;
    if (fabs(da[2]) > fabs(da[a])) a = 2;
    const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    const double len = sqrt((da[0] * da[0] + da[1] * da[1]) + da[2] * da[2]);
    const bool walk = ok && fabs(da[a]) > 0.0 && len < 1.7976931348623157e308 && pa[0] == pa[0] && pa[1] == pa[1] && pa[2] == pa[2];
    if (walk) {
        for (int64_t e = g.n_listed + ql; e < (int64_t)g.n_listed + g.n_big; e += kLanes) test_entry(e);  // the wide triangles
    }
    double bound = best;
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) bound = fmin(bound, __shfl_xor(bound, off));
    if (walk) {
        const double inv_da = 1.0 / da[a], unit = len / fabs(da[a]);  // distance along the line per unit of the dominant axis
        const int ga = g.g[a];
        const int j0 = grid_cell_of(pa[a], g.lo[a], g.inv_h, ga);  // the vertex's slab
        const double hs = g.h * (double)(1 + g.span[a]);
        bool live[2] = {true, true};
        for (int k = 0; live[0] || live[1]; ++k) {
            for (int sgn = 0; sgn < 2; ++sgn) {
                if (!live[sgn] || (k == 0 && sgn == 1)) continue;
                const int j = sgn == 0 ? j0 + k : j0 - k;
                if (j < 0 || j >= ga) {
                    live[sgn] = false;
                    continue;
                }
                // the axis interval a triangle listed in slab j can occupy, slightly widened
                const double epsa = 1e-9 * (fabs(pa[a]) + fabs(g.lo[a]) + hs * (double)(j + 1)) + 1e-300;
                const double A0 = g.lo[a] + g.h * (double)j - epsa, A1 = g.lo[a] + g.h * (double)j + hs + epsa;
                const double gap = fmax(fmax(A0 - pa[a], pa[a] - A1), 0.0);
                if (gap * unit > bound * (1.0 + 1e-9)) {  // (monotone in k: this direction is done)
                    live[sgn] = false;
                    continue;
                }
                double t0 = (A0 - pa[a]) * inv_da, t1 = (A1 - pa[a]) * inv_da;
                if (t0 > t1) {
                    const double tmp = t0;
                    t0 = t1;
                    t1 = tmp;
                }
                if (bound < __builtin_huge_val()) {  // nothing farther than the best hit matters
                    const double tl = bound / len * (1.0 + 1e-9);
                    t0 = fmax(t0, -tl);
                    t1 = fmin(t1, tl);
                }
                if (t0 <= t1) {
                    int lo_c[2], n_c[2];
                    bool any = true;
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const int d = s2 == 0 ? b : c;
                        const double x0 = pa[d] + t0 * da[d], x1 = pa[d] + t1 * da[d];
                        const double eps = 1e-9 * (fabs(x0) + fabs(x1) + fabs(g.lo[d]) + g.h) + 1e-300;
                        const double f0 = (fmin(x0, x1) - eps - g.lo[d]) * g.inv_h, f1 = (fmax(x0, x1) + eps - g.lo[d]) * g.inv_h;
                        const int gd = g.g[d];
                        if (!(f1 >= 0.0) || !(f0 < (double)gd + (double)g.span[d] + 1.0)) any = false;  // (also NaN)
                        const double c0 = floor(f0) - (double)g.span[d], c1 = floor(f1);
                        const int i0 = c0 > 0.0 ? (c0 < (double)gd ? (int)c0 : gd) : 0;
                        const int i1 = c1 < (double)(gd - 1) ? (c1 >= 0.0 ? (int)c1 : -1) : gd - 1;
                        lo_c[s2] = i0;
                        n_c[s2] = i1 - i0 + 1;
                        if (n_c[s2] <= 0) any = false;
                    }
                    if (any && a != 0) {
                        // b is the x axis: the cells of a row are one contiguous run of entries; the lanes take rows
                        for (int r = ql; r < n_c[1]; r += kLanes) {
                            int cell3[3];
                            cell3[a] = j;
                            cell3[b] = lo_c[0];
                            cell3[c] = lo_c[1] + r;
                            const int64_t idx = ((int64_t)cell3[2] * g.g[1] + cell3[1]) * g.g[0] + cell3[0];
                            const int32_t e0 = g.cell_start[idx], e1 = g.cell_start[idx + n_c[0]];
                            for (int32_t e = e0; e < e1; ++e) test_entry(e);
                        }
                    } else if (any) {
                        const int ncell = n_c[0] * n_c[1];
                        for (int r = ql; r < ncell; r += kLanes) {
                            const int rb = r % n_c[0], rc2 = r / n_c[0];
                            const int64_t idx = ((int64_t)(lo_c[1] + rc2) * g.g[1] + (lo_c[0] + rb)) * g.g[0] + j;  // (a = x, b = y, c = z)
                            const int32_t e0 = g.cell_start[idx], e1 = g.cell_start[idx + 1];
                            for (int32_t e = e0; e < e1; ++e) test_entry(e);
                        }
                    }
                }
                bound = best;
#pragma unroll
                for (int off = 1; off < kLanes; off <<= 1) bound = fmin(bound, __shfl_xor(bound, off));
            }
        }
    }
    // the best of the line's lanes: smallest distance, exact ties to the lowest original triangle
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) take_better(best, bo, bp, off);
    if (ok && ql == 0) {
        cp[i] = bp.x;
        cp[fit.n + i] = bp.y;
        cp[2 * fit.n + i] = bp.z;
        found[i] = best < __builtin_huge_val() ? 1 : 0;
    }
}

}  // namespace

void launch_line_nearest(gingr_ctx *ctx, Cloud fit, const double *dirs_soa, Cloud v, const int32_t *tri, const int32_t *tri_orig,
                         int64_t T, double *boxes, double *cp_soa, int32_t *found) {
    const int nt = (int)ceil_div(T, kTriTile);
    hipLaunchKernelGGL(line_group_boxes_kernel, dim3((unsigned)ceil_div((int64_t)6 * ceil_div(nt, kLineGroup), 64)), dim3(64), 0, ctx->stream,
                       boxes, nt);
    hipLaunchKernelGGL(line_nearest_kernel, dim3((unsigned)ceil_div(fit.n, kLineQueries)), dim3(kSurfThreads), 0, ctx->stream, fit,
                       dirs_soa, v, tri, tri_orig, T, boxes, cp_soa, found);
}
#ifndef GINGR_LINE_GRID_LANES
#define GINGR_LINE_GRID_LANES 4  // (measured at 41k x 82k: 1 / 2 / 4 / 8 / 16 / 32 lanes per line: 0.321 / 0.265 / 0.235 / 0.237 / 0.244 / 0.280 ms per iteration)
#endif
void launch_line_nearest_grid(gingr_ctx *ctx, Cloud fit, const double *dirs_soa, const TriGrid &g, double *cp_soa, int32_t *found) {
    constexpr int kLanes = GINGR_LINE_GRID_LANES;
    hipLaunchKernelGGL(line_grid_kernel<kLanes>, dim3((unsigned)ceil_div(fit.n, 256 / kLanes)), dim3(256), 0, ctx->stream, fit, dirs_soa, g.v, cp_soa,
                       found);
}
