// Device helpers of the surface kernels (surface*.hip): small vectors, the point / triangle and line / triangle routines, the point
// to box gap (wave boxes and box to box gaps: box_device.h),
// and the routines more than one kernel runs -- each has ONE body here.  Everything is inlined into its caller; arithmetic is written
// without FMA contraction in the oracle's operation order, so a helper gives the bits its callers' own expressions gave.
#pragma once
#include "box_device.h"
#include "surface.h"

namespace {  // (one private copy per translation unit, like the kernels that use it)

constexpr int kCpThreads = 256;  // threads of a tile-scan workgroup: four waves, one per 64-triangle quarter of a tile

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// closest point of triangle (A, B, C) to p: Ericson, Real-Time Collision Detection 5.1.5, with his region tests in his order but
// evaluated as selects: on a wavefront every lane lands in a different Voronoi region, so the branching form executes all seven
// paths (and their four divisions) one after the other.  Here the region picks a numerator, a denominator, a base corner and two
// edge vectors; ONE division; the result is  base + e1 * s1 + e2 * s2  -- the same floating-point expressions as the branching
// form (an edge region adds  e2 * 0  = +0, a vertex region adds two zeros).
__device__ __forceinline__ V3 closest_on_triangle(V3 p, V3 A, V3 B, V3 C) {
    const V3 ab = sub(B, A), ac = sub(C, A), bc = sub(C, B), ap = sub(p, A), bp = sub(p, B), cp = sub(p, C);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const bool rA = d1 <= 0.0 && d2 <= 0.0;
    const bool rB = !rA && d3 >= 0.0 && d4 <= d3;
    const bool rAB = !rA && !rB && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0;
    const bool rC = !rA && !rB && !rAB && d6 >= 0.0 && d5 <= d6;
    const bool rAC = !rA && !rB && !rAB && !rC && vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0;
    const bool rBC = !rA && !rB && !rAB && !rC && !rAC && va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0;
    const bool vertex = rA || rB || rC;
    const double num = vertex ? 0.0 : (rAB ? d1 : (rAC ? d2 : (rBC ? (d4 - d3) : 1.0)));
    const double den = vertex ? 1.0 : (rAB ? (d1 - d3) : (rAC ? (d2 - d6) : (rBC ? ((d4 - d3) + (d5 - d6)) : ((va + vb) + vc))));
    const double q = num / den;
    const bool interior = !vertex && !rAB && !rAC && !rBC;
    const V3 base = (rB || rBC) ? B : (rC ? C : A);
    const V3 e1 = rBC ? bc : (rAC ? ac : ab);
    const double s1 = vertex ? 0.0 : (interior ? vb * q : q);
    const double s2 = interior ? vc * q : 0.0;
    return V3{(base.x + e1.x * s1) + ac.x * s2, (base.y + e1.y * s1) + ac.y * s2, (base.z + e1.z * s1) + ac.z * s2};
}

// Barycentric weights (of A, B, C) of the closest point of triangle (A, B, C) to p: the region logic of closest_on_triangle with
// the weights spelled out -- vertex regions (1,0,0), edge regions (1-q, q, 0), interior (1 - v - w, v, w).
__device__ __forceinline__ V3 closest_barycentric(V3 p, V3 A, V3 B, V3 C) {
    const V3 ab = sub(B, A), ac = sub(C, A), ap = sub(p, A), bp = sub(p, B), cp = sub(p, C);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) return V3{1.0, 0.0, 0.0};
    if (d3 >= 0.0 && d4 <= d3) return V3{0.0, 1.0, 0.0};
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double q = d1 / (d1 - d3);
        return V3{1.0 - q, q, 0.0};
    }
    if (d6 >= 0.0 && d5 <= d6) return V3{0.0, 0.0, 1.0};
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double q = d2 / (d2 - d6);
        return V3{1.0 - q, 0.0, q};
    }
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double q = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        return V3{0.0, 1.0 - q, q};
    }
    const double q = 1.0 / ((va + vb) + vc);
    const double v = vb * q, w = vc * q;
    return V3{(1.0 - v) - w, v, w};
}

__device__ __forceinline__ double point_box_gap2(double qx, double qy, double qz, const double *__restrict__ bx) {
    const double gx = fmax(fmax(bx[0] - qx, qx - bx[3]), 0.0), gy = fmax(fmax(bx[1] - qy, qy - bx[4]), 0.0),
                 gz = fmax(fmax(bx[2] - qz, qz - bx[5]), 0.0);
    return __builtin_fma(gz, gz, __builtin_fma(gy, gy, gx * gx));
}

struct Tri9 {
    double ax, ay, az, bx, by, bz, cx, cy, cz, orig;
};

struct Corners { V3 A, B, C; };  // of triangle t of the mesh (v, tri)
__device__ __forceinline__ Corners gather_corners(Cloud v, const int32_t *__restrict__ tri, int64_t t) {
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    return Corners{V3{v.x[a], v.y[a], v.z[a]}, V3{v.x[b], v.y[b], v.z[b]}, V3{v.x[c], v.y[c], v.z[c]}};
}

// bb[6] = the box of triangle tt: as tri_tile_bbox_kernel left it in tribox (one contiguous read), or rebuilt from its corners
__device__ __forceinline__ void stage_tri_box(double *bb, int64_t tt, const double *tribox, const int32_t *tri, Cloud v) {
    if (tribox) {
        const double *sb = tribox + 6 * tt;
        bb[0] = sb[0], bb[1] = sb[1], bb[2] = sb[2], bb[3] = sb[3], bb[4] = sb[4], bb[5] = sb[5];
    } else {
        const int32_t a = tri[3 * tt], b = tri[3 * tt + 1], c = tri[3 * tt + 2];
        const double ax = v.x[a], ay = v.y[a], az = v.z[a], bx = v.x[b], by = v.y[b], bz = v.z[b], cx = v.x[c], cy = v.y[c], cz = v.z[c];
        bb[0] = fmin(fmin(ax, bx), cx), bb[1] = fmin(fmin(ay, by), cy), bb[2] = fmin(fmin(az, bz), cz);
        bb[3] = fmax(fmax(ax, bx), cx), bb[4] = fmax(fmax(ay, by), cy), bb[5] = fmax(fmax(az, bz), cz);
    }
}

// Moeller-Trumbore on the infinite line {p + t dir} with inclusive barycentric bounds: hit(ip) runs when the line meets triangle
// (A, B, C) in a point ip != p.  kEarlyOut: a triangle whose barycentric numerators are clearly outside [0, det] is dropped before the
// division; the survivors go through the same expressions.  What "closer" means, and ties, are the caller's.
template <bool kEarlyOut, typename F>
__device__ __forceinline__ void line_hits_triangle(V3 p, V3 dir, V3 A, V3 B, V3 C, F &&hit) {
    const V3 e1 = sub(B, A), e2 = sub(C, A);
    const V3 pv = cross3(dir, e2);
    const double det = dot3(e1, pv);
    const V3 tv = sub(p, A);
    const double nu = dot3(tv, pv);
    const double ad = fabs(det), su = det > 0.0 ? nu : -nu;
    if (kEarlyOut && (su < -1e-9 * ad || su > ad * (1.0 + 1e-9))) return;  // u clearly outside [0, 1]
    const V3 qv = cross3(tv, e1);
    const double nw = dot3(qv, dir);
    const double sw = det > 0.0 ? nw : -nw;
    if (kEarlyOut && (sw < -1e-9 * ad || su + sw > ad * (1.0 + 2e-9))) return;  // w < 0 or u + w > 1, clearly
    const double inv = 1.0 / det;
    const double u = nu * inv;
    const double w = nw * inv;
    const double tt = dot3(e2, qv) * inv;
    if (det != 0.0 && u >= 0.0 && u <= 1.0 && w >= 0.0 && u + w <= 1.0) {
        const V3 ip{p.x + tt * dir.x, p.y + tt * dir.y, p.z + tt * dir.z};
        if (ip.x != p.x || ip.y != p.y || ip.z != p.z) hit(ip);
    }
}

// One lane-merge step of a query's best hit: the candidate of the lane `off` away replaces this lane's when it is nearer; exact ties go
// to the lowest original triangle (Id: unsigned, or a double that holds the number).  True when it was taken.
template <typename Id>
__device__ __forceinline__ bool take_better(double &best, Id &bo, V3 &bp, int off) {
    const double od = __shfl_xor(best, off);
    const Id oo = __shfl_xor(bo, off);
    const double ox = __shfl_xor(bp.x, off), oy = __shfl_xor(bp.y, off), oz = __shfl_xor(bp.z, off);
    if (od < best || (od == best && oo < bo)) {
        best = od;
        bo = oo;
        bp = V3{ox, oy, oz};
        return true;
    }
    return false;
}

// Per-wave queue of (query slot, triangle position) pairs in LDS (128 entries: up to 63 left over + 64 pushed): the survivors of a
// step's box tests are compacted across the wave (ballot + prefix count), and as soon as 64 are queued every lane pops one.
struct WaveQueue {
    unsigned int *q;  // the wave's entries: (query slot << 26) | position of the triangle in `tri`
    int lane;
    int tail;  // queued pairs (wave-uniform)
    // true when 64 pairs are queued: the caller flushes 64
    __device__ __forceinline__ bool push(bool pass, int slot, unsigned pos) {
        const unsigned long long m = __ballot(pass);
        if (!m) return false;
        if (pass) q[tail + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = ((unsigned)slot << 26) | pos;
        tail += __builtin_popcountll(m);
        return tail >= 64;
    }
    // pops up to 64 pairs, one per lane: each(mine, query slot, triangle position) runs in every lane (mine: the lane holds a pair);
    // then the entries beyond `count` move to the front
    template <typename F>
    __device__ __forceinline__ void flush(int count, F &&each) {
        __builtin_amdgcn_wave_barrier();
        const bool mine = lane < count;
        const unsigned e = q[mine ? lane : 0];
        each(mine, (int)(e >> 26), (int64_t)(e & 0x3FFFFFFu));
        if (tail > count) {
            const unsigned rest = lane + count < tail ? q[lane + count] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (lane + count < tail) q[lane] = rest;
        }
        tail -= count;
    }
};

// The cells the ball of radius r round (qx, qy, qz) reaches in the grid g, as entry runs for the query's kLanes lanes (lane ql): every
// listed triangle sits in the cell of its box's lower corner, so the cells [c0 - span, c1] hold all that reach the ball; along x they
// are ONE contiguous run of entries per (y, z) row; the short list of wide triangles is one more run.  cell_s[k] = first entry of
// run k, cell_off[k] = exclusive prefix of the run lengths, total = their sum.  False (nothing written) when a cell coordinate is not
// finite or the ball covers more than kTriGridMaxCells runs.
template <int kLanes>
__device__ __forceinline__ bool grid_ball_runs(const TriGridDev &g, double qx, double qy, double qz, double r, int ql, int32_t *cell_s,
                                               int32_t *cell_off, int32_t &total) {
    const double f0[3] = {(qx - r - g.lo[0]) * g.inv_h, (qy - r - g.lo[1]) * g.inv_h, (qz - r - g.lo[2]) * g.inv_h};
    const double f1[3] = {(qx + r - g.lo[0]) * g.inv_h, (qy + r - g.lo[1]) * g.inv_h, (qz + r - g.lo[2]) * g.inv_h};
    bool fin = true;
    int c0[3], c1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        fin = fin && fabs(f0[d]) < 1e15 && fabs(f1[d]) < 1e15;
        c0[d] = grid_clamp_cell(f0[d], g.g[d]);
        c1[d] = grid_clamp_cell(f1[d], g.g[d]);
    }
    const int x0 = c0[0] > g.span[0] ? c0[0] - g.span[0] : 0, y0 = c0[1] > g.span[1] ? c0[1] - g.span[1] : 0,
              z0 = c0[2] > g.span[2] ? c0[2] - g.span[2] : 0;
    const int ny = c1[1] - y0 + 1, nz = c1[2] - z0 + 1;
    if (!(fin && ny * nz + 1 <= kTriGridMaxCells)) return false;
    const int nrow = ny * nz, nrun = nrow + (g.n_big > 0 ? 1 : 0);
    for (int k = ql; k < nrun; k += kLanes) {  // the entry run of every row, one row per lane
        int32_t s0, n0;
        if (k < nrow) {
            const int rz = k / ny, ry = k - rz * ny;
            const int64_t rowbase = ((int64_t)(z0 + rz) * g.g[1] + (y0 + ry)) * g.g[0];
            s0 = g.cell_start[rowbase + x0];
            n0 = g.cell_start[rowbase + c1[0] + 1] - s0;
        } else {
            s0 = g.n_listed;
            n0 = g.n_big;
        }
        cell_s[k] = s0;
        cell_off[k + 1] = n0;
    }
    __threadfence_block();
    if (ql == 0) {  // exclusive prefix over at most 64 counts
        int32_t off = 0;
        for (int k = 0; k < nrun; ++k) {
            const int32_t n = cell_off[k + 1];
            cell_off[k] = off;
            off += n;
        }
        cell_off[nrun] = off;
    }
    __threadfence_block();
    total = cell_off[nrun];
    return true;
}

// the workgroup's flagged queries (one lane per query passes true): one atomic
__device__ __forceinline__ void count_flagged(bool flagged, int32_t *__restrict__ nflag) {
    const unsigned long long m = __ballot(flagged);
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt, __builtin_popcountll(m));
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(nflag, cnt);
}

}  // namespace
