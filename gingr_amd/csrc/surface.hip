// ICP with the surface correspondence: the reference's DEFAULT ICP method
//     ICPCorrespondence.estimate with TriangularClosestPoint (G/api/registration/config/ICP.scala:36-52,63)
//       -> ClosestPointTriangleMesh3D.closestPointCorrespondence (G/api/registration/utils/ClosestPointRegistrator.scala:75-100)
// For every template (fit) vertex p:  cp = target.operations.closestPointOnSurface(p);  v = the target VERTEX closest to cp;
// weight 0 when v is a boundary vertex (:53-55), when the vertex normals of p and v point into opposite half spaces (:57-60),
// or when the line through p along p - cp meets the template itself closer than |p - cp| (:62-72); else 1.  Only weight-1
// pairs become observations (ICP.scala:50).
//
// scalismo's mesh queries are restated (oracle/gingr_oracle.py, section f2): exact point-triangle closest point (Ericson
// 5.1.5), vertex normal = mean of the adjacent unit cell normals, boundary vertex = on an edge with one adjacent triangle,
// line-triangle intersection = Moeller-Trumbore on the infinite line with inclusive barycentric bounds (UNPINNED: scalismo's
// own intersection routine is not available; with this formulation a triangle that has p as a corner returns exactly p,
// which the reference filters out).  Arithmetic is written without FMA contraction in the oracle's operation order.
//
// Triangles live in a spatial (k-d leaf) order with one bounding box per 256-triangle tile; a wave owns 64 spatially
// coherent queries and skips every tile whose box cannot hold anything closer than what each lane already has -- the same
// exact pruning as the nearest-neighbour kernel (nn_scan.hip).
#include "surface_device.h"

namespace {

// cp (SoA [3][nq]) / d2: closest point of the triangle soup to every query; exact ties go to the lowest ORIGINAL triangle.
// A workgroup of four waves serves 64 queries: every wave holds the same queries and scans ONE 64-triangle quarter of each
// staged tile, visited only if that quarter's box is not farther from a lane's query than the lane's best so far.  Sweep 0
// takes the tiles nearest to the queries' bounding box, then the four waves share their best distances (the bound only), and
// sweep 1 takes the remaining tiles under that bound.  Four times the parallelism of one wave per 64 queries, and the pruning
// works on quarters instead of tiles.

// H copies of every query per workgroup: 64 / H queries, each held by H lanes that take alternate triangles of the quarter.  Same
// arithmetic per (query, triangle) pair, a shorter scan per workgroup and more workgroups: the kernel is bound by its longest
// workgroups, not by the vector ALU.
// The exact closest-point test (~170 instructions) is not run where the box test passes: a step's 64 (query, triangle) pairs
// survive their box tests at a rate of 1.2 % (41k queries x 82k triangles), so running it for the whole wave whenever ANY pair
// survives wastes 98 % of the lanes (the first version of this kernel did; 232 us against 147 us).  Instead the
// survivors of the box tests are COMPACTED across the wave: every lane appends its surviving pair to a per-wave LDS queue (ballot
// + prefix count), and as soon as 64 pairs are queued every lane pops one and runs the exact test on ITS pair -- a different
// query and a different triangle in every lane.  The result goes to the owning query through LDS: an atomic minimum on the
// squared distance (non-negative doubles order like their bit patterns), then an atomic minimum on the original triangle number
// among the lanes that hold that minimum (the tie rule), then the winner stores its point.  All copies of a query prune against
// the shared best after every flush.  The queue is drained before the tile in LDS is replaced.
template <int H>
__global__ __launch_bounds__(kCpThreads) void surface_cp_queue_kernel(Cloud q, Cloud v, const int32_t *__restrict__ tri,
                                                                     const int32_t *__restrict__ tri_orig, int64_t T,
                                                                     const double *__restrict__ boxes, double *__restrict__ cp,
                                                                     double *__restrict__ d2out, int32_t *__restrict__ tri_out,
                                                                     const int32_t *warm_in, int32_t *pos_out /* may alias warm_in */,
                                                                     const double *__restrict__ tribox,
                                                                     const uint8_t *__restrict__ mask, const int32_t *__restrict__ nmask) {
    // mask / nmask (nullable): only the queries with mask[i] != 0 are answered -- what the triangle-grid search in front of this
    // launch could not certify (surface_cp_grid_kernel) -- and the whole launch is a no-op when *nmask == 0
    if (nmask && *nmask == 0) return;
    __shared__ double tbox[kTriTile][6];  // staged tile: the triangles' bounding boxes only (the exact test reads memory)
    constexpr int QPB = 64 / H;  // queries per workgroup
    __shared__ unsigned long long qbest[4][QPB];  // per wave and query: bits of the best squared distance so far
    __shared__ unsigned int qorig[4][QPB];        // ... its original triangle (lowest on ties)
    __shared__ double qpt[4][3][QPB];             // ... its point
    __shared__ int qpos[4][QPB];                  // ... its position in `tri` (the next call's warm start)
    __shared__ double sq[3][QPB];                 // the queries
    __shared__ unsigned int wqueue[4][128];  // (query slot << 26) | position of the triangle in `tri`
    __shared__ double sbound[4][QPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ql = lane & (QPB - 1), half = lane / QPB;
    const int64_t i = (int64_t)blockIdx.x * QPB + ql;
    const bool ok = i < q.n && (!mask || mask[i] != 0);
    if (mask && !__syncthreads_or(ok)) return;  // nothing flagged in this workgroup
    const double qx = ok ? q.x[i] : 0.0, qy = ok ? q.y[i] : 0.0, qz = ok ? q.z[i] : 0.0;
    const unsigned long long kInfBits = 0x7FF0000000000000ull;
    // Warm start (nullable): the triangle (position in `tri`) that was closest to this query LAST time -- a template vertex moves
    // little between two ICP iterations.  Its exact distance is a valid candidate: the bound is tight before the first tile instead
    // of after the first 64 evaluated pairs of every wave.  Same minimum, same tie rule (an equally close triangle lies in a tile
    // whose gap does not exceed the bound, so it is still evaluated and wins on the lower original id).
    unsigned long long wbits = kInfBits;
    unsigned worig = 0xFFFFFFFFu;
    int wpos = -1;
    V3 wpt{qx, qy, qz};
    if (warm_in && ok) {
        const int32_t tg = warm_in[i];
        if (tg >= 0 && tg < T) {
            const Corners w = gather_corners(v, tri, tg);
            const V3 pq{qx, qy, qz};
            const V3 c = closest_on_triangle(pq, w.A, w.B, w.C);
            const V3 dd = sub(c, pq);
            const double dist = (dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z;
            if (dist == dist) {  // NaN: cold start
                wbits = __builtin_bit_cast(unsigned long long, dist);
                worig = (unsigned)(tri_orig ? tri_orig[tg] : tg);
                wpos = tg;
                wpt = c;
            }
        }
    }
    if (half == 0) {
        qbest[wave][ql] = wbits;
        qorig[wave][ql] = worig;
        qpos[wave][ql] = wpos;
        qpt[wave][0][ql] = wpt.x, qpt[wave][1][ql] = wpt.y, qpt[wave][2][ql] = wpt.z;
        if (wave == 0) sq[0][ql] = qx, sq[1][ql] = qy, sq[2][ql] = qz;
    }
    __syncthreads();
    double best = __builtin_bit_cast(double, wbits), bound = __builtin_huge_val();
    WaveQueue wq{wqueue[wave], lane, 0};
    const Box wb = wave_box(ok, qx, qy, qz);
    const int nt = (int)((T + kTriTile - 1) / kTriTile);
    const double *qboxes = boxes + (int64_t)nt * 6;
    // what every lane does with the pair it pops (WaveQueue::flush)
    auto each = [&](bool mine, int tq, int64_t tg) {
        const V3 pp{sq[0][tq], sq[1][tq], sq[2][tq]};
        Tri9 tr;  // the queue outlives the staged tile: the triangle comes from memory (L2: it was staged a moment ago)
        {
            const int32_t va = tri[3 * tg], vb = tri[3 * tg + 1], vc = tri[3 * tg + 2];
            tr = Tri9{v.x[va], v.y[va], v.z[va], v.x[vb], v.y[vb], v.z[vb], v.x[vc], v.y[vc], v.z[vc],
                      (double)(tri_orig ? tri_orig[tg] : (int32_t)tg)};
        }
        const V3 c = closest_on_triangle(pp, V3{tr.ax, tr.ay, tr.az}, V3{tr.bx, tr.by, tr.bz}, V3{tr.cx, tr.cy, tr.cz});
        const V3 dd = sub(c, pp);
        const double dist = (dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z;
        const unsigned long long db = __builtin_bit_cast(unsigned long long, dist);
        const unsigned long long old = qbest[wave][tq];
        if (mine && db <= old) atomicMin(&qbest[wave][tq], db);
        __builtin_amdgcn_wave_barrier();
        const unsigned long long now = qbest[wave][tq];
        const bool top = mine && db == now;
        if (top && now < old) qorig[wave][tq] = 0xFFFFFFFFu;  // a strictly better distance: the old triangle no longer competes
        __builtin_amdgcn_wave_barrier();
        if (top) atomicMin(&qorig[wave][tq], (unsigned)tr.orig);
        __builtin_amdgcn_wave_barrier();
        if (top && qorig[wave][tq] == (unsigned)tr.orig) {
            qpt[wave][0][tq] = c.x, qpt[wave][1][tq] = c.y, qpt[wave][2][tq] = c.z;
            qpos[wave][tq] = (int)tg;
        }
        __builtin_amdgcn_wave_barrier();
        best = __builtin_bit_cast(double, qbest[wave][ql]);  // every copy of the query prunes against the shared best
    };
    double gmin = __builtin_huge_val();
    for (int t = lane; t < nt; t += 64) gmin = fmin(gmin, box_gap2(wb, boxes + (int64_t)t * 6));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gmin = fmin(gmin, __shfl_xor(gmin, off));
    gmin = uniform_d(gmin);
    for (int phase = 0; phase < 2; ++phase) {
        double bmax = ok ? bound : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, off));
        bmax = uniform_d(bmax) * (1.0 + 1e-12);
        for (int tc = 0; tc < nt; tc += 64) {
            const int tl = tc + lane;
            const double g = tl < nt ? box_gap2(wb, boxes + (int64_t)tl * 6) : __builtin_huge_val();
            unsigned long long cand = __ballot(tl < nt && (phase == 0 ? !(g > gmin) : (g > gmin && !(g > bmax))));
            while (cand) {  // workgroup-uniform (same queries, same bound in every wave)
                const int t = tc + __builtin_ctzll(cand);
                cand &= cand - 1;
                const int64_t tb = (int64_t)t * kTriTile, q0 = tb + 64 * wave;
                const double pd = point_box_gap2(qx, qy, qz, qboxes + ((int64_t)t * 4 + wave) * 6);
                const bool need = ok && q0 < T && !(pd > fmin(best, bound) * (1.0 + 1e-12));
                const bool wave_needs = __any(need);
                if (!__syncthreads_or(wave_needs)) continue;
                {
                    const int64_t tt = tb + threadIdx.x;
                    if (tt < T) stage_tri_box(tbox[threadIdx.x], tt, tribox, tri, v);
                }
                __syncthreads();
                if (wave_needs) {
                    const int cnt = (int)min((int64_t)64, T - q0);
                    for (int j0 = 0; j0 < cnt; j0 += H) {
                        const int jj = j0 + half;
                        const bool live = jj < cnt;
                        const double gap = point_box_gap2(qx, qy, qz, tbox[64 * wave + (live ? jj : cnt - 1)]);
                        const bool pass = need && live && !(gap > fmin(best, bound) * (1.0 + 1e-12));
                        if (wq.push(pass, ql, (unsigned)(q0 + jj))) wq.flush(64, each);
                    }
                }
                __syncthreads();
            }
        }
        if (wq.tail > 0) wq.flush(wq.tail, each);  // drain: the sweep's results feed the bound / the answer
        if (phase == 0) {  // share the distance bound of sweep 0 between the waves
            if (half == 0) sbound[wave][ql] = __builtin_bit_cast(double, qbest[wave][ql]);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) bound = fmin(bound, sbound[k][ql]);
            __syncthreads();
        }
    }
    __syncthreads();
    if (wave == 0 && half == 0 && ok) {  // combine the four waves: smallest distance, ties -> lowest original triangle
        int w = 0;
        for (int k = 1; k < 4; ++k)
            if (qbest[k][ql] < qbest[w][ql] || (qbest[k][ql] == qbest[w][ql] && qorig[k][ql] < qorig[w][ql])) w = k;
        cp[i] = qpt[w][0][ql];
        cp[q.n + i] = qpt[w][1][ql];
        cp[2 * q.n + i] = qpt[w][2][ql];
        d2out[i] = __builtin_bit_cast(double, qbest[w][ql]);
        if (tri_out) tri_out[i] = (int32_t)qorig[w][ql];
        if (pos_out) pos_out[i] = qpos[w][ql];
    }
}

// ---- closest surface point over a uniform grid of the (fixed) target triangles (round 4) -------------------------------------------
// The target mesh of a registration does not move, so gingr_fitter_set_meshes bins its triangles once: cell c lists (positions in
// `tri` of) the triangles whose bounding box overlaps it.  A query starts from the triangle that was closest to it in the previous
// scan (warm start; a template vertex moves little between two iterations): its exact distance r bounds the answer, and every
// triangle that holds a point within r of the query has a bounding box that overlaps a cell the ball of radius r overlaps -- the
// cell of that point -- so scanning the triangle lists of the cells [cell(q - r), cell(q + r)] (a slack of 1e-9 r covers the
// rounding of the cell index; host and device evaluate the same floor((x - lo) * inv_h), which is monotone in x) finds the exact
// minimum and, by the (distance, original triangle id) order, the same winner on ties as the tile scan.  Same point-triangle routine,
// same separately rounded distance: bit-identical closest points.  A query whose ball covers more than kTriGridMaxCells cells (far
// from the surface, the early iterations), a cold start, or a non-finite query is FLAGGED and answered by the masked tile scan
// (surface_cp_queue_kernel) that follows.  kLanes lanes per query take the cells of the block in turn; a triangle listed in several
// cells is evaluated more than once with the same result.
#ifndef GINGR_TRI_GRID_LANES
#define GINGR_TRI_GRID_LANES 16
#endif
constexpr int kTriGridCand = 96;  // candidates (entries that pass the box test and the home-cell rule) kept per query; more: the tile scan

template <int kLanes>
__global__ __launch_bounds__(256) void surface_cp_grid_kernel(Cloud q, Cloud v, const int32_t *__restrict__ tri,
                                                             const int32_t *__restrict__ tri_orig, int64_t T, TriGridDev g,
                                                             double *__restrict__ cp, double *__restrict__ d2out,
                                                             int32_t *__restrict__ tri_out,
                                                             int32_t *warm /* in: last closest triangle, out: this one's */,
                                                             uint8_t *__restrict__ flag, int32_t *__restrict__ nflag,
                                                             int32_t *__restrict__ nflag_next) {
    static_assert(kLanes == 32 || kLanes == 16 || kLanes == 8, "sub-wave ballots below");
    constexpr int QPB = 256 / kLanes;
    __shared__ int32_t cell_s[QPB][kTriGridMaxCells], cell_off[QPB][kTriGridMaxCells + 1];
    __shared__ int32_t cand[QPB][kTriGridCand];
    if (blockIdx.x == 0 && threadIdx.x == 0) *nflag_next = 0;  // the counter of the NEXT search (nobody reads it during this one)
    const int ql = threadIdx.x % kLanes, qi = threadIdx.x / kLanes, wslot = (threadIdx.x & 63) / kLanes;  // wslot: the query's slot in its wave
    const int64_t i = (int64_t)blockIdx.x * QPB + qi;
    const bool ok = i < q.n;
    const double qx = ok ? q.x[i] : 0.0, qy = ok ? q.y[i] : 0.0, qz = ok ? q.z[i] : 0.0;
    const V3 p{qx, qy, qz};
    double best = __builtin_huge_val();
    unsigned bo = 0xFFFFFFFFu;
    int bpos = -1;
    V3 bp{qx, qy, qz};
    auto consider = [&](V3 A, V3 B, V3 C, int pos, unsigned o) {
        const V3 c = closest_on_triangle(p, A, B, C);
        const V3 dd = sub(c, p);
        const double dist = (dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z;
        if (dist < best || (dist == best && o < bo)) {
            best = dist;
            bo = o;
            bpos = pos;
            bp = c;
        }
    };
    bool fl = ok;  // flagged unless the block below certifies the answer
    if (ok) {  // (uniform over the kLanes lanes of a query)
        const int32_t tg = warm[i];
        if (tg >= 0 && tg < T) {  // every lane of the query evaluates the warm triangle: the same bound everywhere
            const Corners w = gather_corners(v, tri, tg);
            consider(w.A, w.B, w.C, (int)tg, (unsigned)(tri_orig ? tri_orig[tg] : tg));
        }
        if (best < __builtin_huge_val()) {  // (NaN / no warm triangle: stays flagged)
            const double bound = best;  // the ball every candidate is tested against (the running best only shrinks inside it)
            const double r = sqrt(bound) * (1.0 + 1e-9) + 1e-300;
            int32_t total;
            if (grid_ball_runs<kLanes>(g, qx, qy, qz, r, ql, cell_s[qi], cell_off[qi], total)) {
                // (2) all entries of the runs, flattened over the lanes: the box against the ball; survivors go to the query's list
                int ncand = 0, k = 0;
                bool overflow = false;
                for (int32_t base = 0; base < total; base += kLanes) {
                    const int32_t idx = base + ql;
                    bool pass = false;
                    int32_t e = 0;
                    if (idx < total) {
                        while (cell_off[qi][k + 1] <= idx) ++k;
                        e = cell_s[qi][k] + (idx - cell_off[qi][k]);
                        pass = !(point_box_gap2(qx, qy, qz, g.boxes + (int64_t)e * 6) > bound);  // (equal: a possible tie, evaluated)
                    }
                    const unsigned hm = (unsigned)(__ballot(pass) >> (kLanes * wslot)) & (kLanes == 32 ? 0xffffffffu : ((1u << (kLanes & 31)) - 1u));
                    if (pass) {
                        const int slot = ncand + __builtin_popcount(hm & ((1u << ql) - 1u));
                        if (slot < kTriGridCand) cand[qi][slot] = e;
                    }
                    ncand += __builtin_popcount(hm);
                }
                if (ncand > kTriGridCand) overflow = true, ncand = 0;
                __threadfence_block();
                // (3) the exact routine on the survivors, one per lane
                for (int c = ql; c < ncand; c += kLanes) {
                    const double *rc = g.recs + (int64_t)cand[qi][c] * kTriRec;
                    const long long meta = __builtin_bit_cast(long long, rc[9]);
                    consider(V3{rc[0], rc[1], rc[2]}, V3{rc[3], rc[4], rc[5]}, V3{rc[6], rc[7], rc[8]}, (int)(meta & 0xffffffffLL),
                             (unsigned)((unsigned long long)meta >> 32));
                }
                fl = overflow;
            }
        }
    }
    // combine the lanes of the query: smallest distance, then lowest original triangle
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        const int op = __shfl_xor(bpos, off);
        if (take_better(best, bo, bp, off)) bpos = op;
    }
    if (ok && ql == 0) {
        flag[i] = fl ? 1 : 0;
        if (!fl) {
            cp[i] = bp.x;
            cp[q.n + i] = bp.y;
            cp[2 * q.n + i] = bp.z;
            d2out[i] = best;
            if (tri_out) tri_out[i] = (int32_t)bo;
            warm[i] = bpos;
        }
    }
    count_flagged(ok && ql == 0 && fl, nflag);
}

// bary[3 i + k]: weight of corner k of triangle tri_id[i] (original numbering; corners given in `tri_corners` [3 T] as positions in
// the cloud v) for query i
__global__ __launch_bounds__(256) void barycentric_kernel(Cloud q, Cloud v, const int32_t *__restrict__ tri_by_orig,
                                                          const int32_t *__restrict__ tri_id, double *__restrict__ bary) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= q.n) return;
    const int64_t t = tri_id[i];
    const Corners c = gather_corners(v, tri_by_orig, t);
    const V3 w = closest_barycentric(V3{q.x[i], q.y[i], q.z[i]}, c.A, c.B, c.C);
    bary[3 * i] = w.x;
    bary[3 * i + 1] = w.y;
    bary[3 * i + 2] = w.z;
}

}  // namespace

void launch_barycentric(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri_by_orig, const int32_t *tri_id, double *bary) {
    hipLaunchKernelGGL(barycentric_kernel, dim3((unsigned)ceil_div(q.n, 256)), dim3(256), 0, ctx->stream, q, v, tri_by_orig, tri_id, bary);
}
void launch_surface_closest_point(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri, const int32_t *tri_orig, int64_t T,
                                  const double *boxes, double *cp_soa, double *d2, int32_t *tri_out, int32_t *warm, bool warm_valid,
                                  const double *tribox, const uint8_t *mask, const int32_t *nmask) {
    // queries per workgroup = 64 / H.  The kernel is bound by its longest workgroups: fewer queries per workgroup = more, shorter
    // workgroups and a tighter query box for the tile pruning.
    // warm: one int32 per query, read as last call's winning triangles when warm_valid, rewritten with this call's
    const int32_t *win = (warm && warm_valid) ? warm : (const int32_t *)nullptr;
    with_surface_h(surface_h(q.n), [&](auto H) {
        constexpr int kH = decltype(H)::value;
        hipLaunchKernelGGL(surface_cp_queue_kernel<kH>, dim3((unsigned)ceil_div(q.n, 64 / kH)), dim3(kCpThreads), 0, ctx->stream, q, v, tri,
                           tri_orig, T, boxes, cp_soa, d2, tri_out, win, warm, tribox, mask, nmask);
    });
}

// closest point of every query the grid certifies (warm start required: `warm` holds last scan's triangles); the others are flagged
// (g.flag, g.cur_nflag()) for the masked launch_surface_closest_point that must follow
void launch_surface_cp_grid(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri, const int32_t *tri_orig, int64_t T, TriGrid &g,
                            double *cp_soa, double *d2, int32_t *tri_out, int32_t *warm) {
    g.parity ^= 1;
    int32_t *cur = g.nflag + g.parity, *next = g.nflag + (g.parity ^ 1);
    constexpr int kLanes = GINGR_TRI_GRID_LANES;  // queries per wave = 64 / kLanes: their entries and candidates are spread over the lanes
    hipLaunchKernelGGL(surface_cp_grid_kernel<kLanes>, dim3((unsigned)ceil_div(q.n, 256 / kLanes)), dim3(256), 0, ctx->stream, q, v, tri, tri_orig,
                       T, g.v, cp_soa, d2, tri_out, warm, g.flag, cur, next);
}
