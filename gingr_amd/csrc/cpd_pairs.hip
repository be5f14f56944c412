// The two all-pairs passes of the CPD update for gfx950 (MI355X): soft-assignment statistics in two streaming passes (P is never
// materialised), the kernels that combine their chunk partials, and their launchers.
//
// Reference loops replaced (G/ = src/main/scala/gingr/):
//   cpd_colsum   : K_ij and its column sums               G/api/registration/config/CPD.scala:63-68,71
//   cpd_rowstats : P_ij = K_ij/den_j, P1 = row sums, P*X  CPD.scala:36-45,74,138,144
//
// Shape of both CPD passes: a thread keeps PT points of the "owned" side in registers (targets in pass 1, fit points
// in pass 2), the other side streams through LDS in 256-point tiles read with wave-uniform (broadcast) 16-byte
// reads, so HBM traffic is O(M+N) per block column and the kernels are bound by float64 VALU issue (the software
// exponential), not by memory.  The streamed dimension is split into chunks (gridDim.y, cpd_plan.h) so that >> 256 workgroups
// exist; chunk partials are combined by a second kernel in a FIXED order (no float atomics: results are bitwise
// reproducible run to run).
#include "common.h"
#include "block_sum.h"
#include "box_device.h"
#include "cpd_plan.h"
#include "fastexp.h"

namespace {

constexpr int kBlock = 256;

// Table of the two CPD passes: 2^11 entries (16 KB of LDS), floor form (fastexp.h).  An 8192-entry table (byte offset by one SDWA
// shift) was measured in round 1 and lost to its LDS footprint; the floor form gets the one-instruction offset with 2048 entries.
constexpr int kTB = 11;
constexpr int kTabN = 1 << kTB;

// -DGINGR_STAMPS (diagnostic builds only: `make variant NAME=stamps DEFS=-DGINGR_STAMPS`, tools/stamps_shard.py): every wave of the
// two CPD pair loops leaves eight 64-bit words per launch in a device buffer -- the 100 MHz wall clock at entry / owned points and
// boxes ready / table barrier passed / first quarter staged / pair loop done / exit, the core-clock cycles of the whole wave, and
// its hardware id -- so that a one-round launch (a short row shard) can be taken apart per wave.  Nothing of it exists in the product build.
#ifdef GINGR_STAMPS
__device__ unsigned long long *g_stamp_buf = nullptr;   // [2 kernels][kStampWaves][8]
constexpr int kStampWaves = 1 << 15;
struct Stamps {
    unsigned long long *p;
    long long c0;
    __device__ __forceinline__ void begin(int kernel) {
        const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x;
        const unsigned w = wg * 4 + (threadIdx.x >> 6);
        p = (g_stamp_buf && w < kStampWaves) ? g_stamp_buf + ((size_t)kernel * kStampWaves + w) * 8 : nullptr;
        c0 = clock64();
        mark(0);
    }
    __device__ __forceinline__ void mark(int slot) {
        const unsigned long long t = wall_clock64();
        if (p && (threadIdx.x & 63) == 0) p[slot] = t;
    }
    __device__ __forceinline__ void end() {
        mark(5);
        if (p && (threadIdx.x & 63) == 0) {
            p[6] = (unsigned long long)(clock64() - c0);
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            p[7] = ((unsigned long long)xcc << 32) | hw;
        }
    }
};
#define STAMP_DECL Stamps stamps__;
#define STAMP_BEGIN(k) stamps__.begin(k);
#define STAMP(slot) stamps__.mark(slot);
#define STAMP_END stamps__.end();
#else
#define STAMP_DECL
#define STAMP_BEGIN(k)
#define STAMP(slot)
#define STAMP_END
#endif

// ---------------------------------------------------------------- exact-zero culling
// K_ij = 2^(c d2 / table size) is flushed to exactly +0 by v_ldexp_f64 once c*d2/size < -1076, i.e. d2 > 1491.7 sigma2.  When the
// bounding boxes of the owned block and of a streamed 256-point tile are farther apart than that (with margin: 1500
// sigma2), every pair of the tile pair contributes exactly +0 to every sum and the tile is skipped: bit-identical results.
// This only triggers when the points are spatially coherent (the fitter keeps model rows and targets in k-d leaf order).
// 1500 * sigma2 * (-c), with -c = table size * log2(e) / (2 sigma2)
#define GINGR_CULL_SCALED(entries) (1084.0 * (double)(entries))
constexpr double kFineCullRatio = 16.0;  // fine culling once the flush radius is below a quarter of the largest possible distance

// bounding box of a wave's owned points (invalid slots excluded), wave-uniform, in scalar registers.  In the CPD passes all four
// waves of a workgroup hold the SAME owned points, so this is also the workgroup's box -- computed redundantly, no LDS, and
// bit-identical in every wave (block-uniform branches may depend on it).
template <int PT>
__device__ __forceinline__ Box wave_bbox(const double (&x)[PT], const double (&y)[PT], const double (&z)[PT], const bool (&ok)[PT]) {
    double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
    double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
#pragma unroll
    for (int t = 0; t < PT; ++t)
        if (ok[t]) {
            lo[0] = fmin(lo[0], x[t]); hi[0] = fmax(hi[0], x[t]);
            lo[1] = fmin(lo[1], y[t]); hi[1] = fmax(hi[1], y[t]);
            lo[2] = fmin(lo[2], z[t]); hi[2] = fmax(hi[2], z[t]);
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
        }
    Box b;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        b.lo[d] = uniform_d(lo[d]);
        b.hi[d] = uniform_d(hi[d]);
    }
    return b;
}

// bounding box of each owned slot t over the wave: the 64 consecutive points {base + 64 t + lane} (a quarter k-d leaf); wave
// uniform, kept in scalar registers (measured faster than a round trip through LDS, spills included)
template <int PT>
__device__ __forceinline__ void slot_boxes(const double (&x)[PT], const double (&y)[PT], const double (&z)[PT],
                                           const bool (&ok)[PT], Box (&sb)[PT]) {
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        double lo[3] = {ok[t] ? x[t] : __builtin_huge_val(), ok[t] ? y[t] : __builtin_huge_val(), ok[t] ? z[t] : __builtin_huge_val()};
        double hi[3] = {ok[t] ? x[t] : -__builtin_huge_val(), ok[t] ? y[t] : -__builtin_huge_val(), ok[t] ? z[t] : -__builtin_huge_val()};
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
                hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
            }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sb[t].lo[d] = uniform_d(lo[d]);
            sb[t].hi[d] = uniform_d(hi[d]);
        }
    }
}

// Lane-parallel exact-zero culling for one wave: the tile parts of a chunk (part p = box tile t0 + p, clipped to the chunk
// [c0, c1)) are tested 64 at a time -- lane l tests part pbase + l against the box of the wave's quarter q of that part -- and the
// outcome comes back as wave-uniform bit masks, so the walk over the parts (PartWalk::next) is scalar code with no per-part box
// arithmetic (uniform float64 arithmetic still costs full VALU instructions on gfx950: 12 per test, ~1.5 % of a dense pass).
//   act     bit l: the wave's quarter of part pbase + l exists and can receive non-zeros
//   slot[t] (FINE) bit l: owned slot t can receive non-zeros from it
// bad (nullable): per box tile, non-zero = never cull (a non-finite 1/den: 0 * inf must stay NaN).  boxes == nullptr: nothing is culled.
template <int PT, bool FINE>
struct PartWalk {
    int64_t c0, c1, t0;
    int nparts, pbase, q;
    unsigned long long act, slot[PT];
    const double *sub;      // quarter boxes, [6] per 64 points of the streamed cloud
    const int32_t *bad;
    double negc;

    __device__ __forceinline__ void init(int64_t c0_, int64_t c1_, int q_, const double *sub_, const int32_t *bad_, double negc_) {
        c0 = c0_;
        c1 = c1_;
        q = q_;
        sub = sub_;
        bad = bad_;
        negc = negc_;
        t0 = c0 / kTile;
        nparts = c1 > c0 ? (int)((c1 - 1) / kTile - t0 + 1) : 0;
        pbase = 0;
        act = 0;
    }
    __device__ __forceinline__ void bounds(int p, int64_t *ib, int64_t *ie) const {
        const int64_t a = (t0 + p) * kTile, b = a + kTile;
        *ib = a > c0 ? a : c0;
        *ie = b < c1 ? b : c1;
    }
    __device__ __forceinline__ void batch(const Box &own, const Box (&sown)[PT]) {
        const int lane = threadIdx.x & 63;
        const int p = pbase + lane;
        int64_t ib, ie;
        bounds(p, &ib, &ie);
        const bool has = p < nparts && q * 64 < (int)(ie - ib);
        bool on = has;
        bool son[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) son[t] = has;
        if (has && sub && !(bad && bad[(t0 + p)])) {
            const double *qbox = sub + (ib / 64 + q) * 6;
            if (FINE) {
                on = false;
#pragma unroll
                for (int t = 0; t < PT; ++t) {
                    son[t] = !(box_gap2(sown[t], qbox) * negc > GINGR_CULL_SCALED(kTabN));  // NaN boxes are never culled
                    on = on || son[t];
                }
            } else {
                on = !(box_gap2(own, qbox) * negc > GINGR_CULL_SCALED(kTabN));
            }
        }
        act = __ballot(on);
        if (FINE) {
#pragma unroll
            for (int t = 0; t < PT; ++t) slot[t] = __ballot(son[t]);
        }
        pbase += 64;
    }
    // next part with work for this wave: false when the chunk is exhausted
    __device__ __forceinline__ bool next(const Box &own, const Box (&sown)[PT], int64_t *ib, int64_t *ie, unsigned *mask) {
        while (act == 0) {
            if (pbase >= nparts) return false;
            batch(own, sown);
        }
        const int l = __builtin_ctzll(act);
        act &= act - 1;
        bounds(pbase - 64 + l, ib, ie);
        unsigned m = (1u << PT) - 1u;
        if (FINE) {
            m = 0;
#pragma unroll
            for (int t = 0; t < PT; ++t) m |= (unsigned)((slot[t] >> l) & 1ull) << t;
        }
        *mask = m;
        return true;
    }
};

// One launch round (every workgroup resident from the start, e.g. the row shard of an 8-rank job): the SIMD arbiter favours the
// oldest wave, so the four waves of a SIMD finish one after the other (time stamps: 53 / 80 / 107 / 141 us of a 148 us launch) and
// the last one runs alone at the single-wave rate of one instruction per ~5.3 cycles.  Lowering a wave's priority as it advances
// keeps the four abreast until the end.  Not used when rounds overlap: there the stagger hides the prologues.
__device__ __forceinline__ void fair_priority(int64_t done, int64_t total) {
    const int64_t f = total > 0 ? (4 * done) / total : 3;
    if (f <= 0)
        __builtin_amdgcn_s_setprio(3);
    else if (f == 1)
        __builtin_amdgcn_s_setprio(2);
    else if (f == 2)
        __builtin_amdgcn_s_setprio(1);
    else
        __builtin_amdgcn_s_setprio(0);
}

// ---------------------------------------------------------------- pass 1: column sums of K
// Tile loops.  [j0, j1) is a range of tile entries (the whole tile or one 64-point quarter); with MASKED only the owned slots
// t whose bit is set in `mask` (wave-uniform) are updated -- the others are known to receive exact zeros from this range.
template <int PT, bool CLAMP, bool MASKED>
__device__ __forceinline__ void colsum_tile(const P4 *tile, int j0, int j1, unsigned mask, const double (&x)[PT],
                                            const double (&y)[PT], const double (&z)[PT], double (&acc)[PT], double c, double lim,
                                            const double *T) {
#pragma unroll 2
    for (int ii = j0; ii < j1; ++ii) {
        const P4 p = tile[ii];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            if (MASKED && !((mask >> t) & 1u)) continue;
            const double dx = x[t] - p.x, dy = y[t] - p.y, dz = z[t] - p.z;
            double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
            if (CLAMP) d2 = fastexp_clamp_d2(d2, lim);
            acc[t] += fastexp2_floor_scaled(d2, c, T);
        }
    }
}

// Accuracy-guarded fast path: exponent argument from the norm expansion
//     t = c|x - y|^2 = c|x~|^2 + c|y~|^2 - 2c x~.y~     (x~, y~ centred on the target centroid)
// = 1 add + 3 FMAs per pair instead of the 6 + 1 instructions of the difference form.  Its cancellation error is a
// relative error of K_ij of about 7.7e-16 * R^2 / (2 sigma2) (R = cloud radius about the centroid), so it is used only
// while that bound stays below kExpandTol; otherwise the kernels fall back to the exact differences (wave-uniform choice).
constexpr double kExpandTol = 1e-12;

__device__ __forceinline__ bool use_expansion(double rmax_centered, double c) {
    // R^2 <= 3 rmax^2;  R^2 / (2 sigma2) = R^2 |c| ln2 / table size
    const double ratio = 3.0 * rmax_centered * rmax_centered * (-c) * (0.69314718055994530942 / kTabN);
    return ratio * 7.7e-16 < kExpandTol;
}

// Owned-side constants of the expansion form.  n = c|x~|^2 of an owned point is split into its nearest integer, folded into the
// magic constant of the range reduction (mg = MAGIC + rint(n): the table index and the exponent then come out for A + rint(n)
// although only A is ever added), and the fraction n - rint(n) in [-1/2, 1/2], which is a constant FACTOR 2^(frac/2048) of every
// K of that owned point and is applied once to the finished sums (expand_owned_scale).  One add per pair less.
__device__ __forceinline__ double expand_owned_magic(double n, double *frac) {
    const double ni = __builtin_rint(n);
    *frac = n - ni;  // exact
    return GINGR_EXP_MAGIC8 + ni;
}
__device__ __forceinline__ double expand_owned_scale(double frac) { return exp2(frac * (1.0 / kTabN)); }

// tile entries: (-2c y~, c|y~|^2); owned: x~ and mg = MAGIC + rint(c|x~|^2)   (float64 rounding mode: toward -inf)
template <int PT, bool MASKED>
__device__ __forceinline__ void colsum_tile_expand(const P4 *tile, int j0, int j1, unsigned mask, const double (&x)[PT],
                                                   const double (&y)[PT], const double (&z)[PT], const double (&mg)[PT],
                                                   double (&acc)[PT], const double *T) {
#pragma unroll 2
    for (int ii = j0; ii < j1; ++ii) {
        const P4 p = tile[ii];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            if (MASKED && !((mask >> t) & 1u)) continue;
            const double A = __builtin_fma(z[t], p.z, __builtin_fma(y[t], p.y, __builtin_fma(x[t], p.x, p.w)));
            acc[t] += fastexp2_floor_core(A + mg[t], __builtin_amdgcn_fract(A), T);
        }
    }
}

// Work split of both CPD passes.  A workgroup owns 64*PT points (one 256-point k-d leaf at PT = 4) and ALL FOUR of its waves hold
// the same owned points in registers; of every streamed 256-point tile wave q takes the 64-point quarter q.  The four waves'
// accumulators are added in LDS in a fixed order ((w0 + w1) + (w2 + w3)) before anything goes to memory, so a workgroup covers a
// chunk four times as long as it would with one accumulator set per wave and the launch writes a quarter of the chunk partials
// (50k x 50k: 25 instead of 98 chunks; 40 MB instead of 157 MB of row-statistics partials) for the same number of workgroups.
//
// FINE selects the variant with the quarter-tile x slot culling; it pays when the cull radius is small against the clouds (the
// regime, a property of sigma2 and the cloud extents that only the device knows).  The plain variant culls per (workgroup, tile)
// and per (wave's quarter).  Both variants give bit-identical results, so the host launches ONE of them, picked from the regime
// word the previous launches left in pinned host memory (regime_out; possibly stale -- that only costs time).  Two kernels
// rather than one with a switch: sharing one kernel cost the plain regime 7 % in the row-statistics pass.
template <int PT, bool FINE>
__global__ __launch_bounds__(kBlock) void cpd_colsum_kernel(Cloud fit, Cloud tgt, const double *__restrict__ sigma2,
                                                            const double *__restrict__ aux,
                                                            const double *__restrict__ fit_boxes, ChunkPlan plan,
                                                            double *__restrict__ partial, int32_t *regime_out) {
    __shared__ double T[kTabN];
    __shared__ P4 tile[kTile];
    __shared__ double sred[4][64 * PT];  // the waves' accumulators, combined in the epilogue
    __shared__ double sfrac[64 * PT];    // per owned point: fraction of c|x~|^2 (expansion form), parked until the epilogue
    STAMP_DECL
    STAMP_BEGIN(0)
    // Everything the prologue needs from memory is requested up front -- the exponential table, the owned points, the scalars -- so
    // that a workgroup of a one-round launch (a short row shard, a small cloud) waits for ONE round trip, not for a chain of them.
    FloorTableRegs trom;
    fastexp_floor_table_fetch256(trom);
    const double s2in = sigma2[0], aux0 = aux[0], aux1 = aux[1], cx = aux[2], cy = aux[3], cz = aux[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's number, provably uniform: loop bounds and LDS bases stay scalar
    // the workgroup's 64*PT CONSECUTIVE points (one 256-point k-d leaf at PT = 4: a compact box), the same in every wave
    const int64_t jbase = (int64_t)blockIdx.x * (64 * PT) + lane;
    double x[PT], y[PT], z[PT], n[PT], acc[PT];
    bool okv[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const int64_t j = jbase + (int64_t)t * 64;
        const bool ok = j < tgt.n;
        okv[t] = ok;
        x[t] = ok ? tgt.x[j] : 0.0;
        y[t] = ok ? tgt.y[j] : 0.0;
        z[t] = ok ? tgt.z[j] : 0.0;
    }
    // ... and the first quarter this wave will most likely stage (the first tile part of its chunk: the walk below confirms it or
    // picks another one when that part is culled)
    int64_t i0, i1;
    plan.range(blockIdx.y, fit.n, &i0, &i1);
    const int q0 = q * 64;
    double lx = 0.0, ly = 0.0, lz = 0.0;  // the staged point of the quarter about to be computed (in flight during the previous one)
    const int64_t spec_ib = i0;
    {
        const int64_t e = min((i0 / kTile + 1) * kTile, i1), i = i0 + q0 + lane;
        if (i < e) {
            lx = fit.x[i];
            ly = fit.y[i];
            lz = fit.z[i];
        }
    }
    const double c = fastexp_scale_for_variance<kTB>(2.0 * s2in);
    const double am = aux0 + aux1;
    // regime of the fine culling: the zero-flush radius is well inside the clouds' extent (3 am^2 bounds every squared distance)
    if (regime_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        *regime_out = (fit_boxes && 3.0 * am * am * (-c) > kFineCullRatio * GINGR_CULL_SCALED(kTabN)) ? 1 : 0;
        __threadfence_system();
    }
    const bool clamp = fastexp_needs_clamp(3.0 * am * am, c);               // wave-uniform
    const bool expand = use_expansion(fmax(aux0, aux1), c);                 // wave-uniform
    const double lim = fastexp_d2_limit<kTB>(c);
    const double m2c = -2.0 * c;
    fastexp_floor_table_park256(T, trom);
    const Box own = wave_bbox<PT>(x, y, z, okv);  // raw coordinates, before any centring
    constexpr unsigned kAllSlots = (1u << PT) - 1u;
    Box sown[PT];  // per owned slot (64 consecutive points)
    if (FINE) slot_boxes<PT>(x, y, z, okv, sown);
    const double *fit_sub = fit_boxes ? fit_boxes + ((fit.n + kTile - 1) / kTile) * 6 : nullptr;
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        if (expand) {
            x[t] -= cx;
            y[t] -= cy;
            z[t] -= cz;
        }
        double fr;
        n[t] = expand_owned_magic(c * __builtin_fma(z[t], z[t], __builtin_fma(y[t], y[t], x[t] * x[t])), &fr);
        if (q == 0) sfrac[t * 64 + lane] = fr;
        acc[t] = 0.0;
    }
    STAMP(1)
    __syncthreads();       // the exponential table (filled by all four waves) and sfrac are complete
    STAMP(2)
    fastexp_round_down();  // the floor form of the exponential needs it; every float64 result up to the epilogue rounds down
    // A chunk starts and ends on 64-point quarters, not necessarily on tiles: every step handles the part of ONE box tile that lies
    // inside the chunk, so the tile / quarter boxes apply unchanged.  Of each part wave q takes the quarter q: it stages those 64
    // entries itself into its own slice of `tile` and is the only reader, so the pair loop has no workgroup barrier -- the waves
    // run decoupled -- and the loads of the wave's NEXT quarter are issued before the pairs of the current one are computed.
    struct Work {
        int64_t ib, ie;
        unsigned mask;
        bool valid;
    };
    PartWalk<PT, FINE> walk;
    walk.init(i0, i1, q, fit_boxes ? fit_sub : nullptr, nullptr, -c);
    auto find = [&]() {  // next tile part of the chunk in which this wave's quarter can receive non-zeros
        Work w{0, 0, kAllSlots, false};
        w.valid = walk.next(own, sown, &w.ib, &w.ie, &w.mask);
        return w;
    };
    auto issue = [&](const Work &w) {
        const int64_t i = w.ib + q0 + lane;
        if (i < w.ie) {
            lx = fit.x[i];
            ly = fit.y[i];
            lz = fit.z[i];
        }
    };
    Work cur = find();
    if (cur.valid && cur.ib != spec_ib) issue(cur);  // (otherwise the prologue's request was the right one)
#ifdef GINGR_STAMPS
    bool first__ = true;
#endif
    while (cur.valid) {
        if (plan.fair) fair_priority(cur.ib - i0, i1 - i0);
        __builtin_amdgcn_wave_barrier();  // (compiler fence) the previous quarter's reads are issued before the slice is rewritten
        if (cur.ib + q0 + lane < cur.ie) {
            if (expand) {
                const double fx = lx - cx, fy = ly - cy, fz = lz - cz;
                tile[q0 + lane] = P4{m2c * fx, m2c * fy, m2c * fz, c * __builtin_fma(fz, fz, __builtin_fma(fy, fy, fx * fx))};
            } else {
                tile[q0 + lane] = P4{lx, ly, lz, 0.0};
            }
        }
        __builtin_amdgcn_wave_barrier();  // LDS serves one wave's accesses in order: its reads below see its own writes
#ifdef GINGR_STAMPS
        if (first__) { STAMP(3) first__ = false; }
#endif
        const Work nxt = find();
        if (nxt.valid) issue(nxt);
        const int q1 = min((int)(cur.ie - cur.ib), q0 + 64);
        const unsigned mask = cur.mask;
        if (expand) {
            if (!FINE || mask == kAllSlots)
                colsum_tile_expand<PT, false>(tile, q0, q1, mask, x, y, z, n, acc, T);
            else
                colsum_tile_expand<PT, true>(tile, q0, q1, mask, x, y, z, n, acc, T);
        } else if (clamp) {
            if (!FINE || mask == kAllSlots)
                colsum_tile<PT, true, false>(tile, q0, q1, mask, x, y, z, acc, c, lim, T);
            else
                colsum_tile<PT, true, true>(tile, q0, q1, mask, x, y, z, acc, c, lim, T);
        } else {
            if (!FINE || mask == kAllSlots)
                colsum_tile<PT, false, false>(tile, q0, q1, mask, x, y, z, acc, c, lim, T);
            else
                colsum_tile<PT, false, true>(tile, q0, q1, mask, x, y, z, acc, c, lim, T);
        }
        cur = nxt;
    }
    fastexp_round_nearest();
    STAMP(4)
#pragma unroll
    for (int t = 0; t < PT; ++t) sred[q][t * 64 + lane] = acc[t];
    __syncthreads();
    for (int p = tid; p < 64 * PT; p += kBlock) {
        double v = (sred[0][p] + sred[1][p]) + (sred[2][p] + sred[3][p]);
        if (expand) v *= expand_owned_scale(sfrac[p]);
        const int64_t j = (int64_t)blockIdx.x * (64 * PT) + p;
        if (j < tgt.n) partial[(int64_t)blockIdx.y * tgt.n + j] = v;
    }
    STAMP_END
}

// out[j] = sum over chunks (ascending) of partial[chunk][j]
__global__ void chunk_reduce_kernel(const double *__restrict__ partial, int nchunks, int64_t n, double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partial[(int64_t)c * n + j];
    out[j] = s;
}

// den[j] = colsum[j] + c ; inv_den ; Pt1 ; per-block partial of xPx = sum_j Pt1_j |x_j|^2.
// Always launched with kScalarBlocks workgroups; part[0..kScalarBlocks) receives the xPx partials.
constexpr int kScalarBlocks = 256;

// chunk_partial != nullptr (single shard): the column sums are still spread over the nchunks chunk partials of the column-sum
// pass and are added up here, in ascending chunk order like chunk_reduce_kernel (one launch and one pass over den less).
__global__ __launch_bounds__(256) void cpd_den_finalize_kernel(Cloud tgt, const double *__restrict__ sigma2, double w,
                                                               double m_over_n, double *__restrict__ den,
                                                               double *__restrict__ inv_den, double *__restrict__ Pt1,
                                                               int32_t *__restrict__ tile_bad, double *__restrict__ part,
                                                               double *__restrict__ scalars,
                                                               const double *__restrict__ chunk_partial, int nchunks) {
    __shared__ double sh[256];
    const double s2 = sigma2[0];
    // c = w/(1-w) * (2 pi sigma2)^(3/2) * (M/N)     CPD.scala:69-70
    const double c = w / (1.0 - w) * pow(2.0 * 3.14159265358979323846 * s2, 1.5) * m_over_n;
    double xpx = 0.0;
    // one 256-point tile per workgroup and pass (block stride = tile size), so tile_bad needs no clearing beforehand
    for (int64_t jt = (int64_t)blockIdx.x * 256; jt < tgt.n; jt += (int64_t)kScalarBlocks * 256) {
        const int64_t j = jt + threadIdx.x;
        int bad = 0;
        if (j < tgt.n) {
        double colsum;
        if (chunk_partial) {
            colsum = 0.0;
#pragma unroll 8
            for (int ch = 0; ch < nchunks; ++ch) colsum += chunk_partial[(int64_t)ch * tgt.n + j];  // loads ahead, adds in order
        } else {
            colsum = den[j];
        }
        const double d = colsum + c;
        const double inv = 1.0 / d;
        const double pt1 = colsum / d;
        den[j] = d;
        inv_den[j] = inv;
        Pt1[j] = pt1;
        bad = !(fabs(inv) <= 1.79769313486231570815e308);  // never cull this tile
        const double xx = tgt.x[j], yy = tgt.y[j], zz = tgt.z[j];
        xpx += pt1 * (xx * xx + yy * yy + zz * zz);
        }
        const int any_bad = __syncthreads_or(bad);
        if (tile_bad && threadIdx.x == 0) tile_bad[jt / kTile] = any_bad;
    }
    const double tot = block_sum<256>(xpx, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = tot;
        if (blockIdx.x == 0) scalars[5] = c;
    }
}

// ---------------------------------------------------------------- pass 2: row statistics
// tile entries: (x, y, z, 1/den); tw entries: (x, y, z)/den, so that P1 and P.X are four FMAs on K_ij (the product
// K * (x/den) instead of (K/den) * x: one rounding placed differently, one instruction less per pair)
template <int PT, bool CLAMP, bool MASKED>
__device__ __forceinline__ void rowstats_tile(const P4 *tile, const P4 *tw, int j0, int j1, unsigned mask,
                                              const double (&x)[PT], const double (&y)[PT], const double (&z)[PT],
                                              double (&a1)[PT], double (&ax)[PT], double (&ay)[PT], double (&az)[PT], double c,
                                              double lim, const double *T) {
#pragma unroll 2
    for (int jj = j0; jj < j1; ++jj) {
        const P4 p = tile[jj];
        const P4 q = tw[jj];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            if (MASKED && !((mask >> t) & 1u)) continue;
            const double dx = p.x - x[t], dy = p.y - y[t], dz = p.z - z[t];
            double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
            if (CLAMP) d2 = fastexp_clamp_d2(d2, lim);
            const double k = fastexp2_floor_scaled(d2, c, T);
            a1[t] = __builtin_fma(k, p.w, a1[t]);
            ax[t] = __builtin_fma(k, q.x, ax[t]);
            ay[t] = __builtin_fma(k, q.y, ay[t]);
            az[t] = __builtin_fma(k, q.z, az[t]);
        }
    }
}

// expansion form of pass 2: tile entries (-2c x~, c|x~|^2) + 1/den; owned y~ and n = c|y~|^2.  P.X is accumulated as
// sum_j p a_j with a_j = -2c x~_j and rescaled once at the end: PX = ctr*P1 - (sum_j p a_j) / (2c).
// tw entries: (a_j / den_j, 1 / den_j)
template <int PT, bool MASKED>
__device__ __forceinline__ void rowstats_tile_expand(const P4 *tile, const P4 *tw, int j0, int j1, unsigned mask,
                                                     const double (&x)[PT], const double (&y)[PT], const double (&z)[PT],
                                                     const double (&mg)[PT], double (&a1)[PT], double (&ax)[PT], double (&ay)[PT],
                                                     double (&az)[PT], const double *T) {
#pragma unroll 2
    for (int jj = j0; jj < j1; ++jj) {
        const P4 p = tile[jj];
        const P4 q = tw[jj];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            if (MASKED && !((mask >> t) & 1u)) continue;
            const double A = __builtin_fma(z[t], p.z, __builtin_fma(y[t], p.y, __builtin_fma(x[t], p.x, p.w)));
            const double k = fastexp2_floor_core(A + mg[t], __builtin_amdgcn_fract(A), T);
            a1[t] = __builtin_fma(k, q.w, a1[t]);
            ax[t] = __builtin_fma(k, q.x, ax[t]);
            ay[t] = __builtin_fma(k, q.y, ay[t]);
            az[t] = __builtin_fma(k, q.z, az[t]);
        }
    }
}

// __launch_bounds__'s second argument (waves per SIMD): with four points per thread the kernel cannot hold four waves anyway; telling
// the compiler that three are enough lets it use up to 168 registers instead of parking values in accumulator registers inside
// the pair loop (17 extra v_accvgpr moves per 8 pairs at the default heuristic).
template <int PT, bool FINE>  // work split, FINE / regime_out: see cpd_colsum_kernel
__global__ __launch_bounds__(kBlock, (PT >= 4 ? 3 : 4)) void cpd_rowstats_kernel(Cloud fit, Cloud tgt, const double *__restrict__ sigma2,
                                                              const double *__restrict__ aux,
                                                              const double *__restrict__ inv_den,
                                                              const double *__restrict__ tgt_boxes,
                                                              const int32_t *__restrict__ tile_bad, ChunkPlan plan,
                                                              double *__restrict__ partial, int32_t *regime_out) {
    // one LDS block: [T | tile | tw] during the pair loop, the waves' accumulators [4 waves][4 planes][64 PT] in the epilogue
    constexpr int kRed = 4 * 4 * 64 * PT;
    constexpr int kLoop = kTabN + 4 * kTile + 4 * kTile;
    __shared__ double smem[kRed > kLoop ? kRed : kLoop];
    __shared__ double sfrac[64 * PT];  // see cpd_colsum_kernel
    double *T = smem;
    P4 *tile = reinterpret_cast<P4 *>(smem + kTabN);
    P4 *tw = reinterpret_cast<P4 *>(smem + kTabN + 4 * kTile);
    STAMP_DECL
    STAMP_BEGIN(1)
    FloorTableRegs trom;  // table, owned points, scalars and the first quarter are requested together: see cpd_colsum_kernel
    fastexp_floor_table_fetch256(trom);
    const double s2in = sigma2[0], aux0 = aux[0], aux1 = aux[1], cx = aux[2], cy = aux[3], cz = aux[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave's number, provably uniform: loop bounds and LDS bases stay scalar
    const int64_t ibase = (int64_t)blockIdx.x * (64 * PT) + lane;
    double x[PT], y[PT], z[PT], n[PT], a1[PT], ax[PT], ay[PT], az[PT];
    bool okv[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const int64_t i = ibase + (int64_t)t * 64;
        const bool ok = i < fit.n;
        okv[t] = ok;
        x[t] = ok ? fit.x[i] : 0.0;
        y[t] = ok ? fit.y[i] : 0.0;
        z[t] = ok ? fit.z[i] : 0.0;
    }
    int64_t j0, j1;
    plan.range(blockIdx.y, tgt.n, &j0, &j1);
    const int q0 = q * 64;
    double lx = 0.0, ly = 0.0, lz = 0.0, linv = 0.0;
    const int64_t spec_jb = j0;
    {
        const int64_t e = min((j0 / kTile + 1) * kTile, j1), j = j0 + q0 + lane;
        if (j < e) {
            lx = tgt.x[j];
            ly = tgt.y[j];
            lz = tgt.z[j];
            linv = inv_den[j];
        }
    }
    const double c = fastexp_scale_for_variance<kTB>(2.0 * s2in);
    const double am = aux0 + aux1;
    if (regime_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        *regime_out = (tgt_boxes && 3.0 * am * am * (-c) > kFineCullRatio * GINGR_CULL_SCALED(kTabN)) ? 1 : 0;
        __threadfence_system();
    }
    const bool clamp = fastexp_needs_clamp(3.0 * am * am, c);               // wave-uniform
    const bool expand = use_expansion(fmax(aux0, aux1), c);                 // wave-uniform
    const double lim = fastexp_d2_limit<kTB>(c);
    const double m2c = -2.0 * c;
    fastexp_floor_table_park256(T, trom);
    const Box own = wave_bbox<PT>(x, y, z, okv);  // raw coordinates, before any centring; identical in every wave
    constexpr unsigned kAllSlots = (1u << PT) - 1u;
    Box sown[PT];  // per owned slot (64 consecutive points)
    if (FINE) slot_boxes<PT>(x, y, z, okv, sown);
    const double *tgt_sub = tgt_boxes ? tgt_boxes + ((tgt.n + kTile - 1) / kTile) * 6 : nullptr;
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        if (expand) {
            x[t] -= cx;
            y[t] -= cy;
            z[t] -= cz;
        }
        double fr;
        n[t] = expand_owned_magic(c * __builtin_fma(z[t], z[t], __builtin_fma(y[t], y[t], x[t] * x[t])), &fr);
        if (q == 0) sfrac[t * 64 + lane] = fr;
        a1[t] = ax[t] = ay[t] = az[t] = 0.0;
    }
    STAMP(1)
    __syncthreads();       // the exponential table (filled by all four waves) and sfrac are complete
    STAMP(2)
    fastexp_round_down();  // see cpd_colsum_kernel
    // one box tile (or the part of it inside the chunk) per step, wave q on quarter q, next quarter's loads in flight: see
    // cpd_colsum_kernel
    struct Work {
        int64_t jb, je;
        unsigned mask;
        bool valid;
    };
    PartWalk<PT, FINE> walk;
    walk.init(j0, j1, q, tgt_boxes ? tgt_sub : nullptr, tgt_boxes ? tile_bad : nullptr, -c);
    auto find = [&]() {
        Work w{0, 0, kAllSlots, false};
        w.valid = walk.next(own, sown, &w.jb, &w.je, &w.mask);
        return w;
    };
    auto issue = [&](const Work &w) {
        const int64_t j = w.jb + q0 + lane;
        if (j < w.je) {
            lx = tgt.x[j];
            ly = tgt.y[j];
            lz = tgt.z[j];
            linv = inv_den[j];
        }
    };
    Work cur = find();
    if (cur.valid && cur.jb != spec_jb) issue(cur);  // (otherwise the prologue's request was the right one)
#ifdef GINGR_STAMPS
    bool first__ = true;
#endif
    while (cur.valid) {
        if (plan.fair) fair_priority(cur.jb - j0, j1 - j0);
        __builtin_amdgcn_wave_barrier();
        if (cur.jb + q0 + lane < cur.je) {
            const double inv = linv;
            if (expand) {
                const double tx = lx - cx, ty = ly - cy, tz = lz - cz;
                const double ax_ = m2c * tx, ay_ = m2c * ty, az_ = m2c * tz;
                tile[q0 + lane] = P4{ax_, ay_, az_, c * __builtin_fma(tz, tz, __builtin_fma(ty, ty, tx * tx))};
                tw[q0 + lane] = P4{ax_ * inv, ay_ * inv, az_ * inv, inv};
            } else {
                tile[q0 + lane] = P4{lx, ly, lz, inv};
                tw[q0 + lane] = P4{lx * inv, ly * inv, lz * inv, inv};
            }
        }
        __builtin_amdgcn_wave_barrier();
#ifdef GINGR_STAMPS
        if (first__) { STAMP(3) first__ = false; }
#endif
        const Work nxt = find();
        if (nxt.valid) issue(nxt);
        const int q1 = min((int)(cur.je - cur.jb), q0 + 64);
        const unsigned mask = cur.mask;
        if (expand) {
            if (!FINE || mask == kAllSlots)
                rowstats_tile_expand<PT, false>(tile, tw, q0, q1, mask, x, y, z, n, a1, ax, ay, az, T);
            else
                rowstats_tile_expand<PT, true>(tile, tw, q0, q1, mask, x, y, z, n, a1, ax, ay, az, T);
        } else if (clamp) {
            if (!FINE || mask == kAllSlots)
                rowstats_tile<PT, true, false>(tile, tw, q0, q1, mask, x, y, z, a1, ax, ay, az, c, lim, T);
            else
                rowstats_tile<PT, true, true>(tile, tw, q0, q1, mask, x, y, z, a1, ax, ay, az, c, lim, T);
        } else {
            if (!FINE || mask == kAllSlots)
                rowstats_tile<PT, false, false>(tile, tw, q0, q1, mask, x, y, z, a1, ax, ay, az, c, lim, T);
            else
                rowstats_tile<PT, false, true>(tile, tw, q0, q1, mask, x, y, z, a1, ax, ay, az, c, lim, T);
        }
        cur = nxt;
    }
    fastexp_round_nearest();
    STAMP(4)
    // combine the four waves in a fixed order; the LDS block is reused, so everybody must be done with T / tile / tw first
    __syncthreads();
    constexpr int kPts = 64 * PT;
    double *sred = smem;
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        sred[(q * 4 + 0) * kPts + t * 64 + lane] = a1[t];
        sred[(q * 4 + 1) * kPts + t * 64 + lane] = ax[t];
        sred[(q * 4 + 2) * kPts + t * 64 + lane] = ay[t];
        sred[(q * 4 + 3) * kPts + t * 64 + lane] = az[t];
    }
    __syncthreads();
    const int64_t M = fit.n;
    double *base = partial + (int64_t)blockIdx.y * 4 * M;
    const double back = expand ? -0.5 / c : 1.0;  // sum_j p a_j -> sum_j p x~_j
    for (int p = tid; p < kPts; p += kBlock) {
        double v[4];
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
            v[pl] = (sred[(0 * 4 + pl) * kPts + p] + sred[(1 * 4 + pl) * kPts + p]) + (sred[(2 * 4 + pl) * kPts + p] + sred[(3 * 4 + pl) * kPts + p]);
        if (expand) {
            const double e = expand_owned_scale(sfrac[p]);
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) v[pl] *= e;
        }
        const int64_t i = (int64_t)blockIdx.x * kPts + p;
        if (i < M) {
            base[i] = v[0];
            base[M + i] = expand ? __builtin_fma(cx, v[0], back * v[1]) : v[1];
            base[2 * M + i] = expand ? __builtin_fma(cy, v[0], back * v[2]) : v[2];
            base[3 * M + i] = expand ? __builtin_fma(cz, v[0], back * v[3]) : v[3];
        }
    }
    STAMP_END
}

// P1 / PX from chunk partials plus per-block partials of
// Np = sum P1, trPXY = sum_i y_i . PX_i, yPy = sum_i P1_i |y_i|^2 over the local rows.
// Always launched with kScalarBlocks workgroups; part[(1..3)*kScalarBlocks + block].
// A workgroup of 1024 threads takes 256 consecutive rows at a time: thread (g, row) adds the chunks of quarter g of the chunk range,
// [g nch / 4, (g + 1) nch / 4), in ascending order -- every load instruction reads a 512-byte run of one chunk plane, the four planes
// are independent chains, so a thread keeps 4 x 4 loads in flight -- and the four quarter sums of a row are combined as
// (q0 + q1) + (q2 + q3): a fixed order.  (Round 2 used one thread per row over all chunks: the 30 chunks of a 6250-row shard were 8
// dependent batches of loads, 9.5 us of pure latency; four threads per row need two.)
// obs.weight != nullptr: the CPD observations of the rows (CPDCorrespondence.estimate + getUncertainty, CPD.scala:36-46,120-128)
// are produced in the same pass -- weight_i = P1_i / (sigma2 lambda), e_i = weight_i (R^T (yhat_i - c - t) - (ref_i - c) - mean_i)
// with yhat_i = y_i + (PX_i / P1_i - y_i); rows overridden by a landmark get weight 0 (GingrAlgorithm.scala:289-292).
// ROWS (round 4): rows per workgroup step, 256 or 64 (4 ROWS threads).  With 256 a shard of 6 250 rows keeps only 25 of the 256
// workgroups -- 25 compute units -- busy reading its 6 MB of partials (9.2 us, a sixth of the rows in three quarters of the full
// cloud's time); 64 rows per workgroup spread the same rows over 98.  Same order of additions per row either way.
template <int ROWS>
__global__ __launch_bounds__(4 * ROWS) void rowstats_reduce_kernel(const double *__restrict__ partial, int nchunks, Cloud fit,
                                                                   double *__restrict__ P1, double *__restrict__ PX,
                                                                   double *__restrict__ part, CpdObsArgs obs) {
    __shared__ double sh[ROWS];
    __shared__ double quart[3][4][ROWS];  // [quarter 1..3][plane][row]
    const int64_t M = fit.n;
    const int row = threadIdx.x % ROWS, g = threadIdx.x / ROWS;
    const int c0 = (int)((int64_t)g * nchunks / 4), c1 = (int)((int64_t)(g + 1) * nchunks / 4);
    double np = 0.0, tr = 0.0, ypy = 0.0;
    for (int64_t i0 = (int64_t)blockIdx.x * ROWS; i0 < M; i0 += (int64_t)kScalarBlocks * ROWS) {
        const int64_t i = i0 + row;
        const bool ok = i < M;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        double yx = 0.0, yy = 0.0, yz = 0.0, rf[3] = {0.0, 0.0, 0.0}, mn[3] = {0.0, 0.0, 0.0};
        int masked = 0;
        if (ok) {
            if (g == 0) {  // what the finishing thread of the row needs besides the sums: requested together with them
                yx = fit.x[i];
                yy = fit.y[i];
                yz = fit.z[i];
                if (obs.weight) {
                    masked = obs.lm_mask ? obs.lm_mask[i] : 0;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        rf[d] = obs.ref[d * M + i];
                        mn[d] = obs.mean[d * M + i];
                    }
                }
            }
            const double *b = partial + i;
#pragma unroll 4
            for (int c = c0; c < c1; ++c) {
                const double *bc = b + (int64_t)c * 4 * M;
                v[0] += bc[0];
                v[1] += bc[M];
                v[2] += bc[2 * M];
                v[3] += bc[3 * M];
            }
        }
        if (g > 0) {
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) quart[g - 1][pl][row] = v[pl];
        }
        __syncthreads();
        if (g == 0 && ok) {
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) v[pl] = (v[pl] + quart[0][pl][row]) + (quart[1][pl][row] + quart[2][pl][row]);
            P1[i] = v[0];
            PX[i] = v[1];
            PX[M + i] = v[2];
            PX[2 * M + i] = v[3];
            if (obs.weight) {
                if (masked) {
                    obs.weight[i] = 0.0;
                    obs.evec[i] = obs.evec[M + i] = obs.evec[2 * M + i] = 0.0;
                } else {
                    const double p1inv = 1.0 / v[0];                                                  // CPD.scala:37
                    const double ox = yx + (v[1] * p1inv - yx), oy = yy + (v[2] * p1inv - yy), oz = yz + (v[3] * p1inv - yz);
                    const double wgt = 1.0 / (obs.sigma2[0] * obs.lambda * p1inv);                     // CPD.scala:126
                    const double *R = obs.R;
                    const double dx = ox - obs.center[0] - obs.t[0], dy = oy - obs.center[1] - obs.t[1], dz = oz - obs.center[2] - obs.t[2];
                    const double ex = R[0] * dx + R[3] * dy + R[6] * dz - (rf[0] - obs.center[0]) - mn[0];
                    const double ey = R[1] * dx + R[4] * dy + R[7] * dz - (rf[1] - obs.center[1]) - mn[1];
                    const double ez = R[2] * dx + R[5] * dy + R[8] * dz - (rf[2] - obs.center[2]) - mn[2];
                    obs.weight[i] = wgt;
                    obs.evec[i] = wgt * ex;
                    obs.evec[M + i] = wgt * ey;
                    obs.evec[2 * M + i] = wgt * ez;
                }
            }
            np += v[0];
            tr += yx * v[1] + yy * v[2] + yz * v[3];
            ypy += v[0] * (yx * yx + yy * yy + yz * yz);
        }
        __syncthreads();  // quart is rewritten by the next group of rows
    }
    // the scalar partials of the block: only the ROWS finishing threads hold values
    double tot[3] = {0.0, 0.0, 0.0};
    const double vals[3] = {np, tr, ypy};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (g == 0) sh[row] = vals[q];
        __syncthreads();
#pragma unroll
        for (int st = ROWS / 2; st > 0; st >>= 1) {
            if (g == 0 && row < st) sh[row] += sh[row + st];
            __syncthreads();
        }
        tot[q] = sh[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[kScalarBlocks + blockIdx.x] = tot[0];
        part[2 * kScalarBlocks + blockIdx.x] = tot[1];
        part[3 * kScalarBlocks + blockIdx.x] = tot[2];
    }
}
__global__ __launch_bounds__(256) void cpd_scalars_finish_kernel(const double *__restrict__ part, double *__restrict__ scalars,
                                                                 double *__restrict__ xch8, int contribute_xpx) {
    __shared__ double sh[256];
    const int map[4] = {1, 0, 2, 3};  // part slot -> scalar index
    for (int q = 0; q < 4; ++q) {
        const double tot = block_sum<256>(part[q * kScalarBlocks + threadIdx.x], sh);
        if (threadIdx.x == 0) {
            scalars[map[q]] = tot;
            // xPx is a sum over ALL targets, computed on every shard: only one of them may contribute it
            if (xch8) xch8[map[q]] = (map[q] == 1 && !contribute_xpx) ? 0.0 : tot;
        }
        __syncthreads();
    }
    if (xch8 && threadIdx.x >= 4 && threadIdx.x < 8) xch8[threadIdx.x] = 0.0;
}

// Resident workgroups of the chip for one of the all-pairs kernels (compute units x workgroups per unit), queried once: the
// `resident` of the chunk planner (cpd_plan.h: plan_chunks), which makes a launch come out just under a whole number of rounds.
inline int resident_workgroups(int which /* 0 column sums, 1 row statistics PT = 2, 2 row statistics PT = kPT */) {
    static int cache[3] = {0, 0, 0};
    if (cache[which] > 0) return cache[which];
    int per_cu = 0, dev = 0;
    hipError_t e;
    if (which == 0)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cpd_colsum_kernel<GINGR_PT_DEFAULT, false>, kBlock, 0);
    else if (which == 1)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cpd_rowstats_kernel<2, false>, kBlock, 0);
    else
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cpd_rowstats_kernel<GINGR_PT_DEFAULT, false>, kBlock, 0);
    if (e != hipSuccess || per_cu < 1) per_cu = which == 2 ? 3 : 4;
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    (void)hipGetLastError();
    cache[which] = per_cu * cus;
    return cache[which];
}

// The quarter-tile x slot culling variant (FINE) pays for its longer prologue and per-part slot tests only when the streamed cloud
// is long: measured in the late regime (tools/fine_cull_sweep.sh, sigma2 = 4) it wins 3 % at 50k streamed points, 1 % at 30k and
// LOSES 4 % at 15k, 8 % at 1.6k (femur) -- bit-identical results either way.
constexpr int64_t kFineMinStream = 24576;

// one variant, picked from the regime the device last reported (stale at worst: the results are the same)
inline bool fine_variant(const gingr_ctx *ctx, const double *boxes, int64_t stream_len) {
    return boxes && (ctx->fine_override >= 0 ? ctx->fine_override != 0
                                             : (stream_len >= kFineMinStream && ctx->regime_host &&
                                                *(volatile int32_t *)ctx->regime_host != 0));
}

inline int colsum_resident() { return resident_workgroups(0); }
inline int rowstats_resident(int64_t M, int64_t N) { return resident_workgroups(rowstats_pt(M, N) == 2 ? 1 : 2); }

}  // namespace

int64_t cpd_colsum_ws_doubles(int64_t M, int64_t N) { return colsum_ws_doubles(M, N, colsum_resident()); }
int cpd_colsum_chunks(int64_t M, int64_t N) { return colsum_plan(M, N, 0, colsum_resident()).nch; }
int64_t cpd_rowstats_ws_doubles(int64_t M, int64_t N) { return rowstats_ws_doubles(M, N, rowstats_resident(M, N)); }

int launch_cpd_colsum(gingr_ctx *ctx, Cloud fit, Cloud target, const double *sigma2_dev, const double *aux,
                      const double *fit_boxes, double *ws, double *den_partial, int forced_chunks) {
    const PairPlan pp = colsum_plan(fit.n, target.n, forced_chunks, colsum_resident());
    {
        TimerScope ts(ctx, 0);
        dim3 grid((unsigned)ceil_div(target.n, 64 * pp.pt), (unsigned)pp.nch);
        const double *boxes = ctx->cull ? fit_boxes : (const double *)nullptr;
        const bool fine = fine_variant(ctx, boxes, fit.n);
        int32_t *regime_out = boxes ? ctx->regime_dev : (int32_t *)nullptr;
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, ctx->stream, fit, target, sigma2_dev, aux, boxes, pp.plan, ws, regime_out);
        };
        if (pp.pt == 1)
            launch(cpd_colsum_kernel<1, false>);
        else if (pp.pt == 2)  // (small clouds never take the quarter-tile culling variant: kFineMinStream)
            launch(cpd_colsum_kernel<2, false>);
        else if (fine)
            launch(cpd_colsum_kernel<kPT, true>);
        else
            launch(cpd_colsum_kernel<kPT, false>);
    }
    if (den_partial)  // nullptr: the caller adds the chunk partials up itself (launch_cpd_den_finalize with the returned count)
        hipLaunchKernelGGL(chunk_reduce_kernel, dim3((unsigned)ceil_div(target.n, 256)), dim3(256), 0, ctx->stream, ws, pp.nch,
                           target.n, den_partial);
    return pp.nch;
}

void launch_cpd_den_finalize(gingr_ctx *ctx, Cloud target, const double *sigma2_dev, double w, int64_t M_total,
                             double *den, double *inv_den, double *Pt1, int32_t *tile_bad, double *part,
                             double *scalars_dev, const double *chunk_partial, int nchunks) {
    hipLaunchKernelGGL(cpd_den_finalize_kernel, dim3(kScalarBlocks), dim3(256), 0, ctx->stream, target, sigma2_dev, w,
                       (double)M_total / (double)target.n, den, inv_den, Pt1, tile_bad, part, scalars_dev, chunk_partial, nchunks);
}

void launch_cpd_rowstats(gingr_ctx *ctx, Cloud fit, Cloud target, const double *sigma2_dev, const double *aux,
                         const double *inv_den, const double *tgt_boxes, const int32_t *tile_bad, double *ws, double *P1,
                         double *PX_soa, double *part, double *scalars_dev, double *xch8, int contribute_xpx,
                         const CpdObsArgs *obs, bool finish_scalars) {
    const PairPlan pp = rowstats_plan(fit.n, target.n, rowstats_resident(fit.n, target.n));
    {
        TimerScope ts(ctx, 1);
        dim3 grid((unsigned)ceil_div(fit.n, 64 * pp.pt), (unsigned)pp.nch);
        const bool cull = ctx->cull && tgt_boxes && tile_bad;
        const double *boxes = cull ? tgt_boxes : (const double *)nullptr;
        const bool fine = fine_variant(ctx, boxes, target.n);
        int32_t *regime_out = boxes ? ctx->regime_dev : (int32_t *)nullptr;
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, ctx->stream, fit, target, sigma2_dev, aux, inv_den, boxes, tile_bad,
                               pp.plan, ws, regime_out);
        };
        if (pp.pt == 1) {
            launch(cpd_rowstats_kernel<1, false>);
        } else if (pp.pt == 2) {
            if (fine)
                launch(cpd_rowstats_kernel<2, true>);
            else
                launch(cpd_rowstats_kernel<2, false>);
        } else {
            if (fine)
                launch(cpd_rowstats_kernel<kPT, true>);
            else
                launch(cpd_rowstats_kernel<kPT, false>);
        }
    }
    CpdObsArgs none;
    memset(&none, 0, sizeof(none));
    if (fit.n <= (int64_t)kScalarBlocks * 64)  // up to 16 384 rows: a quarter of the rows per workgroup, four times the workgroups
        hipLaunchKernelGGL(rowstats_reduce_kernel<64>, dim3(kScalarBlocks), dim3(256), 0, ctx->stream, ws, pp.nch, fit, P1, PX_soa, part,
                           obs ? *obs : none);
    else
        hipLaunchKernelGGL(rowstats_reduce_kernel<256>, dim3(kScalarBlocks), dim3(1024), 0, ctx->stream, ws, pp.nch, fit, P1, PX_soa, part,
                           obs ? *obs : none);
    if (finish_scalars)  // otherwise the caller's phase-1 finalize kernel sums the block partials (cpd_scalar_partials_layout)
        hipLaunchKernelGGL(cpd_scalars_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, part, scalars_dev, xch8, contribute_xpx);
}

#ifdef GINGR_STAMPS
// diagnostic build only (not in include/gingr_hip.h): allocate / read back the stamp buffer of the two pair loops
extern "C" int gingr_debug_stamps_enable(gingr_ctx *ctx) {
    unsigned long long *buf = nullptr;
    const size_t bytes = (size_t)2 * kStampWaves * 8 * sizeof(unsigned long long);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&buf), bytes));
    HIP_TRY(ctx, hipMemset(buf, 0, bytes));
    HIP_TRY(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf)));
    return GINGR_OK;
}
extern "C" int gingr_debug_stamps_read(gingr_ctx *ctx, unsigned long long *host /* [2][32768][8] */) {
    unsigned long long *buf = nullptr;
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpyFromSymbol(&buf, HIP_SYMBOL(g_stamp_buf), sizeof(buf)));
    if (!buf) return gingr_set_error(ctx, GINGR_ERR_STATE, "stamps not enabled");
    HIP_TRY(ctx, hipMemcpy(host, buf, (size_t)2 * kStampWaves * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return GINGR_OK;
}
#endif
