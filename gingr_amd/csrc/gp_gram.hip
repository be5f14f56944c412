// Weighted Gram passes of the GiNGR update for padded rank rp <= 112, their reductions and the downdate (gfx950, MI355X).
//
//   gram_kernel       Q^T L Q of DiscreteLowRankGaussianProcess.regression (G/api/GingrAlgorithm.scala:300) -- the only
//                     GEMM-shaped op of the path; float64 MFMA (v_mfma_f64_16x16x4_f64), split over row slabs
// rp >= 128: gp_wide.hip.
//
// Layout: Q0 is row-major [3M][rp]: the 3 x rp block of one point is contiguous (2.7 KB at r = 100), so one point's
// observation weight, rotation and epilogue touch one contiguous block; rp = rank rounded up to 16 (MFMA tile).
// All reductions across workgroups go through per-block partials combined in a fixed order (bitwise reproducible).
#include "gp.h"
#include "gp_device.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------------------------------------- weighted Gram
// A workgroup of 4 waves computes one 64x64 patch (4x4 MFMA tiles) of G over one slab of rows; the waves interleave
// the 4-row steps of the slab and are summed through LDS in a fixed order.
//   D(16x16) += A(16x4) B(4x16),  A[i][k] = w_row * Q0[row0+k][a0+i],  B[k][j] = Q0[row0+k][b0+j]
// lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]: both are Q0[row0 + (l>>4)][col0 + (l&15)], i.e. four
// 128-byte row segments per load instruction.  D: lane holds col j = l&15, rows i = (l>>4) + 4*reg.
// The next step's fragments are loaded before the current step's 16 MFMAs are issued (software prefetch).
// Generalised for the one-off moment Grams S[d][e] = sum_i Q0[3i+d]^T Q0[3i+e]: logical row L maps to the physical rows
// L*row_stride + offA (A side) and L*row_stride + offB (B side); `full` enumerates all patches instead of pa <= pb.
__global__ __launch_bounds__(256) void gram_kernel(const double *__restrict__ Q0, int64_t rows, int rp,
                                                   const double *__restrict__ weight, int64_t rows_per_slab, int nbp,
                                                   int row_stride, int offA, int offB, int full,
                                                   double *__restrict__ partial) {
    __shared__ double red[16 * 4 * 64];
    int pa = 0, pb = 0;
    if (full) {
        pa = blockIdx.y / nbp;
        pb = blockIdx.y - pa * nbp;
    } else {  // triangular patch index -> (pa <= pb)
        int t = blockIdx.y;
        for (pa = 0; pa < nbp; ++pa) {
            const int cnt = nbp - pa;
            if (t < cnt) {
                pb = pa + t;
                break;
            }
            t -= cnt;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab;
    const int64_t r1 = min(rows, r0 + rows_per_slab);
    v4f64 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0, 0, 0, 0};
    // Column interleave: tile t of the patch holds the columns {p*64 + 4*lane16 + t}, so the four fragment values a lane
    // needs per side are 32 contiguous bytes (two 16-byte loads) instead of four 8-byte loads 128 bytes apart.
    const bool vla = pa * 64 + 4 * cl < rp, vlb = pb * 64 + 4 * cl < rp;  // rp is a multiple of 16: all-or-nothing per lane
    const bool diag = pa == pb && offA == offB;
    typedef double d4 __attribute__((ext_vector_type(4)));
    double ca[4], cb[4];
    auto load = [&](int64_t row, double fa[4], double fb[4]) {
        const int64_t rr = row + kq;
        const bool valid = rr < r1;
        const int64_t rc = valid ? rr : r0;
        const double wv = valid ? (weight ? weight[row_stride == 1 ? rc / 3 : rc] : 1.0) : 0.0;
        d4 vb4 = d4{0, 0, 0, 0};
        if (vlb && valid) vb4 = *reinterpret_cast<const d4 *>(Q0 + (rc * row_stride + offB) * rp + pb * 64 + 4 * cl);
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[t] = vb4[t];
        if (diag) {
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = fb[t] * wv;
        } else {
            d4 va4 = d4{0, 0, 0, 0};
            if (vla && valid) va4 = *reinterpret_cast<const d4 *>(Q0 + (rc * row_stride + offA) * rp + pa * 64 + 4 * cl);
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = va4[t] * wv;
        }
    };
    int64_t row = r0 + 4 * wave;
    if (row < r1) load(row, ca, cb);
    for (; row < r1; row += 16) {
        double na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
        if (row + 16 < r1) load(row + 16, na, nb);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[i], cb[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ca[t] = na[t];
            cb[t] = nb[t];
        }
    }
    // waves 1..3 are added into wave 0 in order
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) red[((i * 4 + j) * 4 + reg) * 64 + lane] = acc[i][j][reg];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[i][j][reg] += red[((i * 4 + j) * 4 + reg) * 64 + lane];
        }
    }
    if (wave != 0) return;
    double *out = partial + (int64_t)blockIdx.x * rp * rp;
    // D[i_row][j_col]: i_row = kq + 4*reg is the A-side lane index, j_col = cl the B-side lane index
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = pa * 64 + 4 * (kq + 4 * reg) + i;
                const int gj = pb * 64 + 4 * cl + j;
                if (gi < rp && gj < rp) out[(int64_t)gi * rp + gj] = acc[i][j][reg];
            }
        }
}

// Weighted Gram for rp <= 112 (NT = rp / 16 <= 7 column tiles): a PAIR of waves keeps the whole upper triangle of G -- the
// NT (NT + 1) / 2 accumulator tiles are dealt alternately to the two waves (14 + 14 at NT = 7) -- so a 4-row step needs NT fragment
// loads per wave for half of NT (NT + 1) / 2 MFMAs (7 : 14 instead of 8 : 16 for the 64 x 64 patches, and twice per pair), no
// padded tile is ever multiplied and the symmetric half is never computed.  A = w * fragment, B = fragment: one load serves both
// operands.  Eight waves per workgroup = four K groups (they interleave the 4-row steps of the slab) x two tile halves, two waves
// per SIMD: 112 accumulator registers per wave stay in VGPRs.  (One wave holding all 28 tiles needs the AGPR half of the file and
// the compiler then copies all 224 accumulator registers to and from it in every step: 85 us at 50k points instead of 59 us.)
// The K groups are summed through LDS in a fixed order.  Same fragment layout and output layout as gram_kernel.
// upper-triangle tile q (row-major over t <= u) -> (t, u)
template <int NT>
__host__ __device__ constexpr int tri_row(int q) {
    int t = 0;
    while (q >= NT - t) q -= NT - t, ++t;
    return t;
}
template <int NT>
__host__ __device__ constexpr int tri_col(int q) {
    int t = 0;
    while (q >= NT - t) q -= NT - t, ++t;
    return t + q;
}

// RPP: basis rows per point -- 3 (Q0: the weight / evec index of a row is row / 3, the plane row % 3) or 1 (a plane of the compact basis
// Qc, gp.h: one row per point, weight and evec indexed by the row itself; evec points at the plane's own part)
template <int NT, int HALF, bool FULL, int RPP>
__device__ __forceinline__ void gram_tri_half(const double *__restrict__ Q0, int rp, const double *__restrict__ weight, int64_t r0,
                                              int64_t r1, int kgroup, int kq, int cl, int lane, double *red, double *xchg,
                                              double *__restrict__ out, const double *__restrict__ evec, int64_t npts,
                                              double *__restrict__ rhs_out, double *rsh) {
    constexpr int kTiles = NT * (NT + 1) / 2;
    constexpr int kMine = HALF == 0 ? (kTiles + 1) / 2 : kTiles / 2;
    constexpr int kM = kMine > 0 ? kMine : 1;
    v4f64 acc[kM];
#pragma unroll
    for (int q = 0; q < kMine; ++q) acc[q] = v4f64{0, 0, 0, 0};
    // The two waves of a K group need the SAME NT fragments of every 4-row step.  Each loads only every other one (HALF 0: tiles
    // 0, 2, 4, ...; HALF 1: 1, 3, 5, ...) and the pair exchanges them through LDS -- loading all of them in both waves fetched every
    // basis row twice from the fabric (PMC FETCH_SIZE 221 MB for 134 MB of basis at 50k points, rank 100: the second request for
    // a line arrives while the first is still in flight and is not merged).
    //
    // What bounds this loop (tools/ubench_mfma_f64_fill.hip, profiles/r03_ubench_mfma_f64_fill.txt): while a float64 MFMA runs, its
    // SIMD issues NO other vector instruction -- integer, move or float64, from either wave; each one adds its full issue time to
    // the MFMA stream (2.3-5.2 ns), whereas LDS traffic, the barrier and most of a global load's issue are free beside it.  So the
    // time of a step is (28 MFMAs of the SIMD's two waves) + (every VALU instruction of both waves), wherever those are placed,
    // and the loop is built to issue as few as possible:
    //   * the PRODUCER of a fragment scales it (w * fragment, the A operand) and adds it to the right-hand side; both forms go
    //     through LDS, the consumers read 2 NT values and multiply nothing;
    //   * addresses advance incrementally (16 rows per step: pointer += 16 rp, point index += 5 or 6); the from-scratch form (64-bit
    //     multiplies, a division by 3) cost ~45 instructions per step and wave;
    //   * rows past the slab are handled on a wave-uniform slow path (last step of the last slab, prefetches past the end), the
    //     fast path has no selects;
    //   * two operand sets (cur, a) and two prefetch slots alternate, the loop is unrolled by two instead of moving registers.
    // The hand-over of step s+1 is issued between the MFMAs of step s (its latencies hide there); global loads run two steps ahead.
    constexpr int kOwn = HALF == 0 ? (NT + 1) / 2 : NT / 2;  // fragments this wave loads
    constexpr int kO = kOwn > 0 ? kOwn : 1;
    // evec != nullptr: the right-hand side Q0^T evec rides along (each wave for the fragments it loads).  evec: SoA planes [3][npts].
    const bool with_rhs = evec != nullptr;
    const bool with_w = weight != nullptr;
    const int kgu = __builtin_amdgcn_readfirstlane(kgroup);
    const int64_t ubase = r0 + 4 * kgu;       // wave-uniform: row of lane group kq = 0 in step 0; 16 rows further per step
    const int64_t first = ubase + kq;
    const double *pclamp = Q0 + r0 * rp + cl;  // rows past the slab read row r0 (finite); the consumer sets their w and e to 0
    const double *pnext = Q0 + first * rp + cl;
    const int64_t pstep = 16 * (int64_t)rp;
    int64_t left_u = r1 - ubase;  // wave-uniform: rows from the first row of the next step to load to the slab's end
    // row -> (point, coordinate) = (row / 3, row % 3); 16 rows further: (point + 5, coordinate + 1) or (point + 6, coordinate - 2).
    // `third` = coordinate * ceil(2^32 / 3): adding ceil(2^32 / 3) carries exactly when the coordinate wraps (the excess of 2 per
    // wrap stays below the margin for 7e8 wraps).  evec is SoA [3][npts]: entry (coordinate, point).
    const int64_t pt_first = first / RPP;
    const int rem_first = (int)(first - RPP * pt_first);
    constexpr unsigned kThird = 0x55555556u;
    unsigned third = (unsigned)rem_first * kThird;
    const double *wclamp = with_w ? weight + r0 / RPP : pclamp;
    const double *eclamp = with_rhs ? evec + r0 / RPP : pclamp;
    const double *wp = with_w ? weight + pt_first : pclamp;  // without weights / evec: any readable address, the value is not used
    const double *ep = with_rhs ? evec + rem_first * npts + pt_first : pclamp;
    const int64_t estep = with_rhs ? 5 + npts : 0, ewrap = with_rhs ? 6 - 2 * npts : 0;
    double fn[2][kO], wn[2], en[2];
    int vrows[2];  // wave-uniform, per prefetch slot: how many of the step's four rows are inside the slab (4 = all)
    // Both paths issue the same loads in the same order, and nothing touches the loaded values here: the waits at the consumer stay
    // counted (vmcnt(n) leaves the younger slot in flight).
    auto load_next = [&](auto slot) __attribute__((always_inline)) {
        constexpr int L = decltype(slot)::value;
        if (left_u >= 4) {  // wave-uniform: all four rows of the step inside the slab
            vrows[L] = 4;
#pragma unroll
            for (int k = 0; k < kOwn; ++k) fn[L][k] = pnext[16 * (2 * k + HALF)];
            wn[L] = *wp;
            en[L] = *ep;
        } else {  // rows past the slab (last step of the last slab, prefetches past the end): clamped addresses
            vrows[L] = (int)max((int64_t)0, left_u);
            const bool valid = left_u > kq;
            const double *p = valid ? pnext : pclamp;
#pragma unroll
            for (int k = 0; k < kOwn; ++k) fn[L][k] = p[16 * (2 * k + HALF)];
            wn[L] = *(valid ? wp : wclamp);
            en[L] = *(valid ? ep : eclamp);
        }
        left_u -= 16;
        pnext += pstep;
        if constexpr (RPP == 1) {
            wp += 16;
            ep += 16;
        } else {
            const unsigned t2 = third + kThird;
            const bool wrap = t2 < third;
            third = t2;
            wp += wrap ? 6 : 5;
            ep += wrap ? ewrap : estep;
        }
    };
    double racc[kO];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) racc[k] = 0.0;
    // every wave of the workgroup runs the same number of steps (the barrier inside is workgroup wide): the K group with the
    // most rows sets it; steps past a wave's own rows multiply zeros (w = 0, clamped addresses)
    const int64_t nsteps = (r1 - r0 + 15) / 16;
    constexpr int kBufStride = 4 * 2 * NT * 64;  // xchg: [2 buffers][4 K groups][plain, scaled][NT][64 lanes]
    double *xbuf = xchg + (size_t)kgu * 2 * NT * 64 + lane;
    double cur[2][NT], a[2][NT];
    auto hand_over_write = [&](auto slot) __attribute__((always_inline)) {  // fragments of slot L go to buffer L (step parity = slot = buffer)
        constexpr int L = decltype(slot)::value;
        double w = wn[L], e = en[L];
        if constexpr (!FULL) {  // without weights / evec the loads above read a placeholder
            w = with_w ? w : 1.0;
            e = with_rhs ? e : 0.0;
        }
        if (vrows[L] < 4) {  // wave-uniform
            asm volatile("; rows past the slab");  // (keeps this a scalar branch: as selects it is 5 VALU in every step)
            const bool valid = vrows[L] > kq;
            w = valid ? w : 0.0;
            e = valid ? e : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kOwn; ++k) {
            xbuf[L * kBufStride + (2 * k + HALF) * 64] = fn[L][k];
            xbuf[L * kBufStride + (NT + 2 * k + HALF) * 64] = fn[L][k] * w;
            racc[k] = __builtin_fma(fn[L][k], e, racc[k]);  // e = 0 without evec
        }
    };
    auto hand_over_read = [&](auto set) __attribute__((always_inline)) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            cur[S][t] = xbuf[S * kBufStride + t * 64];
            a[S][t] = xbuf[S * kBufStride + (NT + t) * 64];
        }
    };
    auto mfmas = [&](auto set, auto begin, auto endq) __attribute__((always_inline)) {  // tiles [begin, end) of this wave's share, operands of `set`
        constexpr int S = decltype(set)::value;
        static_for<decltype(begin)::value, decltype(endq)::value>([&](auto m) {
            constexpr int mi = decltype(m)::value, q = 2 * mi + HALF, tr = tri_row<NT>(q), tc = tri_col<NT>(q);
            acc[mi] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[S][tr], cur[S][tc], acc[mi], 0, 0, 0);
        });
    };
    using std::integral_constant;
    constexpr integral_constant<int, 0> c0{};
    constexpr integral_constant<int, 1> c1{};
    constexpr int kQ1 = kMine / 4, kQ2 = kMine / 2, kQ3 = (3 * kMine) / 4;
    // prologue: steps 0 and 1 requested, step 0 through LDS into set 0, step 2 requested
    load_next(c0);
    load_next(c1);
    hand_over_write(c0);
    __syncthreads();
    load_next(c0);
    hand_over_read(c0);
    // one step: the MFMAs of set S with the hand-over of the next step (set T = 1 - S) slotted between them
    auto step = [&](auto set) __attribute__((always_inline)) {
        constexpr int S = decltype(set)::value, T = 1 - S;
        constexpr integral_constant<int, T> other{};
        __builtin_amdgcn_sched_barrier(0);
        mfmas(set, integral_constant<int, 0>{}, integral_constant<int, kQ1>{});
        __builtin_amdgcn_sched_barrier(0);
        hand_over_write(other);  // own fragments of the next step (requested two steps ago)
        __builtin_amdgcn_sched_barrier(0);
        mfmas(set, integral_constant<int, kQ1>{}, integral_constant<int, kQ2>{});
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        load_next(other);  // the step after the next two, into the slot just written out
        hand_over_read(other);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(set, integral_constant<int, kQ2>{}, integral_constant<int, kQ3>{});
        __builtin_amdgcn_sched_barrier(0);
        mfmas(set, integral_constant<int, kQ3>{}, integral_constant<int, kMine>{});
        __builtin_amdgcn_sched_barrier(0);
    };
    // (the step after the last one is handed over too and never multiplied: w = 0 rows, one barrier more, no branch in the loop)
    int64_t st = 0;
    for (; st + 1 < nsteps; st += 2) {
        step(c0);
        step(c1);
    }
    if (st < nsteps) step(c0);
    __syncthreads();  // the exchange buffers are free: slot 1 of the K-group reduction below reuses them
    if (evec) {  // workgroup-uniform.  Right-hand side: lanes of a column (the four kq) first, then the K groups 0..3 in order
#pragma unroll
        for (int k = 0; k < kOwn; ++k) {
            racc[k] += __shfl_xor(racc[k], 16);
            racc[k] += __shfl_xor(racc[k], 32);
        }
        if (kq == 0)
#pragma unroll
            for (int k = 0; k < kOwn; ++k) rsh[kgroup * (NT * 16) + (2 * k + HALF) * 16 + cl] = racc[k];
        __syncthreads();
        if (HALF == 0 && kgroup == 0 && kq == 0)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = t * 16 + cl;
                rhs_out[c] = ((rsh[c] + rsh[NT * 16 + c]) + rsh[2 * NT * 16 + c]) + rsh[3 * NT * 16 + c];
            }
    }
    // K groups: (0 + 2) + (1 + 3), two rounds through LDS (both halves at once, disjoint parts of a slot); slot 1 is the exchange area
    // (1 024 NT doubles >= the 128 NT (NT + 1) (+ 256) of a slot for NT <= 7)
    static_assert(((kTiles + 1) / 2) * 2 * 256 <= 2 * kBufStride, "the exchange area must hold one slot of the K-group reduction");
    double *slot0 = red + HALF * ((kTiles + 1) / 2) * 256, *slot1 = xchg + HALF * ((kTiles + 1) / 2) * 256;
    auto put = [&](double *slot) {
#pragma unroll
        for (int q = 0; q < kMine; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) slot[(q * 4 + reg) * 64 + lane] = acc[q][reg];
    };
    auto add = [&](const double *slot) {
#pragma unroll
        for (int q = 0; q < kMine; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) acc[q][reg] += slot[(q * 4 + reg) * 64 + lane];
    };
    if (kgroup >= 2) put(kgroup == 2 ? slot0 : slot1);
    __syncthreads();
    if (kgroup < 2) add(kgroup == 0 ? slot0 : slot1);
    __syncthreads();
    if (kgroup == 1) put(slot0);
    __syncthreads();
    if (kgroup == 0) add(slot0);
    if (kgroup != 0) return;
    // D[i][j] of tile (t, u): i = kq + 4 reg is the A-side index (column 16 t + i of Q0), j = cl the B-side index
    int q = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = t; u < NT; ++u, ++q)
            if ((q & 1) == HALF)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) out[(int64_t)(16 * t + kq + 4 * reg) * rp + 16 * u + cl] = acc[q >> 1][reg];
}

// FULL: weight and evec are both given (the per-iteration call) -- their loads are unconditional
template <int NT, bool FULL, int RPP = 3>
__global__ __launch_bounds__(512) void gram_tri_kernel(const double *__restrict__ Q0, int64_t rows, int rp,
                                                       const double *__restrict__ weight, int64_t rows_per_slab,
                                                       double *__restrict__ partial, const double *__restrict__ evec, int64_t npts,
                                                       double *__restrict__ rhs_partial, ZeroGate gate) {
    constexpr int kTiles = NT * (NT + 1) / 2;
    if (!gate_open(gate)) return;  // (workgroup-uniform: the downdate launch in front did the work)
    __shared__ double red[(kTiles + 1) * 256];
    __shared__ double xchg[2 * 4 * 2 * NT * 64];
    __shared__ double rsh[4 * NT * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab;
    const int64_t r1 = min(rows, r0 + rows_per_slab);
    double *out = partial + (int64_t)blockIdx.x * rp * rp;
    double *rhs_out = rhs_partial ? rhs_partial + (int64_t)blockIdx.x * rp : nullptr;  // one row of right-hand-side partials per slab
    if constexpr (RPP == 1) {  // plane blockIdx.z of the compact basis; partials [slab][plane][rp * rp + rp], the right-hand side last
        const int d = blockIdx.z;
        Q0 += (int64_t)d * (rows + kCompactRowSlack) * rp;
        evec += (int64_t)d * npts;
        out = partial + ((int64_t)blockIdx.x * 3 + d) * (rp * rp + rp);
        rhs_out = out + rp * rp;
    }
    if ((wave >> 2) == 0)
        gram_tri_half<NT, 0, FULL, RPP>(Q0, rp, weight, r0, r1, wave & 3, kq, cl, lane, red, xchg, out, evec, npts, rhs_out, rsh);
    else
        gram_tri_half<NT, 1, FULL, RPP>(Q0, rp, weight, r0, r1, wave & 3, kq, cl, lane, red, xchg, out, evec, npts, rhs_out, rsh);
}

// G[i][j] = sum over slabs (fixed order): 32 consecutive elements x 8 slab groups per workgroup, so every load instruction
// reads 256-byte runs of one slab; group g adds the slabs g, g+8, ... in ascending order, the groups are combined as
// ((0+1)+(2+3))+((4+5)+(6+7)).  symmetric: only i <= j is read (upper patches) and mirrored; otherwise every element.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double *__restrict__ partial, int nslabs, int rp, int symmetric,
                                                          double *__restrict__ G) {
    __shared__ double sh[8][33];
    const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int idx = blockIdx.x * 32 + el;
    const int rr = rp * rp;
    const int i = idx / rp, j = idx - i * rp;
    const bool need = idx < rr && !(symmetric && i > j);
    double s = 0.0;
    if (need) {
        const double *p = partial + idx;
#pragma unroll 8
        for (int b = g; b < nslabs; b += 8) s += p[(int64_t)b * rr];
    }
    sh[g][el] = s;
    __syncthreads();
    if (g == 0 && need) {
        const double t = ((sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el])) + ((sh[4][el] + sh[5][el]) + (sh[6][el] + sh[7][el]));
        G[i * rp + j] = t;
        if (symmetric) G[j * rp + i] = t;
    }
}

// Everything that turns the partial sums of phase 1 into the shard's exchange segment, in ONE launch (instead of gram_reduce +
// block_partials_reduce + cpd_scalars_finish): workgroups [0, nG) reduce the Gram slab partials exactly like gram_reduce_kernel
// (same grouping, same order), workgroups [nG, nG + rp) the right-hand-side partials of the basis sweep exactly like
// block_partials_reduce_kernel, and the last workgroup the four scalar sums of the CPD passes like cpd_scalars_finish_kernel
// (scalar_mode 1) or just clears the eight scalars (mode 0: ICP).  nslabs == 0: G was produced elsewhere (scaled moment copy).
__global__ __launch_bounds__(256) void phase1_finalize_kernel(Phase1FinalizeArgs A) {
    __shared__ double sh[8][33];
    __shared__ double sv[256];
    const int rp = A.rp, rr = rp * rp;
    const int nG = (A.nslabs > 0 || A.scaled_src) ? (rr + 31) / 32 : 0;
    const int b = blockIdx.x;
    if (A.gate.counts && gate_open(A.gate)) {  // (gate.run_if_many = 1) the weighted pass over the basis ran instead of the downdate
        A.nslabs = A.alt_nslabs;
        A.scaled_src = nullptr;
        A.sweep_blocks = A.alt_nslabs;
    }
    if (b < nG) {
        const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
        const int idx = b * 32 + el;
        if (A.nslabs <= 0) {  // no Gram pass: every row carries the weight 1 / sigma2, G is the model's moment scaled
            if (g == 0 && idx < rr) A.G[idx] = A.scaled_contribute ? A.scaled_src[idx] * (1.0 / A.sigma2[0]) : 0.0;
            return;
        }
        const int i = idx / rp, j = idx - i * rp;
        const bool need = idx < rr && !(i > j);
        double s = 0.0;
        if (A.sep_map) {  // compact partials: entry (i, j) of the dense G is entry (pos i, pos j) of its class's block, or +0.0
            constexpr int64_t kBlock = kCompactCols * kCompactCols + kCompactCols;
            const SepMap sm{rp};
            const int ci = need ? A.sep_map[sm.cls(i)] : -1, cj = need ? A.sep_map[sm.cls(j)] : -1;
            if (ci >= 0 && ci == cj) {  // (class lists are in model order: i <= j gives pos i <= pos j, the upper tiles the pass wrote)
                const double *p = A.gram_partial + ci * kBlock + A.sep_map[sm.pos(i)] * kCompactCols + A.sep_map[sm.pos(j)];
#pragma unroll 8
                for (int q = g; q < A.nslabs; q += 8) s += p[(int64_t)q * 3 * kBlock];
            }
        } else if (need) {
            const double *p = A.gram_partial + idx;
#pragma unroll 8
            for (int q = g; q < A.nslabs; q += 8) s += p[(int64_t)q * rr];
        }
        sh[g][el] = s;
        __syncthreads();
        if (g == 0 && need) {
            double t = ((sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el])) + ((sh[4][el] + sh[5][el]) + (sh[6][el] + sh[7][el]));
            if (A.scaled_src)  // the partials are Q^T Q of the zero-weight rows: the model's moment minus them, every other row at 1 / sigma2
                t = ((A.scaled_contribute ? A.scaled_src[idx] : 0.0) - t) * (1.0 / A.sigma2[0]);
            A.G[i * rp + j] = t;
            A.G[j * rp + i] = t;
        }
        return;
    }
    if (b < nG + rp) {
        const int k = b - nG;
        double s = 0.0;
        if (A.sep_map) {  // behind the Gram block of column k's class, at its position there; padding columns: +0.0
            constexpr int64_t kBlock = kCompactCols * kCompactCols + kCompactCols;
            const SepMap sm{rp};
            const int c = A.sep_map[sm.cls(k)];
            if (c >= 0) {
                const double *p = A.gram_partial + c * kBlock + kCompactCols * kCompactCols + A.sep_map[sm.pos(k)];
                for (int q = threadIdx.x; q < A.nslabs; q += 256) s += p[(int64_t)q * 3 * kBlock];
            }
        } else {
            for (int q = threadIdx.x; q < A.sweep_blocks; q += 256) s += A.sweep_partial[(int64_t)q * rp + k];
        }
        sv[threadIdx.x] = s;
        __syncthreads();
#pragma unroll
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) sv[threadIdx.x] += sv[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) A.rhs[k] = sv[0];
        return;
    }
    // scalars
    if (A.scalar_mode == 1) {
        const int map[4] = {1, 0, 2, 3};  // part slot -> scalar index (cpd_scalars_finish_kernel)
        for (int q = 0; q < 4; ++q) {
            sv[threadIdx.x] = A.part[q * GINGR_SCALAR_BLOCKS + threadIdx.x];
            __syncthreads();
#pragma unroll
            for (int st = 128; st > 0; st >>= 1) {
                if ((int)threadIdx.x < st) sv[threadIdx.x] += sv[threadIdx.x + st];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                const double tot = sv[0];
                if (A.scalars_local) A.scalars_local[map[q]] = tot;
                // xPx is a sum over ALL targets, computed on every shard: only one of them may contribute it
                A.sc8[map[q]] = (map[q] == 1 && !A.contribute_xpx) ? 0.0 : tot;
            }
            __syncthreads();
        }
        if (threadIdx.x >= 4 && threadIdx.x < 8) A.sc8[threadIdx.x] = 0.0;
    } else if (threadIdx.x < 8) {
        A.sc8[threadIdx.x] = 0.0;
    }
}

// Q^T Q of the vertices whose weight is exactly 0, slab by slab (launch_gram_downdate).  A workgroup owns the whole rp x rp matrix:
// thread (ti, tj) of a 16 x 16 arrangement keeps the entries (ti + 16 a, tj + 16 b), a, b < 7, in registers.  It walks its slab's
// vertices 256 at a time -- a ballot finds the zero-weight ones -- and adds, for each of them in ascending order, the three rows of the
// basis (staged in LDS four vertices at a time: 14 reads per row and thread) as outer products: fixed order, no atomics.
__global__ __launch_bounds__(256) void gram_downdate_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ weight,
                                                            int64_t verts_per_slab, double *__restrict__ partial, ZeroGate gate) {
    if (!gate_open(gate)) return;  // (workgroup-uniform: too many zero-weight rows, the pass over the basis behind this launch runs)
    constexpr int kBatch = 4;  // zero-weight vertices staged together: their rows are requested at once (a slab with several of them
                               // would otherwise pay one memory round trip per vertex, and the launch ends with its slowest slab)
    // Ranks above 112 (round 6): the matrix is cut into 112-column patches and blockIdx.y picks one of the upper ones (pa <= pb); a
    // workgroup then keeps the 7 x 7 entries per thread of ITS patch and stages the two column ranges of the rows.  One patch for
    // rp <= 112: the code (and the bits) of round 5.
    int pa = 0, pb = 0;
    {
        const int np = (rp + 111) / 112;
        int t = blockIdx.y;
        for (pa = 0; pa < np; ++pa) {
            if (t < np - pa) {
                pb = pa + t;
                break;
            }
            t -= np - pa;
        }
    }
    const int ca0 = 112 * pa, cb0 = 112 * pb;
    __shared__ double q[kBatch][3][112], qb[kBatch][3][112];
    __shared__ unsigned long long zmask[16];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;  // (tj fastest: the sixteen lanes of a row write 128 contiguous bytes)
    const int64_t v0 = (int64_t)blockIdx.x * verts_per_slab, v1 = v0 + verts_per_slab < M ? v0 + verts_per_slab : M;
    double acc[7][7];
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = 0; b < 7; ++b) acc[a][b] = 0.0;
    constexpr int kRounds = 4;  // 1 024 vertices per pass: their weights are requested together (one memory round trip, not four)
    for (int64_t base = v0; base < v1; base += 256 * kRounds) {
        double wv[kRounds];
#pragma unroll
        for (int r2 = 0; r2 < kRounds; ++r2) {
            const int64_t v = base + 256 * r2 + tid;
            wv[r2] = v < v1 ? weight[v] : 1.0;
        }
        __syncthreads();  // (the previous pass's readers of zmask are done)
#pragma unroll
        for (int r2 = 0; r2 < kRounds; ++r2) {
            const unsigned long long m = __ballot(wv[r2] == 0.0);
            if ((tid & 63) == 0) zmask[4 * r2 + (tid >> 6)] = m;
        }
        __syncthreads();
        // the mask words are walked in scalar registers (workgroup-uniform: a dynamically indexed per-lane copy of the sixteen words
        // would be a chain of selects per access -- it was most of this kernel's time)
        auto word = [&](int k) {
            const unsigned long long v = zmask[k];
            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
            return ((unsigned long long)hi << 32) | (unsigned long long)lo;
        };
        int w = 0;
        unsigned long long cur = word(0);
        for (;;) {
            int64_t vz[kBatch];
            int nb = 0;
            while (nb < kBatch) {  // the next (up to) kBatch zero-weight vertices, ascending
                if (cur == 0) {
                    if (++w >= 4 * kRounds) break;
                    cur = word(w);
                    continue;
                }
                vz[nb++] = base + 64 * w + __builtin_ctzll(cur);
                cur &= cur - 1;
            }
            if (nb == 0) break;
            __syncthreads();  // (the previous batch's rows have been used)
            for (int t = tid; t < kBatch * 3 * 112; t += 256) {
                const int s2 = t / (3 * 112), r2 = t - s2 * (3 * 112), d = r2 / 112, k = r2 - 112 * d;
                if (s2 < nb) {
                    const double *row = Q0 + (3 * vz[s2] + d) * (int64_t)rp;
                    q[s2][d][k] = ca0 + k < rp ? row[ca0 + k] : 0.0;
                    if (pb != pa) qb[s2][d][k] = cb0 + k < rp ? row[cb0 + k] : 0.0;
                }
            }
            __syncthreads();
            const double(*qcol)[3][112] = pb != pa ? qb : q;  // (workgroup-uniform)
            for (int s2 = 0; s2 < nb; ++s2) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double qi[7], qj[7];
#pragma unroll
                    for (int a = 0; a < 7; ++a) qi[a] = q[s2][d][ti + 16 * a], qj[a] = qcol[s2][d][tj + 16 * a];
#pragma unroll
                    for (int a = 0; a < 7; ++a)
#pragma unroll
                        for (int b = 0; b < 7; ++b) acc[a][b] = __builtin_fma(qi[a], qj[b], acc[a][b]);
                }
            }
        }
    }
    double *out = partial + (int64_t)blockIdx.x * rp * rp;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            const int i = ca0 + ti + 16 * a, j = cb0 + tj + 16 * b;
            if (i < rp && j < rp) out[i * rp + j] = acc[a][b];
        }
}

}  // namespace

static void gram_plan(int64_t M, int32_t rp, int *nbp, int *npatch, int *nslabs, int64_t *rows_per_slab) {
    const int64_t rows = 3 * M;
    *nbp = (rp + 63) / 64;
    *npatch = *nbp * (*nbp + 1) / 2;
    int64_t want = 768 / *npatch;  // ~3 workgroups of 4 waves per CU
    if (want < 1) want = 1;
    // a slab writes a full rp x rp partial: below ~256 rows per slab the partials cost more than the rows they summarise
    const int64_t max_slabs = ceil_div(rows, 256);
    if (want > max_slabs) want = max_slabs;
    if (want < 1) want = 1;
    *rows_per_slab = round_up(ceil_div(rows, want), 16);
    *nslabs = (int)ceil_div(rows, *rows_per_slab);
}

// slabs of gram_tri_kernel (one workgroup each): 256 = one per CU; small shards keep at least 64 rows per slab
static void gram_tri_plan(int64_t M, int *nslabs, int64_t *rows_per_slab) {
    const int64_t rows = 3 * M;
    const int64_t want = std::min<int64_t>(256, std::max<int64_t>(1, ceil_div(rows, 64)));
    *rows_per_slab = round_up(ceil_div(rows, want), 16);
    *nslabs = (int)ceil_div(rows, *rows_per_slab);
}

int64_t gram_ws_doubles(int64_t M, int32_t rp) {
    int nbp, npatch, nslabs, nslabs_tri;
    int64_t rps;
    gram_plan(M, rp, &nbp, &npatch, &nslabs, &rps);
    gram_tri_plan(M, &nslabs_tri, &rps);
    const int64_t n = (int64_t)std::max(nslabs, nslabs_tri) * rp * rp;
    return rp >= 128 ? std::max(n, gram_wide_ws_doubles(M, rp)) : n;
}

int launch_gram(gingr_ctx *ctx, const double *Q0, int64_t M, int32_t rp, const double *weight, double *ws, double *G, const double *evec,
                double *rhs_partial, bool *rhs_done, const ZeroGate *gate) {
    if (rhs_done) *rhs_done = false;
    int nbp, npatch, nslabs;
    int64_t rps;
    gram_plan(M, rp, &nbp, &npatch, &nslabs, &rps);
    {
        const int nt = rp / 16;
        if (nt <= 7) {
            TimerScope ts(ctx, 2);
            // whole upper triangle per wave: one workgroup per slab; ~3 slabs' worth of waves per SIMD is not needed (one wave per
            // SIMD, deep prefetch), so 256 slabs = one workgroup per CU
            gram_tri_plan(M, &nslabs, &rps);
            const bool fuse = evec && rhs_partial && rhs_done;  // Q0^T evec out of the same pass: [nslabs][rp] partials
            if (fuse) *rhs_done = true;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(nslabs), dim3(512), 0, ctx->stream, Q0, 3 * M, (int)rp, weight, rps, ws,
                                   fuse ? evec : (const double *)nullptr, M, fuse ? rhs_partial : (double *)nullptr, gate ? *gate : ZeroGate{});
            };
            const bool full = fuse && weight;
#define GINGR_GRAM_TRI(n) \
    case n: \
        if (full) go(gram_tri_kernel<n, true>); \
        else go(gram_tri_kernel<n, false>); \
        break;
            switch (nt) {
                GINGR_GRAM_TRI(1)
                GINGR_GRAM_TRI(2)
                GINGR_GRAM_TRI(3)
                GINGR_GRAM_TRI(4)
                GINGR_GRAM_TRI(5)
                GINGR_GRAM_TRI(6)
                default:
                    if (full) go(gram_tri_kernel<7, true>);
                    else go(gram_tri_kernel<7, false>);
                    break;
            }
#undef GINGR_GRAM_TRI
        } else {
            // rp >= 128: eight waves share the triangle (gp_wide.hip); the right-hand side rides along whenever it is asked for
            const bool fuse = evec && rhs_partial && rhs_done;
            if (fuse) *rhs_done = true;
            nslabs = launch_gram_wide(ctx, Q0, M, rp, weight, ws, fuse ? evec : nullptr, fuse ? rhs_partial : nullptr, gate);
        }
    }
    if (G)  // nullptr: the caller reduces the slab partials itself (launch_phase1_finalize with the returned slab count)
        hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp, 32)), dim3(256), 0, ctx->stream, ws,
                           nslabs, (int)rp, 1, G);
    return nslabs;
}

// slabs of the compact pass, per plane: two workgroups per CU over the three planes (a wave has three tiles of work per step, far less
// than the seven-tile pass, so one workgroup per CU would leave the memory system idle); small models keep at least 64 rows per slab
static void gram_compact_plan(int64_t M, int *nslabs, int64_t *rows_per_slab) {
    const int64_t want = std::min<int64_t>(170, std::max<int64_t>(1, ceil_div(M, 64)));
    *rows_per_slab = round_up(ceil_div(M, want), 16);
    *nslabs = (int)ceil_div(M, *rows_per_slab);
}

int64_t gram_compact_ws_doubles(int64_t M) {
    int nslabs;
    int64_t rps;
    gram_compact_plan(M, &nslabs, &rps);
    return (int64_t)nslabs * 3 * (kCompactCols * kCompactCols + kCompactCols);
}

int launch_gram_compact(gingr_ctx *ctx, const double *Qc, int64_t M, const double *weight, const double *evec, double *ws) {
    int nslabs;
    int64_t rps;
    gram_compact_plan(M, &nslabs, &rps);
    TimerScope ts(ctx, 2);
    hipLaunchKernelGGL((gram_tri_kernel<kCompactCols / 16, true, 1>), dim3(nslabs, 1, 3), dim3(512), 0, ctx->stream, Qc, M, (int)kCompactCols,
                       weight, rps, ws, evec, M, (double *)nullptr, ZeroGate{});
    return nslabs;
}

int launch_gram_downdate(gingr_ctx *ctx, const double *Q0, int64_t M, int32_t rp, const double *weight, double *ws, const ZeroGate *gate) {
    int nslabs_tri;  // never more slabs than the weighted Gram pass would write: the workspace behind them belongs to the right-hand-side sweep
    int64_t rows_per_slab;
    gram_tri_plan(M, &nslabs_tri, &rows_per_slab);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min(nslabs_tri, 128), ceil_div(M, 64)));
    const int64_t vps = ceil_div(M, want);
    const int nslabs = (int)ceil_div(M, vps);
    const int np = (rp + 111) / 112;  // 112-column patches; the upper ones only
    hipLaunchKernelGGL(gram_downdate_kernel, dim3((unsigned)nslabs, (unsigned)(np * (np + 1) / 2)), dim3(256), 0, ctx->stream, Q0, M, (int)rp, weight,
                       vps, ws, gate ? *gate : ZeroGate{});
    return nslabs;
}

void launch_phase1_finalize(gingr_ctx *ctx, const Phase1FinalizeArgs &a) {
    const int nG = (a.nslabs > 0 || a.scaled_src) ? (a.rp * a.rp + 31) / 32 : 0;
    hipLaunchKernelGGL(phase1_finalize_kernel, dim3((unsigned)(nG + a.rp + 1)), dim3(256), 0, ctx->stream, a);
}

namespace {
// S[d][e][a][b] = T[d rp + a][e rp + b], T the (3 rp) x (3 rp) product of the three-rows-per-point view
__global__ __launch_bounds__(256) void moment_scatter_kernel(const double *__restrict__ T, int rp, MomentLayout ml, double *__restrict__ mom) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = 3 * (int64_t)rp;
    if (idx >= w * w) return;
    const int I = (int)(idx / w), J = (int)(idx - (int64_t)I * w);
    const int d = I / rp, a = I - d * rp, e = J / rp, b = J - e * rp;
    mom[ml.S(d, e) + (int64_t)a * rp + b] = T[idx];
}
// out = in^T ([rp][rp])
__global__ __launch_bounds__(256) void transpose_kernel(const double *__restrict__ in, int rp, double *__restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rp * rp) return;
    const int i = idx / rp, j = idx - i * rp;
    out[idx] = in[j * rp + i];
}
bool moments_as_rows(int32_t rp) { return 3 * rp >= 128 && 3 * rp <= 512; }
}  // namespace

int64_t moment_grams_ws_doubles(int64_t M, int32_t rp) {
    if (moments_as_rows(rp)) return gram_rows_ws_doubles(M, 3 * rp) + 9 * (int64_t)rp * rp;
    return gram_ws_doubles(M, rp);
}

// The nine blocks are the blocks of Z^T Z with Z the basis read as M rows of width 3 rp (the rows 3i, 3i+1, 3i+2 of a point are
// contiguous), so for 3 rp in 128 .. 512 (ranks 43 .. 170) they are ONE symmetric product on the triangle kernel of gp_wide.hip
// instead of nine general ones (0.9 ms -> 0.1 ms at rank 100).  Outside that range: the six blocks d <= e by gram_kernel, the other
// three by transposition.
void launch_moment_grams(gingr_ctx *ctx, const double *Q0, int64_t M, int32_t rp, double *ws, double *mom) {
    const MomentLayout ml{rp};
    if (moments_as_rows(rp)) {
        const int32_t w = 3 * rp;
        double *T = ws + gram_rows_ws_doubles(M, w);
        const int nslabs = launch_gram_rows(ctx, Q0, M, w, ws);
        hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)ceil_div((int64_t)w * w, 32)), dim3(256), 0, ctx->stream, ws, nslabs, (int)w, 1, T);
        hipLaunchKernelGGL(moment_scatter_kernel, dim3((unsigned)ceil_div((int64_t)w * w, 256)), dim3(256), 0, ctx->stream, T, (int)rp, ml, mom);
        return;
    }
    // logical rows = points; same slab plan as the weighted Gram (its workspace is large enough: nslabs is capped by rows/64)
    int nbp, npatch, nslabs;
    int64_t rps;
    gram_plan(M, rp, &nbp, &npatch, &nslabs, &rps);
    rps = round_up(ceil_div(M, nslabs), 16);
    nslabs = (int)ceil_div(M, rps);
    for (int d = 0; d < 3; ++d)
        for (int e = d; e < 3; ++e) {
            hipLaunchKernelGGL(gram_kernel, dim3(nslabs, nbp * nbp), dim3(256), 0, ctx->stream, Q0, M, (int)rp, (const double *)nullptr, rps, nbp,
                               3, d, e, 1, ws);
            hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp, 32)), dim3(256), 0, ctx->stream, ws, nslabs, (int)rp, 0,
                               mom + ml.S(d, e));
            if (e > d)
                hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp, 256)), dim3(256), 0, ctx->stream, mom + ml.S(d, e),
                                   (int)rp, mom + ml.S(e, d));
        }
}
