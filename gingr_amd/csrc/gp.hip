// Posterior solves, transition densities and cached samples of the GiNGR update for gfx950 (MI355X).  The other low-rank GP kernels:
// gp_sweep.hip (basis sweeps), gp_gram.hip and gp_wide.hip (weighted Gram), gp_obs.hip (observations), gp_post_solve.hip.
//
//   posterior_solve   pinv(QtL Q + I) * QtL (y - m)  -> Cholesky solve of the SPD matrix I + G: one workgroup on the building blocks
//                     of solve_blocks.h (LDS up to rp = 128, super-panels on a global workspace above), the multi-workgroup
//                     blocked solve of dense_spd.hip from rp = 256 on
#include "dense_spd.h"
#include "gp.h"
#include "solve_blocks.h"

#include <algorithm>

namespace {

// a = (I + G)^-1 rhs; with zrand != nullptr a posterior SAMPLE of the coefficients: a + L^-T z, z ~ N(0, I)
// (Cov = L^-T L^-1 = (I + G)^-1, the posterior covariance of the coefficients: the same distribution as
//  posterior.sample() of scalismo's SVD-parameterised posterior model, G/api/GingrAlgorithm.scala:211).
// The bordered matrix lives in LDS (r <= 128); above that: posterior_solve_wide_kernel or the blocked solve (launch_posterior_solve).

// GW = false: the workspace is the dynamic LDS block and nothing else -- the compiler then proves every access of the building
// blocks to be address space 3 and emits ds_read / ds_write.  (With one kernel choosing between LDS and a global pointer at run
// time every access was a FLAT instruction: ~3x the latency of the LDS path, 64-bit address arithmetic, SGPR spills.)
// The solve on a workspace `sm` (LDS or global, see below); all kSolveThreads threads.  bad_spd / bad: two ints of LDS.
// FAST (LDS-resident, rp <= 112: sixteen more rows fit into the 160 KB): the identity rows of lds_cholesky / lds_backward_w.
// cols != nullptr (FAST, no zrand): the system is one class of a coordinate-separable model -- rows / columns cols[0 .. r) of the dense G
// (row stride ldg) and rhs, padded to n = rp; the coefficients go back to a[cols[k]] (posterior_solve_lds_kernel<2>).
template <bool FAST, typename PtrD>
__device__ __forceinline__ void posterior_solve_body(PtrD sm, int r, int rp, const double *__restrict__ G, const double *__restrict__ rhs,
                                                     const double *__restrict__ zrand, double *__restrict__ a, DevState *__restrict__ st,
                                                     int *bad_spd, int *bad, const int32_t *__restrict__ cols = nullptr, int ldg = 0) {
    const int n = rp, ld = solve_ld(n);
    constexpr int XR = FAST ? 2 * kNB : kNB;
    auto A = sm;
    auto y = sm + (size_t)n * ld;   // row n of the bordered matrix: the right-hand side (rows n+1 .. n+15 are zero)
    auto rd = sm + (size_t)(n + XR) * ld;  // reciprocal diagonal of L
    auto y2 = rd + n;                       // sampling direction
    const int tid = threadIdx.x;
    if (tid == 0) {
        *bad_spd = 0;
        *bad = 0;
    }
    for (int k = tid; k < kNB * ld; k += kSolveThreads) y[k] = k < r ? rhs[cols ? cols[k] : k] : 0.0;
    for (int k = tid; k < n; k += kSolveThreads) y2[k] = (zrand && k < r) ? zrand[k] : 0.0;
    if (FAST)  // rows n+16 .. n+31: the tiled identity
        for (int k = tid; k < kNB * ld; k += kSolveThreads) {
            const int c = k / ld, j = k - c * ld;
            y[kNB * ld + k] = (j < n && (j & 15) == c) ? 1.0 : 0.0;
        }
    // Mm = QtL Q + I     (scalismo genericRegressionComputations)
    GINGR_STAGE_CLOCK(7)
    if (cols)
        lds_load_spd<kSolveThreads, false, kCompactCols / 16>(A, ld, r, n, G, 1.0, nullptr, 0.0, 1.0, cols, ldg);
    else
        lds_load_spd<kSolveThreads>(A, ld, r, n, G, 1.0, nullptr, 0.0, 1.0);
    GINGR_STAGE_CLOCK(0)
    lds_cholesky<kSolveThreads>(A, ld, n, rd, bad_spd, kNB, FAST ? kNB : 0);  // y <- L^-1 y on the way
    GINGR_STAGE_CLOCK(4)
    if constexpr (FAST) {
        // x = L^-T y into rd (the reciprocal diagonal is not needed any more); the sampling direction L^-T z the same way
        if (zrand) {  // (before y: the second call reuses rd for its result, so the first result moves to y2's place afterwards)
            lds_backward_w<kSolveThreads>(A, ld, n, y + kNB * ld, y2, rd);
            for (int k = tid; k < n; k += kSolveThreads) y2[k] = rd[k];
            __syncthreads();
        }
        lds_backward_w<kSolveThreads>(A, ld, n, y + kNB * ld, y, rd);
        for (int k = tid; k < n; k += kSolveThreads) y[k] = rd[k];
        __syncthreads();
    } else {
        lds_backward<kSolveThreads>(A, ld, n, rd, y);
        if (zrand) lds_backward<kSolveThreads>(A, ld, n, rd, y2);
    }
    GINGR_STAGE_CLOCK(5)
    GINGR_STAGE_CLOCK(6)
    for (int k = tid; k < rp; k += kSolveThreads) {
        const double v = k < r ? y[k] + y2[k] : 0.0;
        if (!cols)
            a[k] = v;
        else if (k < r)
            a[cols[k]] = v;
        if (!finite_d(v)) *bad = 1;
    }
    __syncthreads();
    if (tid == 0) {
        if (*bad_spd)
            st->err = GINGR_ERR_NOT_SPD;
        else if (*bad)
            st->err = GINGR_ERR_NONFINITE;
    }
}

// MODE 0: LDS, identity rows (rp <= 112); 1: LDS (rp = 128)
// MODE 2: a coordinate-separable model (gp.h: SepMap): I + G is three uncoupled systems, one per coordinate class.  Workgroup d gathers
// class d's rows and columns of the dense G / rhs, solves the kCompactCols-padded system as MODE 0 does and writes its coefficients to
// their dense positions; the padding of a is cleared by every workgroup.  Each workgroup stores the error code ITS system gives into
// st->err (plain stores, no hand-over): a non-finite weight or observation enters all three blocks, which then store the same code.
struct SepCounts {
    int32_t rc[3];
};
template <int MODE>
__global__ __launch_bounds__(kSolveThreads) void posterior_solve_lds_kernel(int r, int rp, const double *__restrict__ G,
                                                                  const double *__restrict__ rhs,
                                                                  const double *__restrict__ zrand, double *__restrict__ a,
                                                                  DevState *__restrict__ st, const int32_t *__restrict__ sep_map = nullptr,
                                                                  SepCounts sc = SepCounts{}) {
    extern __shared__ double lds_sm[];
    __shared__ int bad_spd, bad;
    if constexpr (MODE == 2) {
        const int d = blockIdx.x;
        for (int k = r + (int)threadIdx.x; k < rp; k += kSolveThreads) a[k] = 0.0;
        if (sc.rc[d] == 0) return;  // (workgroup-uniform) a coordinate without columns: nothing to solve, nothing to write
        posterior_solve_body<true>(lds_sm, sc.rc[d], kCompactCols, G, rhs, nullptr, a, st, &bad_spd, &bad, sep_map + SepMap{rp}.col(d, 0), rp);
        return;
    }
#ifdef GINGR_SOLVE_TWICE  // tools/ubench_solve.hip only: the second pass runs with the kernel's code in the instruction cache
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
#endif
    posterior_solve_body<MODE == 0>(lds_sm, r, rp, G, rhs, zrand, a, st, &bad_spd, &bad);
#ifdef GINGR_SOLVE_TWICE
    }
#endif
}

// ---- ranks above 128: the bordered matrix (n + 16 rows) does not fit the LDS.  One workgroup of eight waves factors it by SUPER-PANELS
// of SW columns, left-looking: for panel k (columns kb .. kb + SW) every 16 x 16 tile of the rows kb .. n + 16 is formed as
//     (I + G)[tile] - L[rows, 0 : kb] L[panel rows, 0 : kb]^T
// on the matrix pipe straight from the factor already written to the global workspace (L2 resident; fragments read as in
// lds_cholesky's tile_update) and lands in LDS, where lds_cholesky factors the SW x SW head and lets the rows below ride along -- the
// same building blocks, the same bordered form (row n carries the right-hand side through the forward substitution).  The panel then
// goes back to the workspace.  The backward substitution walks the panels bottom-up: a mat-vec with the rows below from the
// workspace, lds_backward on the diagonal block.  Until round 5 the LDS kernel ran on the global workspace through flat addressing,
// one 16-column panel at a time: 265 us at r = 256, 1.46 ms at r = 512 (profiles/r06_base_rank256_512_kernel_stats.txt).
constexpr int kWideSolveThreads = 512;

template <int SW>
struct WideSolveLds {
    double rdl[SW];
    double red[2][kWideSolveThreads / 64][SW];
    double xs[2][512];  // x = L^-T y and, when sampling, L^-T z (n <= 512)
    double yv[2][SW];
    int bad_spd;
};

// The body: factor C = ca G + cs S + ci I (identity on the padding r <= i < n) in the workspace gw, with the bordered row
// b1 + cb b2 riding through the forward substitution, then substitute back.  On return Ls.xs[0] = C^-1 (b1 + cb b2), Ls.xs[1] =
// L^-T zrand (zeros without zrand), the factor and its reciprocal diagonal are in gw ([(n + 16)][n], then [n]), Ls.bad_spd is set on
// a non-positive / non-finite pivot.  All kWideSolveThreads threads; P = the dynamic LDS block [(n + 16)][SW + 1].
template <int SW, bool HAS_S>
__device__ __forceinline__ void wide_solve_body(double *P, WideSolveLds<SW> &Ls, int r, int n, const double *__restrict__ G, double ca,
                                                const double *__restrict__ S, double cs, double ci, const double *__restrict__ b1,
                                                const double *__restrict__ b2, double cb, const double *__restrict__ zrand, double *gw) {
    constexpr int ldp = SW + 1, NW = kWideSolveThreads / 64;
    double *rdl = Ls.rdl;
    auto &red = Ls.red;
    auto &xs = Ls.xs;
    auto &yv = Ls.yv;
    int &bad_spd = Ls.bad_spd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    double *Lg = gw;                          // [(n + 16)][n]: the factor, then the bordered rows
    double *rdg = gw + (size_t)(n + kNB) * n;  // [n] reciprocal diagonal
    const int nvec = zrand ? 2 : 1;
    if (tid == 0) bad_spd = 0;
    GINGR_STAGE_CLOCK(7)
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int NTJ = SW / 16;                                // tile columns of a panel
    constexpr int TSTEP = NW / NTJ;                             // wave w owns tile column w % NTJ, tile rows w / NTJ + TSTEP q
    constexpr int TACC = SW == 64 ? 9 : 9;                      // tiles per wave, at most: ceil((n + 16) / 16 / TSTEP), n <= 256 (512)
    constexpr int HALF = SW / 2;                                // 16-byte units per staged row
    constexpr int RSTEP = kWideSolveThreads / HALF;             // rows a staging round covers
    constexpr int PRE = 17;                                     // staging rounds, at most: ceil((n + 16) / RSTEP), n <= 256 (512)
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int my_tj = wv % NTJ, ti0 = wv / NTJ;
    // the bordered rows of the workspace: the right-hand side, fifteen zero rows (they ride through every panel)
    for (int e = tid; e < kNB * n; e += kWideSolveThreads) Lg[(size_t)n * n + e] = e < r ? (b2 ? __builtin_fma(cb, b2[e], b1[e]) : b1[e]) : 0.0;
    __syncthreads();
    const int srow = tid / HALF, scp = tid % HALF;              // this thread's row (per round) and column pair of a staged slice
    for (int kb = 0; kb < n; kb += SW) {
        const int sw = min(SW, n - kb), rows = n - kb + kNB;
        const int nti = rows >> 4, ntj = sw >> 4;
        // The panel's tiles, C - L[rows, 0 : kb] L[panel rows, 0 : kb]^T, accumulate in registers while the panel's LDS block stages
        // the operands: the factor's columns go through it SW at a time (coalesced 16-byte loads, the next slice requested before the
        // MFMAs of the current one), and C = I + G (bordered rows: the right-hand side) goes through it last and stays, minus the
        // accumulated products.
        // (Fragments fetched straight from the workspace, 8 bytes per lane and sixteen rows per instruction, made this stage 62 % of
        // the kernel: 354k cycles at r = 256.)
        v4f64 acc[TACC];
#pragma unroll
        for (int q = 0; q < TACC; ++q) acc[q] = v4f64{0, 0, 0, 0};
        const bool col_live = my_tj < ntj;
        const int nsl = kb / SW;  // slices of the factor; slice nsl is C
        d2 pre[PRE];
        auto fetch_slice = [&](int sl) __attribute__((always_inline)) {
            // slice nsl is C itself: the same rows and row stride, read from G; the bordered rows always come from the workspace
            const bool is_c = sl == nsl;
            const int col = sl * SW + 2 * scp;  // (== kb + 2 scp for C)
            const double *base = (is_c ? G : Lg) + col;
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                const int gi = kb + srow + u * RSTEP;
                if (gi < n + kNB) pre[u] = *reinterpret_cast<const d2 *>((gi < n ? base : Lg + col) + (size_t)gi * n);
            }
            if (is_c) {  // workgroup-uniform.  Mm = QtL Q + I, identity on the padding   (scalismo genericRegressionComputations)
                d2 ps[HAS_S ? PRE : 1];
                if (HAS_S) {  // the second matrix of the transition density's system, same rows: one more batch of loads per panel
#pragma unroll
                    for (int u = 0; u < PRE; ++u) {
                        const int gi = kb + srow + u * RSTEP;
                        if (gi < n) ps[u] = *reinterpret_cast<const d2 *>(S + col + (size_t)gi * n);
                    }
                }
#pragma unroll
                for (int u = 0; u < PRE; ++u) {
                    const int gi = kb + srow + u * RSTEP;
                    if (gi < n) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const double one = gi == col + h ? 1.0 : 0.0;
                            double t = ca * pre[u][h];
                            if (HAS_S) t = __builtin_fma(cs, ps[u][h], t);
                            pre[u][h] = (gi < r && col + h < r) ? t + ci * one : one;
                        }
                    }
                }
            }
        };
        fetch_slice(0);
        for (int sl = 0; sl <= nsl; ++sl) {
            __syncthreads();  // (the previous slice, or the previous panel's write-back, has been read)
#pragma unroll
            for (int u = 0; u < PRE; ++u)
                if (srow + u * RSTEP < rows) {
                    P[(srow + u * RSTEP) * ldp + 2 * scp] = pre[u][0];
                    P[(srow + u * RSTEP) * ldp + 2 * scp + 1] = pre[u][1];
                }
            __syncthreads();
            if (sl == nsl) break;
            fetch_slice(sl + 1);
            if (col_live) {  // wave-uniform
                const double *pb = P + (16 * my_tj + l15) * ldp + l4;
#pragma unroll
                for (int q = 0; q < TACC; ++q) {
                    const int ti = ti0 + TSTEP * q;
                    if (ti < nti && ti >= my_tj) {  // wave-uniform; strictly above the diagonal: nobody reads it
                        const double *pa = P + (16 * ti + l15) * ldp + l4;
#pragma unroll 8
                        for (int u = 0; u < SW / 4; ++u) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * u], pb[4 * u], acc[q], 0, 0, 0);
                    }
                }
            }
        }
        if (kb > 0 && col_live) {
#pragma unroll
            for (int q = 0; q < TACC; ++q) {
                const int ti = ti0 + TSTEP * q;
                if (ti < nti && ti >= my_tj) {
                    double *pc = P + (16 * ti + l4) * ldp + 16 * my_tj + l15;  // D[i = l4 + 4 g][j = l15]
#pragma unroll
                    for (int g = 0; g < 4; ++g) pc[4 * g * ldp] -= acc[q][g];
                }
            }
        }
        __syncthreads();
        GINGR_STAGE_CLOCK(0)
        lds_cholesky<kWideSolveThreads>(P, ldp, sw, rdl, &bad_spd, rows - sw);
        {   // the panel goes back to the workspace
            const int j = tid % SW;
            if (j < sw)
                for (int i = tid / SW; i < rows; i += kWideSolveThreads / SW) Lg[(size_t)(kb + i) * n + kb + j] = P[i * ldp + j];
        }
        if (tid < sw) rdg[kb + tid] = rdl[tid];
        GINGR_STAGE_CLOCK(4)
        // The next panel's first slice is requested straight away, and at kb = SW that slice IS the panel just written, by other
        // threads: without this barrier a rare race (one posterior in ~1 500 at rank 150 when other kernels share the device; found
        // through the three-shard tests, tools/experiments/stress_group2.py / stress_group3.py).
        __syncthreads();
    }
    // x = L^-T y: y = row n of the workspace (L^-1 rhs); the sampling direction L^-T z rides along
    const int kb_last = ((n - 1) / SW) * SW;
    for (int kb = kb_last; kb >= 0; kb -= SW) {
        const int sw = min(SW, n - kb);
        {   // t_c = y_c - sum over the rows j below the block of L[j][kb + c] x_j: NW row groups, combined in order
            const int c = tid % SW, g = tid / SW;
            constexpr int NG = kWideSolveThreads / SW;
            double s0 = 0.0, s1 = 0.0;
            if (c < sw)
                for (int j = kb + sw + g; j < n; j += NG) {
                    const double l = Lg[(size_t)j * n + kb + c];
                    s0 = __builtin_fma(l, xs[0][j], s0);
                    if (nvec == 2) s1 = __builtin_fma(l, xs[1][j], s1);
                }
            // (NG row groups of SW columns: the first NW of them land in red, the others are added by their owners below)
            static_assert(NG == NW || NG == 2 * NW, "row groups of the backward mat-vec");
            if (NG == 2 * NW) {
                s0 += __shfl_xor(s0, 32);  // SW = 32: groups g and g + 1 share a wave
                s1 += __shfl_xor(s1, 32);
            }
            if (NG == NW || (lane < 32)) {
                red[0][wave][c] = s0;
                red[1][wave][c] = s1;
            }
        }
        {
            const int j = tid % SW;
            if (j < sw)
                for (int i = tid / SW; i < sw; i += kWideSolveThreads / SW) P[i * ldp + j] = Lg[(size_t)(kb + i) * n + kb + j];
        }
        if (tid < sw) rdl[tid] = rdg[kb + tid];
        __syncthreads();
        if (tid < sw) {
            for (int v = 0; v < nvec; ++v) {
                double t = v == 0 ? Lg[(size_t)n * n + kb + tid] : (kb + tid < r ? zrand[kb + tid] : 0.0);
                for (int w = 0; w < NW; ++w) t -= red[v][w][tid];
                yv[v][tid] = t;
            }
        }
        __syncthreads();
        lds_backward<kWideSolveThreads>(P, ldp, sw, rdl, yv[0]);
        if (nvec == 2) lds_backward<kWideSolveThreads>(P, ldp, sw, rdl, yv[1]);
        if (tid < sw) {
            xs[0][kb + tid] = yv[0][tid];
            xs[1][kb + tid] = nvec == 2 ? yv[1][tid] : 0.0;
        }
        __syncthreads();
    }
}

// The solve itself keeps its own, specialised copy of the body (C = I + G, one right-hand side known at compile time): instantiating
// wide_solve_body for it costs 45 more spilled registers and 15 % of the kernel (135 -> 155 us at r = 256, tools/ubench_solve_wide.hip) --
// the register allocator's doing, not the arithmetic's; the transition density above ranks 112 uses the general body.
template <int SW>
__global__ __launch_bounds__(kWideSolveThreads) void posterior_solve_wide_kernel(int r, int n, const double *__restrict__ G,
                                                                                 const double *__restrict__ rhs,
                                                                                 const double *__restrict__ zrand, double *__restrict__ a,
                                                                                 DevState *__restrict__ st, double *gw) {
    extern __shared__ double P[];  // the panel: [rows][SW + 1]
    constexpr int ldp = SW + 1, NW = kWideSolveThreads / 64;
    __shared__ double rdl[SW];
    __shared__ double red[2][NW][SW];
    __shared__ double xs[2][512];  // x = L^-T y and, when sampling, L^-T z (n <= 512)
    __shared__ double yv[2][SW];
    __shared__ int bad_spd, bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    double *Lg = gw;                          // [(n + 16)][n]: the factor, then the bordered rows
    double *rdg = gw + (size_t)(n + kNB) * n;  // [n] reciprocal diagonal
    const int nvec = zrand ? 2 : 1;
    if (tid == 0) bad_spd = 0, bad = 0;
    GINGR_STAGE_CLOCK(7)
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int NTJ = SW / 16;                                // tile columns of a panel
    constexpr int TSTEP = NW / NTJ;                             // wave w owns tile column w % NTJ, tile rows w / NTJ + TSTEP q
    constexpr int TACC = SW == 64 ? 9 : 9;                      // tiles per wave, at most: ceil((n + 16) / 16 / TSTEP), n <= 256 (512)
    constexpr int HALF = SW / 2;                                // 16-byte units per staged row
    constexpr int RSTEP = kWideSolveThreads / HALF;             // rows a staging round covers
    constexpr int PRE = 17;                                     // staging rounds, at most: ceil((n + 16) / RSTEP), n <= 256 (512)
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int my_tj = wv % NTJ, ti0 = wv / NTJ;
    // the bordered rows of the workspace: the right-hand side, fifteen zero rows (they ride through every panel)
    for (int e = tid; e < kNB * n; e += kWideSolveThreads) Lg[(size_t)n * n + e] = e < r ? rhs[e] : 0.0;
    __syncthreads();
    const int srow = tid / HALF, scp = tid % HALF;              // this thread's row (per round) and column pair of a staged slice
    for (int kb = 0; kb < n; kb += SW) {
        const int sw = min(SW, n - kb), rows = n - kb + kNB;
        const int nti = rows >> 4, ntj = sw >> 4;
        // The panel's tiles, C - L[rows, 0 : kb] L[panel rows, 0 : kb]^T, accumulate in registers while the panel's LDS block stages
        // the operands: the factor's columns go through it SW at a time (coalesced 16-byte loads, the next slice requested before the
        // MFMAs of the current one), and C = I + G (bordered rows: the right-hand side) goes through it last and stays, minus the
        // accumulated products.
        // (Fragments fetched straight from the workspace, 8 bytes per lane and sixteen rows per instruction, made this stage 62 % of
        // the kernel: 354k cycles at r = 256.)
        v4f64 acc[TACC];
#pragma unroll
        for (int q = 0; q < TACC; ++q) acc[q] = v4f64{0, 0, 0, 0};
        const bool col_live = my_tj < ntj;
        const int nsl = kb / SW;  // slices of the factor; slice nsl is C
        d2 pre[PRE];
        auto fetch_slice = [&](int sl) __attribute__((always_inline)) {
            // slice nsl is C itself: the same rows and row stride, read from G; the bordered rows always come from the workspace
            const bool is_c = sl == nsl;
            const int col = sl * SW + 2 * scp;  // (== kb + 2 scp for C)
            const double *base = (is_c ? G : Lg) + col;
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                const int gi = kb + srow + u * RSTEP;
                if (gi < n + kNB) pre[u] = *reinterpret_cast<const d2 *>((gi < n ? base : Lg + col) + (size_t)gi * n);
            }
            if (is_c) {  // workgroup-uniform.  Mm = QtL Q + I, identity on the padding   (scalismo genericRegressionComputations)
#pragma unroll
                for (int u = 0; u < PRE; ++u) {
                    const int gi = kb + srow + u * RSTEP;
                    if (gi < n) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const double one = gi == col + h ? 1.0 : 0.0;
                            pre[u][h] = (gi < r && col + h < r) ? pre[u][h] + one : one;
                        }
                    }
                }
            }
        };
        fetch_slice(0);
        for (int sl = 0; sl <= nsl; ++sl) {
            __syncthreads();  // (the previous slice, or the previous panel's write-back, has been read)
#pragma unroll
            for (int u = 0; u < PRE; ++u)
                if (srow + u * RSTEP < rows) {
                    P[(srow + u * RSTEP) * ldp + 2 * scp] = pre[u][0];
                    P[(srow + u * RSTEP) * ldp + 2 * scp + 1] = pre[u][1];
                }
            __syncthreads();
            if (sl == nsl) break;
            fetch_slice(sl + 1);
            if (col_live) {  // wave-uniform
                const double *pb = P + (16 * my_tj + l15) * ldp + l4;
#pragma unroll
                for (int q = 0; q < TACC; ++q) {
                    const int ti = ti0 + TSTEP * q;
                    if (ti < nti && ti >= my_tj) {  // wave-uniform; strictly above the diagonal: nobody reads it
                        const double *pa = P + (16 * ti + l15) * ldp + l4;
#pragma unroll 8
                        for (int u = 0; u < SW / 4; ++u) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * u], pb[4 * u], acc[q], 0, 0, 0);
                    }
                }
            }
        }
        if (kb > 0 && col_live) {
#pragma unroll
            for (int q = 0; q < TACC; ++q) {
                const int ti = ti0 + TSTEP * q;
                if (ti < nti && ti >= my_tj) {
                    double *pc = P + (16 * ti + l4) * ldp + 16 * my_tj + l15;  // D[i = l4 + 4 g][j = l15]
#pragma unroll
                    for (int g = 0; g < 4; ++g) pc[4 * g * ldp] -= acc[q][g];
                }
            }
        }
        __syncthreads();
        GINGR_STAGE_CLOCK(0)
        lds_cholesky<kWideSolveThreads>(P, ldp, sw, rdl, &bad_spd, rows - sw);
        {   // the panel goes back to the workspace
            const int j = tid % SW;
            if (j < sw)
                for (int i = tid / SW; i < rows; i += kWideSolveThreads / SW) Lg[(size_t)(kb + i) * n + kb + j] = P[i * ldp + j];
        }
        if (tid < sw) rdg[kb + tid] = rdl[tid];
        GINGR_STAGE_CLOCK(4)
        // The next panel's first slice is requested straight away, and at kb = SW that slice IS the panel just written, by other
        // threads: without this barrier a rare race (one posterior in ~1 500 at rank 150 when other kernels share the device; found
        // through the three-shard tests, tools/experiments/stress_group2.py / stress_group3.py).
        __syncthreads();
    }
    // x = L^-T y: y = row n of the workspace (L^-1 rhs); the sampling direction L^-T z rides along.  Everything a block reads from
    // the workspace -- the rows below it for the mat-vec, its diagonal block, its reciprocal diagonal -- does not depend on the x of the
    // blocks behind it, so it is requested one block AHEAD, before the sequential substitution of the current block, and waits in
    // registers (round 6: two exposed memory round trips per block less).
    const int kb_last = ((n - 1) / SW) * SW;
    constexpr int NG = kWideSolveThreads / SW;          // row groups of the mat-vec
    constexpr int LV = SW == 64 ? 24 : 30;              // rows a thread takes below a block, at most: (n - SW) / NG
    constexpr int DV = SW * SW / kWideSolveThreads;     // diagonal-block entries per thread
    static_assert(NG == NW || NG == 2 * NW, "row groups of the backward mat-vec");
    const int bc = tid % SW, bg = tid / SW;
    double lv[LV], dv[DV], rdv = 0.0;
    auto prefetch_block = [&](int kb) __attribute__((always_inline)) {
        const int sw = min(SW, n - kb);
#pragma unroll
        for (int q = 0; q < LV; ++q) {
            const int j = kb + sw + bg + q * NG;
            lv[q] = (bc < sw && j < n) ? Lg[(size_t)j * n + kb + bc] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < DV; ++q) {
            const int i = bg + q * NG;
            dv[q] = (bc < sw && i < sw) ? Lg[(size_t)(kb + i) * n + kb + bc] : 0.0;
        }
        rdv = tid < sw ? rdg[kb + tid] : 0.0;
    };
    prefetch_block(kb_last);
    for (int kb = kb_last; kb >= 0; kb -= SW) {
        const int sw = min(SW, n - kb);
        {   // t_c = y_c - sum over the rows j below the block of L[j][kb + c] x_j: NG row groups, combined in order
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int q = 0; q < LV; ++q) {
                const int j = kb + sw + bg + q * NG;
                if (j < n) {
                    s0 = __builtin_fma(lv[q], xs[0][j], s0);
                    if (nvec == 2) s1 = __builtin_fma(lv[q], xs[1][j], s1);
                }
            }
            if (NG == 2 * NW) {
                s0 += __shfl_xor(s0, 32);  // SW = 32: groups g and g + 1 share a wave
                s1 += __shfl_xor(s1, 32);
            }
            if (NG == NW || (lane < 32)) {
                red[0][wave][bc] = s0;
                red[1][wave][bc] = s1;
            }
        }
#pragma unroll
        for (int q = 0; q < DV; ++q) {
            const int i = bg + q * NG;
            if (bc < sw && i < sw) P[i * ldp + bc] = dv[q];
        }
        if (tid < sw) rdl[tid] = rdv;
        const double ybase = tid < sw ? Lg[(size_t)n * n + kb + tid] : 0.0;  // (the forward-substituted right-hand side: written long ago)
        if (kb > 0) prefetch_block(kb - SW);
        __syncthreads();
        if (tid < sw) {
            for (int v = 0; v < nvec; ++v) {
                double t = v == 0 ? ybase : (kb + tid < r ? zrand[kb + tid] : 0.0);
                for (int w = 0; w < NW; ++w) t -= red[v][w][tid];
                yv[v][tid] = t;
            }
        }
        __syncthreads();
        lds_backward<kWideSolveThreads>(P, ldp, sw, rdl, yv[0]);
        if (nvec == 2) lds_backward<kWideSolveThreads>(P, ldp, sw, rdl, yv[1]);
        if (tid < sw) {
            xs[0][kb + tid] = yv[0][tid];
            xs[1][kb + tid] = nvec == 2 ? yv[1][tid] : 0.0;
        }
        __syncthreads();
    }
    GINGR_STAGE_CLOCK(5)
    GINGR_STAGE_CLOCK(6)
    for (int k = tid; k < n; k += kWideSolveThreads) {
        const double v = k < r ? xs[0][k] + xs[1][k] : 0.0;
        a[k] = v;
        if (!finite_d(v)) bad = 1;
    }
    __syncthreads();
    if (tid == 0) {
        if (bad_spd)
            st->err = GINGR_ERR_NOT_SPD;
        else if (bad)
            st->err = GINGR_ERR_NONFINITE;
    }
}

// posterior_logpdf_split_kernel for ranks above 112 (round 6; until then posterior_logpdf_lds_kernel<true>: both factorisations one
// after the other in ONE workgroup of 256 threads, 16-column panels over the global workspace).  Two workgroups of eight waves, the
// same algebra: workgroup 0 factors N = I + G and solves N a = rhs; workgroup 1 factors K = S_tot + eps N with the bordered row
// Q0^T e + eps rhs, so that w = K^-1 (Q0^T e + eps rhs), u = w - a and |c|^2 = u^T (N w - rhs); a travels through fx under the
// release / acquire pair on sync[0] (the launch number `epoch`), sync[1] carries workgroup 0's failure flag.  The factor of K, its
// reciprocal diagonal and a are left in fx ([n x n][n][n]) for posterior_logpdf_cached_kernel.  gw: two workspaces of
// wide_solve_work_doubles(n) doubles each, gw_stride apart.
template <int SW>
__global__ __launch_bounds__(kWideSolveThreads) void posterior_logpdf_wide_kernel(int r, int n, const double *__restrict__ G,
                                                                                  const double *__restrict__ rhs,
                                                                                  const double *__restrict__ Stot,
                                                                                  const double *__restrict__ qte, double *__restrict__ fx,
                                                                                  double *__restrict__ out2, unsigned *sync, unsigned epoch,
                                                                                  double *gw, int64_t gw_stride) {
    extern __shared__ double P[];
    __shared__ WideSolveLds<SW> Ls;
    __shared__ int failed0;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        wide_solve_body<SW, false>(P, Ls, r, n, G, 1.0, nullptr, 0.0, 1.0, rhs, nullptr, 0.0, nullptr, gw);
        for (int k = tid; k < n; k += kWideSolveThreads) fx[(int64_t)n * n + k] = k < r ? Ls.xs[0][k] : 0.0;
        __syncthreads();
        if (tid == 0) {
            sync[1] = (unsigned)Ls.bad_spd;
            __hip_atomic_store(&sync[0], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // a and the flag are visible before it
        }
        return;
    }
    double *gw1 = gw + gw_stride;
    wide_solve_body<SW, true>(P, Ls, r, n, G, GINGR_COEFF_NOISE, Stot, 1.0, GINGR_COEFF_NOISE, qte, rhs, GINGR_COEFF_NOISE, nullptr, gw1);
    const double *w = Ls.xs[0];
    // (G w)_k: the thread's column k (G is symmetric: coalesced over k), two halves of the row range, four chains each
    double *hv = P;  // [2][512] (the panel block is free)
    __syncthreads();
    for (int kk = tid & 255; kk < r; kk += 256) {
        const int half = tid >> 8;
        const int j0 = half ? (r + 1) / 2 : 0, j1 = half ? r : (r + 1) / 2;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int j = j0;
        for (; j + 3 < j1; j += 4) {
            s0 = __builtin_fma(G[(int64_t)j * n + kk], w[j], s0);
            s1 = __builtin_fma(G[(int64_t)(j + 1) * n + kk], w[j + 1], s1);
            s2 = __builtin_fma(G[(int64_t)(j + 2) * n + kk], w[j + 2], s2);
            s3 = __builtin_fma(G[(int64_t)(j + 3) * n + kk], w[j + 3], s3);
        }
        for (; j < j1; ++j) s0 = __builtin_fma(G[(int64_t)j * n + kk], w[j], s0);
        hv[half * 512 + kk] = (s0 + s1) + (s2 + s3);
    }
    // the state-only part for posterior_logpdf_cached_kernel: the factor of K (lower part; the workspace rows have stride n) and its
    // reciprocal diagonal
    for (int64_t e = tid; e < (int64_t)n * n / 2; e += kWideSolveThreads) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        reinterpret_cast<d2 *>(fx)[e] = reinterpret_cast<const d2 *>(gw1)[e];
    }
    for (int k = tid; k < n; k += kWideSolveThreads) fx[(int64_t)n * n + n + k] = gw1[(size_t)(n + kNB) * n + k];
    if (tid == 0) {
        while (__hip_atomic_load(&sync[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) __builtin_amdgcn_s_sleep(2);
        failed0 = (int)__hip_atomic_load(&sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    double part = 0.0;
    for (int k = tid; k < r; k += kWideSolveThreads) {
        const double av = __hip_atomic_load(&fx[(int64_t)n * n + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double nw = (hv[k] + hv[512 + k]) + w[k];  // (N w)_k
        part = __builtin_fma(w[k] - av, nw - rhs[k], part);
    }
    double *redv = P + 1024;  // [kWideSolveThreads]
    redv[tid] = part;
    __syncthreads();
    for (int st2 = kWideSolveThreads / 2; st2 > 0; st2 >>= 1) {
        if (tid < st2) redv[tid] += redv[tid + st2];
        __syncthreads();
    }
    if (tid == 0) {
        const bool bad = Ls.bad_spd || failed0;
        out2[0] = bad ? __builtin_nan("") : -0.5 * redv[0] - 0.5 * (double)r * 1.8378770664093454836;  // log(2 pi)
        out2[1] = bad ? 1.0 : 0.0;
    }
}

// ---- pieces shared by the three transition-density kernels (256 threads: 128 entries x 2 column halves) -------------------------
// u[k] = qte[k] - (S_tot a)[k]: two threads per entry (column halves of the symmetric S_tot: coalesced), four loads in flight.
// Ends with the entries written but NOT yet synchronised.
__device__ __forceinline__ void logpdf_rhs(int r, int rp, const double *__restrict__ Stot, const double *__restrict__ qte, const double *av,
                                           double (*hv)[512], double *u) {
    const int tid = threadIdx.x;
    {
        const int k = tid & 127, half = tid >> 7;
        for (int kk = k; kk < r; kk += 128) {
            const int j0 = half ? (r + 1) / 2 : 0, j1 = half ? r : (r + 1) / 2;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int j = j0;
            for (; j + 3 < j1; j += 4) {
                s0 = __builtin_fma(Stot[(int64_t)j * rp + kk], av[j], s0);
                s1 = __builtin_fma(Stot[(int64_t)(j + 1) * rp + kk], av[j + 1], s1);
                s2 = __builtin_fma(Stot[(int64_t)(j + 2) * rp + kk], av[j + 2], s2);
                s3 = __builtin_fma(Stot[(int64_t)(j + 3) * rp + kk], av[j + 3], s3);
            }
            for (; j < j1; ++j) s0 = __builtin_fma(Stot[(int64_t)j * rp + kk], av[j], s0);
            hv[half][kk] = (s0 + s1) + (s2 + s3);
        }
    }
    __syncthreads();
    for (int k = tid; k < r; k += kSolveThreads) u[k] = qte[k] - (hv[0][k] + hv[1][k]);
}

// u^T (I + G) u, the same value in every thread (red: kSolveThreads doubles of LDS)
__device__ __forceinline__ double logpdf_quadratic(int r, int rp, const double *__restrict__ G, const double *u, double *red) {
    const int tid = threadIdx.x;
    double part = 0.0;
    {
        const int k = tid & 127, half = tid >> 7;
        for (int kk = k; kk < r; kk += 128) {
            const int j0 = half ? (r + 1) / 2 : 0, j1 = half ? r : (r + 1) / 2;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int j = j0;
            for (; j + 3 < j1; j += 4) {  // G symmetric: G[j][kk], coalesced over kk
                s0 = __builtin_fma(G[(int64_t)j * rp + kk], u[j], s0);
                s1 = __builtin_fma(G[(int64_t)(j + 1) * rp + kk], u[j + 1], s1);
                s2 = __builtin_fma(G[(int64_t)(j + 2) * rp + kk], u[j + 2], s2);
                s3 = __builtin_fma(G[(int64_t)(j + 3) * rp + kk], u[j + 3], s3);
            }
            for (; j < j1; ++j) s0 = __builtin_fma(G[(int64_t)j * rp + kk], u[j], s0);
            double g = (s0 + s1) + (s2 + s3);
            if (half == 0) g += u[kk];
            part = __builtin_fma(u[kk], g, part);
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int st2 = kSolveThreads / 2; st2 > 0; st2 >>= 1) {
        if (tid < st2) red[tid] += red[tid + st2];
        __syncthreads();
    }
    return red[0];
}

// log-density of a mesh under the posterior model in scalismo's parameterisation:
//   posterior.gp.logpdf(posterior.coefficients(mesh))   (G/api/sampling/generators/GeneratorWrapperStochastic.scala:42-63)
// With N = Q0' L^-T (any square root of the posterior covariance gives the same norm) the ridge-regression coefficients are
//   c = (N^T N + eps I)^-1 N^T d = L^T (S_tot + eps (I + G))^-1 b,   b = Q0^T e - S_tot a,
// e = R^T(mesh - c - t) - (ref - c) - mean (model frame residual), a = posterior coefficients;  logpdf = -|c|^2/2 - r/2 log(2 pi).
template <bool GW>  // see posterior_solve_lds_kernel
__global__ __launch_bounds__(kSolveThreads) void posterior_logpdf_lds_kernel(int r, int rp, const double *__restrict__ G,
                                                                   const double *__restrict__ rhs,
                                                                   const double *__restrict__ Stot,
                                                                   const double *__restrict__ qte,
                                                                   double *__restrict__ fx /* nullable: [rp*rp] second factor, [rp] a, [rp] 1/diag */,
                                                                   double *__restrict__ out2, double *gwork) {
    extern __shared__ double lds_sm[];
    double *sm;
    if constexpr (GW)
        sm = gwork;
    else
        sm = lds_sm;
    const int n = rp, ld = solve_ld(n);
    double *A = sm;
    double *u = sm + (size_t)n * ld;  // extra row block of the bordered matrix
    double *rd = sm + (size_t)(n + kNB) * ld;
    __shared__ int bad_spd;
    __shared__ double red[kSolveThreads];
    __shared__ double av[512];  // posterior coefficients a (rp <= 512)
    __shared__ double hv[2][512];  // the two half sums of the mat-vecs
    static_assert(kSolveThreads == 256, "the mat-vecs below split 256 threads into 128 entries x 2 halves");
    const int tid = threadIdx.x;
    if (tid == 0) bad_spd = 0;
    // (1) a = (I + G)^-1 rhs: the posterior coefficients of the state (what posterior_solve_lds_kernel computes)
    for (int k = tid; k < kNB * ld; k += kSolveThreads) u[k] = k < r ? rhs[k] : 0.0;
    lds_load_spd<kSolveThreads>(A, ld, r, n, G, 1.0, nullptr, 0.0, 1.0);
    lds_cholesky<kSolveThreads>(A, ld, n, rd, &bad_spd, kNB);  // u <- L^-1 rhs on the way
    lds_backward<kSolveThreads>(A, ld, n, rd, u);
    for (int k = tid; k < rp; k += kSolveThreads) {
        av[k] = k < r ? u[k] : 0.0;
        if (fx) fx[(int64_t)rp * rp + k] = av[k];
    }
    __syncthreads();
    // (2) b = Q0^T e - S_tot a
    for (int k = tid; k < kNB * ld; k += kSolveThreads) u[k] = 0.0;
    __syncthreads();
    logpdf_rhs(r, rp, Stot, qte, av, hv, u);
    // (3) u = (S_tot + eps (I + G))^-1 b
    lds_load_spd<kSolveThreads, true>(A, ld, r, n, G, GINGR_COEFF_NOISE, Stot, 1.0, GINGR_COEFF_NOISE);
    lds_cholesky<kSolveThreads>(A, ld, n, rd, &bad_spd, kNB);                                        // u <- L2^-1 u on the way
    lds_backward<kSolveThreads>(A, ld, n, rd, u);
    __syncthreads();
    if (fx) {  // everything of the second system that depends on the state alone: posterior_logpdf_cached_kernel starts from here
        for (int i = tid >> 6; i < n; i += kSolveThreads / 64)  // one wave per row: no index division, coalesced
            for (int j = tid & 63; j < n; j += 64) fx[(int64_t)i * rp + j] = A[i * ld + j];
        for (int k = tid; k < n; k += kSolveThreads) fx[(int64_t)rp * rp + rp + k] = rd[k];
    }
    // (4) |c|^2 with c = L^T u, L L^T = I + G:  |c|^2 = u^T (I + G) u -- a quadratic form with G itself, so the first factor does
    //     not have to survive the second factorisation (it used to be parked in a global scratch and read back)
    const double n2 = logpdf_quadratic(r, rp, G, u, red);
    if (tid == 0) {
        out2[0] = bad_spd ? __builtin_nan("") : -0.5 * n2 - 0.5 * (double)r * 1.8378770664093454836;  // log(2 pi)
        out2[1] = bad_spd ? 1.0 : 0.0;
    }
}

// posterior_logpdf_lds_kernel on TWO workgroups (r <= 128): the factor of K = S_tot + eps (I + G) does not depend on the posterior
// coefficients a, so workgroup 1 factors it while workgroup 0 factors N = I + G and solves N a = rhs.  Round 4: neither does the
// right-hand side have to wait for a -- S_tot a = K a - eps N a = K a - eps rhs, hence
//     u = K^-1 (Q0^T e - S_tot a) = K^-1 (Q0^T e + eps rhs) - a =: w - a,        |c|^2 = u^T N u = u^T (N w - rhs)
// -- so workgroup 1 lets the forward solve of (Q0^T e + eps rhs) ride through its factorisation, substitutes back, forms N w - rhs,
// and only then picks a up (agent-scope release / acquire on sync[0], the value `epoch` of this launch; sync[1] carries workgroup 0's
// failure flag) for two vector operations: the mat-vec with S_tot, the forward solve and every wait are off the critical path
// (87 us in one workgroup -> 60 -> ~45).  keep != 0 leaves the factor of K, its reciprocal diagonal and a in fx for
// posterior_logpdf_cached_kernel (a Metropolis-Hastings step that asks again about the same state); a always travels through fx.
// Workgroup 0 is dispatched first, so workgroup 1 never waits for a workgroup that has no compute unit.
__global__ __launch_bounds__(kSolveThreads) void posterior_logpdf_split_kernel(int r, int rp, const double *__restrict__ G,
                                                                     const double *__restrict__ rhs,
                                                                     const double *__restrict__ Stot,
                                                                     const double *__restrict__ qte, double *__restrict__ fx,
                                                                     double *__restrict__ out2, unsigned *sync, unsigned epoch, int keep,
                                                                     double *__restrict__ nfac) {
    extern __shared__ double sm[];
    const int n = rp, ld = solve_ld(n);
    double *A = sm;
    double *u = sm + (size_t)n * ld;
    double *rd = sm + (size_t)(n + kNB) * ld;
    __shared__ int bad_spd;
    __shared__ double red[kSolveThreads];
    __shared__ double av[512];
    __shared__ double hv[2][512];
    const int tid = threadIdx.x;
    if (tid == 0) bad_spd = 0;
    if (blockIdx.x == 0) {
        // exactly the arithmetic of posterior_solve_lds_kernel<0> (identity rows through the panel solves, W-form backward substitution):
        // the coefficients a -- and the factor a later sampled proposal a + L^-T z is formed from -- carry the bits the solve kernel
        // would produce for this state
        double *y = u, *W = u + kNB * ld, *x = sm + (size_t)(n + 2 * kNB) * ld;
        for (int k = tid; k < kNB * ld; k += kSolveThreads) {
            y[k] = k < r ? rhs[k] : 0.0;
            const int c = k / ld, j = k - c * ld;
            W[k] = (j < n && (j & 15) == c) ? 1.0 : 0.0;
        }
        lds_load_spd<kSolveThreads>(A, ld, r, n, G, 1.0, nullptr, 0.0, 1.0);
        lds_cholesky<kSolveThreads>(A, ld, n, x, &bad_spd, kNB, kNB);  // y <- L^-1 rhs, W <- the transposed inverses of the diagonal blocks
        lds_backward_w<kSolveThreads>(A, ld, n, W, y, x);
        for (int k = tid; k < rp; k += kSolveThreads) fx[(int64_t)rp * rp + k] = k < r ? x[k] : 0.0;
        __syncthreads();
        if (tid == 0) {
            sync[1] = (unsigned)bad_spd;
            __hip_atomic_store(&sync[0], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // a and the flag are visible before it
        }
        if (nfac) {  // the factor for posterior_sample_cached_kernel: L, then the 16 W rows (the substitution above left both as they
                     // were) -- written BEHIND the hand-over of a (round 6): 115 KB that workgroup 1 does not have to wait for
            for (int i = tid >> 6; i < n + kNB; i += kSolveThreads / 64) {
                const double *src = i < n ? A + i * ld : W + (i - n) * ld;
                for (int j = tid & 63; j < n; j += 64) nfac[(int64_t)i * rp + j] = src[j];
            }
        }
        return;
    }
    GINGR_STAGE_CLOCK(7)
    // (round 6: the W form of the backward substitution here too -- sixteen identity rows ride through the panel solves and come back
    // as the transposed inverses of the diagonal blocks, as in workgroup 0; 12.5k -> ~6k cycles of this workgroup's critical path)
    double *Wk = u + kNB * ld, *rdk = sm + (size_t)(n + 2 * kNB) * ld, *wv = rdk + n;
    for (int k = tid; k < kNB * ld; k += kSolveThreads) {
        u[k] = k < r ? __builtin_fma(GINGR_COEFF_NOISE, rhs[k], qte[k]) : 0.0;
        const int c = k / ld, j = k - c * ld;
        Wk[k] = (j < n && (j & 15) == c) ? 1.0 : 0.0;
    }
    lds_load_spd<kSolveThreads, true>(A, ld, r, n, G, GINGR_COEFF_NOISE, Stot, 1.0, GINGR_COEFF_NOISE);
    GINGR_STAGE_CLOCK(0)
    lds_cholesky<kSolveThreads>(A, ld, n, rdk, &bad_spd, kNB, kNB);  // u <- L_K^-1 (Q0^T e + eps rhs) on the way
    lds_backward_w<kSolveThreads>(A, ld, n, Wk, u, wv);              // wv = w
    __syncthreads();
    rd = rdk;
    u = wv;
    GINGR_STAGE_CLOCK(4)
    {   // hv[0] + hv[1] = G w (two halves of the row range per column, coalesced over the column)
        const int k = tid & 127, half = tid >> 7;
        for (int kk = k; kk < r; kk += 128) {
            const int j0 = half ? (r + 1) / 2 : 0, j1 = half ? r : (r + 1) / 2;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int j = j0;
            for (; j + 3 < j1; j += 4) {
                s0 = __builtin_fma(G[(int64_t)j * rp + kk], u[j], s0);
                s1 = __builtin_fma(G[(int64_t)(j + 1) * rp + kk], u[j + 1], s1);
                s2 = __builtin_fma(G[(int64_t)(j + 2) * rp + kk], u[j + 2], s2);
                s3 = __builtin_fma(G[(int64_t)(j + 3) * rp + kk], u[j + 3], s3);
            }
            for (; j < j1; ++j) s0 = __builtin_fma(G[(int64_t)j * rp + kk], u[j], s0);
            hv[half][kk] = (s0 + s1) + (s2 + s3);
        }
    }
    if (keep) {  // the state-only part for posterior_logpdf_cached_kernel
        for (int i = tid >> 6; i < n; i += kSolveThreads / 64)
            for (int j = tid & 63; j < n; j += 64) fx[(int64_t)i * rp + j] = A[i * ld + j];
        for (int k = tid; k < n; k += kSolveThreads) fx[(int64_t)rp * rp + rp + k] = rd[k];
    }
    if (tid == 0) {
        while (__hip_atomic_load(&sync[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) __builtin_amdgcn_s_sleep(2);
        if (__hip_atomic_load(&sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) bad_spd = 1;
    }
    __syncthreads();
    double part = 0.0;
    for (int k = tid; k < r; k += kSolveThreads) {
        const double a = __hip_atomic_load(&fx[(int64_t)rp * rp + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double nw = (hv[0][k] + hv[1][k]) + u[k];  // (N w)_k
        part = __builtin_fma(u[k] - a, nw - rhs[k], part);
    }
    red[tid] = part;
    __syncthreads();
    for (int st2 = kSolveThreads / 2; st2 > 0; st2 >>= 1) {
        if (tid < st2) red[tid] += red[tid + st2];
        __syncthreads();
    }
    if (tid == 0) {
        out2[0] = bad_spd ? __builtin_nan("") : -0.5 * red[0] - 0.5 * (double)r * 1.8378770664093454836;  // log(2 pi)
        out2[1] = bad_spd ? 1.0 : 0.0;
    }
    GINGR_STAGE_CLOCK(5)
    GINGR_STAGE_CLOCK(6)
    (void)av;
}

// The sampled proposal a + L^-T z of a state whose I + G the two-workgroup log-density kernel has factored already (nfac: [rp*rp] L,
// [16*rp] the W rows; a_mean): one load and one W-form backward substitution instead of the factorisation (32 -> ~12 us at r = 100),
// with the bits posterior_solve_lds_kernel<0> gives (same routines on the same factor, same order of the final addition).
__global__ __launch_bounds__(kSolveThreads) void posterior_sample_cached_kernel(int r, int rp, const double *__restrict__ nfac,
                                                                      const double *__restrict__ a_mean,
                                                                      const double *__restrict__ zrand, double *__restrict__ a,
                                                                      DevState *__restrict__ st) {
    extern __shared__ double sm[];
    const int n = rp, ld = solve_ld(n);
    double *A = sm;
    double *W = sm + (size_t)n * ld;
    double *y2 = sm + (size_t)(n + kNB) * ld;
    double *x = y2 + n;
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    lds_fill_rows<kSolveThreads>(A, ld, nfac, rp, n + kNB, n);  // (rows n .. n+15 of the copy are the W rows: same stride)
    for (int k = tid; k < n; k += kSolveThreads) y2[k] = k < r ? zrand[k] : 0.0;
    __syncthreads();
    lds_backward_w<kSolveThreads>(A, ld, n, W, y2, x);
    __syncthreads();
    for (int k = tid; k < rp; k += kSolveThreads) {
        const double v = k < r ? a_mean[k] + x[k] : 0.0;
        a[k] = v;
        if (!finite_d(v)) bad = 1;
    }
    __syncthreads();
    if (tid == 0 && bad) st->err = GINGR_ERR_NONFINITE;
}

// The same log-density for a state whose posterior_logpdf_lds_kernel has run before (fx: its posterior coefficients and the factor
// of S_tot + eps (I + G), both functions of the state alone): only the mesh-dependent part is left -- b, two triangular solves, the
// quadratic form.  A Metropolis-Hastings step asks for q(x' | x) of a state x that was the x' or the x of the step before.
template <bool GW>
__global__ __launch_bounds__(kSolveThreads) void posterior_logpdf_cached_kernel(int r, int rp, const double *__restrict__ G,
                                                                      const double *__restrict__ Stot,
                                                                      const double *__restrict__ qte,
                                                                      const double *__restrict__ fx, double *__restrict__ out2,
                                                                      double *gwork) {
    extern __shared__ double lds_sm[];
    double *sm;
    if constexpr (GW)
        sm = gwork;
    else
        sm = lds_sm;
    const int n = rp, ld = solve_ld(n);
    double *A = sm;
    double *u = sm + (size_t)n * ld;
    double *rd = sm + (size_t)(n + kNB) * ld;
    __shared__ double red[kSolveThreads];
    __shared__ double av[512];
    __shared__ double hv[2][512];
    const int tid = threadIdx.x;
    if constexpr (GW) {
        for (int i = tid >> 6; i < n; i += kSolveThreads / 64)
            for (int j = tid & 63; j < n; j += 64) A[i * ld + j] = fx[(int64_t)i * rp + j];
    } else {
        lds_fill_rows<kSolveThreads>(A, ld, fx, rp, n, n);
    }
    for (int k = tid; k < n; k += kSolveThreads) {
        rd[k] = fx[(int64_t)rp * rp + rp + k];
        av[k] = k < r ? fx[(int64_t)rp * rp + k] : 0.0;
    }
    for (int k = tid; k < kNB * ld; k += kSolveThreads) u[k] = 0.0;
    __syncthreads();
    logpdf_rhs(r, rp, Stot, qte, av, hv, u);  // step (2) of posterior_logpdf_lds_kernel, same order of operations
    __syncthreads();
    lds_forward<kSolveThreads>(A, ld, n, rd, u);
    lds_backward<kSolveThreads>(A, ld, n, rd, u);
    __syncthreads();
    const double n2 = logpdf_quadratic(r, rp, G, u, red);  // step (4)
    if (tid == 0) {
        out2[0] = -0.5 * n2 - 0.5 * (double)r * 1.8378770664093454836;  // log(2 pi)
        out2[1] = 0.0;
    }
}

// out[i] = (sum_j Binv[i][j] * p[j]) / eps: 16 lanes per output row, fixed-order shuffle reduction.
// Every lane of the 16-lane group returns the result.
__device__ __forceinline__ double binv_row_apply16(const double *__restrict__ Binv, const double *__restrict__ p, int r, int rp,
                                                   int i, int lane16) {
    double s = 0.0;
    if (i < r)
        for (int j = lane16; j < r; j += 16) s = __builtin_fma(Binv[(int64_t)i * rp + j], p[j], s);
    s = group16_sum(s);
    return s / GINGR_COEFF_NOISE;
}


__global__ __launch_bounds__(256) void coeff_solve_kernel(int r, int rp, const double *__restrict__ Binv,
                                                          const double *__restrict__ p, double *__restrict__ out) {
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), lane16 = threadIdx.x & 15;
    const double v = binv_row_apply16(Binv, p, r, rp, i, lane16);
    if (i < rp && lane16 == 0) out[i] = i < r ? v : 0.0;
}

}  // namespace

// the bordered matrix of a one-workgroup solve on the global workspace (posterior_solve_wide_kernel, posterior_logpdf_lds_kernel<true>,
// posterior_logpdf_cached_kernel<true>; per workgroup of posterior_logpdf_wide_kernel)
static int64_t wide_solve_work_doubles(int32_t rp) { return (int64_t)lds_solve_doubles(rp, kNB); }

int64_t posterior_work_doubles(int32_t rp) {
    const int64_t one_workgroup = wide_solve_work_doubles(rp);
    const int64_t two_workgroups = rp >= 128 ? 2 * wide_solve_work_doubles(rp) : 0;  // posterior_logpdf_wide_kernel: side by side
    const int64_t two_dense_systems = rp > 240 ? 2 * DenseSpdWork::doubles(rp, DenseSpdWork::kRhsRows) : 0;  // launch_posterior_logpdf, rp > 384
    return std::max({one_workgroup, two_workgroups, two_dense_systems});
}

namespace {
// From rank 241 on the posterior mean takes the multi-workgroup blocked solve of the classic non-rigid CPD (dense_spd.hip:
// dense_spd_solve3 -- 64-column panels, the trailing update spread over the chip, one launch per stage): one compute unit's matrix
// pipe is the floor of the one-workgroup kernel (380k cycles of MFMA at r = 512), the launches of this form cost ~6 us each.
// Aw: (Mp + 64) x Mp, lower triangle of I + G with the identity on the padding, the right-hand side in border row Mp
// (spd_system_kernel<SpdIdentityPlus, SpdRhsRow>).
__global__ __launch_bounds__(256) void solve_finish_kernel(int r, int rp, const double *__restrict__ W, const int32_t *__restrict__ flag,
                                                           double *__restrict__ a, DevState *__restrict__ st) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < rp; k += 256) {
        const double v = k < r ? W[k] : 0.0;
        a[k] = v;
        if (!finite_d(v)) bad = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (*flag == GINGR_ERR_NOT_SPD)
            st->err = GINGR_ERR_NOT_SPD;
        else if (bad)
            st->err = GINGR_ERR_NONFINITE;
    }
}

// The transition density above padded rank 384 on the same multi-workgroup solve, twice: N a = rhs and K w = Q0^T e + eps rhs with
// K = S_tot + eps N (the two functors below write its bordered system), then one workgroup forms |c|^2 = (w - a)^T (N w - rhs) and
// leaves the factor of K, its reciprocal diagonal and a in fx for posterior_logpdf_cached_kernel.
struct LogpdfElem {  // S_tot + eps (I + G), row stride n
    const double *__restrict__ G, *__restrict__ Stot;
    int n;
    __device__ double operator()(int64_t row, int64_t c) const {
        double v = __builtin_fma(GINGR_COEFF_NOISE, G[row * n + c], Stot[row * n + c]);
        if (row == c) v += GINGR_COEFF_NOISE;
        return v;
    }
};
struct LogpdfRhsRow {  // Q0^T e + eps rhs in border row 0
    const double *__restrict__ rhs, *__restrict__ qte;
    __device__ double operator()(int64_t brow, int64_t c, int r) const {
        return (brow == 0 && c < r) ? __builtin_fma(GINGR_COEFF_NOISE, rhs[c], qte[c]) : 0.0;
    }
};
__global__ __launch_bounds__(512) void logpdf_finish_kernel(int r, int n, int64_t Mp, const double *__restrict__ G, const double *__restrict__ rhs,
                                                            const double *__restrict__ Wn, const double *__restrict__ Wk, const double *__restrict__ Lk,
                                                            const int32_t *__restrict__ flag_n, const int32_t *__restrict__ flag_k,
                                                            double *__restrict__ fx, double *__restrict__ out2) {
    __shared__ double w[512], hv[2][512], red[512];
    const int tid = threadIdx.x;
    for (int k = tid; k < n; k += 512) w[k] = k < r ? Wk[k] : 0.0;
    __syncthreads();
    for (int kk = tid & 255; kk < r; kk += 256) {  // (G w)_k: column k of the symmetric G, two halves of the row range, four chains each
        const int half = tid >> 8;
        const int j0 = half ? (r + 1) / 2 : 0, j1 = half ? r : (r + 1) / 2;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int j = j0;
        for (; j + 3 < j1; j += 4) {
            s0 = __builtin_fma(G[(int64_t)j * n + kk], w[j], s0);
            s1 = __builtin_fma(G[(int64_t)(j + 1) * n + kk], w[j + 1], s1);
            s2 = __builtin_fma(G[(int64_t)(j + 2) * n + kk], w[j + 2], s2);
            s3 = __builtin_fma(G[(int64_t)(j + 3) * n + kk], w[j + 3], s3);
        }
        for (; j < j1; ++j) s0 = __builtin_fma(G[(int64_t)j * n + kk], w[j], s0);
        hv[half][kk] = (s0 + s1) + (s2 + s3);
    }
    // the state-only part for the cached form: factor of K (rows of stride n), its reciprocal diagonal, a
    for (int64_t e = tid; e < (int64_t)n * n; e += 512) {
        const int64_t i = e / n, j = e - i * n;
        fx[e] = j <= i ? Lk[i * Mp + j] : 0.0;
    }
    for (int k = tid; k < n; k += 512) {
        fx[(int64_t)n * n + k] = k < r ? Wn[k] : 0.0;
        fx[(int64_t)n * n + n + k] = 1.0 / Lk[(int64_t)k * Mp + k];
    }
    __syncthreads();
    double part = 0.0;
    for (int k = tid; k < r; k += 512) {
        const double nw = (hv[0][k] + hv[1][k]) + w[k];  // (N w)_k
        part = __builtin_fma(w[k] - Wn[k], nw - rhs[k], part);
    }
    red[tid] = part;
    __syncthreads();
    for (int st2 = 256; st2 > 0; st2 >>= 1) {
        if (tid < st2) red[tid] += red[tid + st2];
        __syncthreads();
    }
    if (tid == 0) {
        const bool bad = *flag_n != 0 || *flag_k != 0;
        out2[0] = bad ? __builtin_nan("") : -0.5 * red[0] - 0.5 * (double)r * 1.8378770664093454836;  // log(2 pi)
        out2[1] = bad ? 1.0 : 0.0;
    }
}
}  // namespace

void launch_posterior_solve_separable(gingr_ctx *ctx, const gingr_model *m, const double *G, const double *rhs, double *a, DevState *st) {
    TimerScope ts(ctx, 5);
    const size_t lds = lds_solve_doubles(kCompactCols, 2 * kNB) * sizeof(double);  // (32 KB: below the limit that needs the attribute)
    hipLaunchKernelGGL(posterior_solve_lds_kernel<2>, dim3(3), dim3(kSolveThreads), lds, ctx->stream, (int)m->r, (int)m->rp, G, rhs,
                       (const double *)nullptr, a, st, (const int32_t *)m->sep_map, SepCounts{{m->rc[0], m->rc[1], m->rc[2]}});
}

void launch_posterior_solve(gingr_ctx *ctx, int32_t r, int32_t rp, const double *G, const double *rhs, const double *zrand,
                            double *work, double *a, DevState *st) {
    TimerScope ts(ctx, 5);
    if (rp > 240 && !zrand) {  // (from rp = 256 on: 138 us against 145 there, 277 against 709 at rp = 512; a sampled proposal needs L^-T z as well: the one-workgroup kernel below)
        const DenseSpdWork ws(rp, DenseSpdWork::kRhsRows);
        double *Aw = work + ws.aw(), *Linv = work + ws.linv(), *W = work + ws.w();
        int32_t *flag = reinterpret_cast<int32_t *>(work + ws.flag());
        launch_spd_system(ctx->stream, (int)r, ws, SpdIdentityPlus{G, (int)rp}, SpdRhsRow{rhs}, Aw, flag);
        dense_spd_solve3(ctx, Aw, ws.Mp, Linv, W, flag);
        hipLaunchKernelGGL(solve_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)r, (int)rp, W, flag, a, st);
        return;
    }
    if (r <= 128) {
        const bool fast = rp <= 112;  // sixteen identity rows fit beside the bordered matrix
        const size_t lds = lds_solve_doubles(rp, fast ? 2 * kNB : kNB) * sizeof(double);
        auto go = [&](auto kern) {
            if (lds > 48 * 1024)  // per function and per device: set whenever needed
                set_dynamic_lds(kern, (size_t)(lds));
            hipLaunchKernelGGL(kern, dim3(1), dim3(kSolveThreads), lds, ctx->stream, (int)r, (int)rp, G, rhs, zrand, a, st,
                               (const int32_t *)nullptr, SepCounts{});
        };
        if (fast)
            go(posterior_solve_lds_kernel<0>);
        else
            go(posterior_solve_lds_kernel<1>);
        return;
    }
    // r > 128: the bordered matrix does not fit the LDS; super-panels of 64 (rp <= 256) or 32 columns on the global workspace
    // (posterior_work_doubles)
    auto gow = [&](auto kern, int sw) {
        const size_t lds = (size_t)(rp + kNB) * (sw + 1) * sizeof(double);
        set_dynamic_lds(kern, (size_t)(lds));
        hipLaunchKernelGGL(kern, dim3(1), dim3(kWideSolveThreads), lds, ctx->stream, (int)r, (int)rp, G, rhs, zrand, a, st, work);
    };
    if (rp <= 256)
        gow(posterior_solve_wide_kernel<64>, 64);
    else
        gow(posterior_solve_wide_kernel<32>, 32);
}

namespace {
// a = V ((V^T rhs) / (1 + lam / sigma2)): two r x r mat-vecs (V from L2), one workgroup; 16 lanes per output entry
__global__ __launch_bounds__(1024) void posterior_solve_eig_kernel(int r, int rp, const double *__restrict__ V,
                                                                   const double *__restrict__ lam, const double *__restrict__ sigma2,
                                                                   const double *__restrict__ rhs, double *__restrict__ a, DevState *st) {
    __shared__ double x[512], t[512];
    __shared__ int bad;
    const int tid = threadIdx.x, lane16 = tid & 15, grp = tid >> 4;
    if (tid == 0) bad = 0;
    for (int k = tid; k < r; k += 1024) x[k] = rhs[k];
    __syncthreads();
    const double inv_s2 = 1.0 / sigma2[0];
    for (int k = grp; k < r; k += 64) {  // t_k = (V[:, k] . rhs) / (1 + lam_k / sigma2)
        double s = 0.0;
        for (int i = lane16; i < r; i += 16) s = __builtin_fma(V[(int64_t)i * r + k], x[i], s);
        s = group16_sum(s);
        if (lane16 == 0) t[k] = s / (1.0 + lam[k] * inv_s2);
    }
    __syncthreads();
    for (int i = grp; i < rp; i += 64) {  // a_i = V[i, :] . t
        double s = 0.0;
        if (i < r)
            for (int k = lane16; k < r; k += 16) s = __builtin_fma(V[(int64_t)i * r + k], t[k], s);
        s = group16_sum(s);
        if (lane16 == 0) {
            a[i] = i < r ? s : 0.0;
            if (!finite_d(s)) bad = 1;
        }
    }
    __syncthreads();
    if (tid == 0 && bad) st->err = GINGR_ERR_NONFINITE;
}
}  // namespace

void launch_posterior_solve_eig(gingr_ctx *ctx, int32_t r, int32_t rp, const double *eigV, const double *eigL, const double *sigma2,
                                const double *rhs, double *a, DevState *st) {
    hipLaunchKernelGGL(posterior_solve_eig_kernel, dim3(1), dim3(1024), 0, ctx->stream, (int)r, (int)rp, eigV, eigL, sigma2, rhs, a, st);
}

int launch_posterior_logpdf(gingr_ctx *ctx, int32_t r, int32_t rp, const double *G, const double *rhs, const double *Stot,
                            const double *qte, double *fx, bool cached, double *work, double *out2, unsigned *sync, unsigned epoch,
                            bool keep_factor, double *nfac) {
    const size_t lds = lds_solve_doubles(rp, kNB) * sizeof(double);
    // the log-density kernels keep 14 KB of static LDS (mat-vec scratch) next to the bordered matrix: with rp = 128 the two exceed the
    // 160 KB of a compute unit, so ranks above 112 take the global-workspace variants (the plain solve fits up to rp = 128)
    const bool in_lds = rp <= 112;
    if (!cached && in_lds && fx && sync) {  // the two factorisations side by side
        const size_t lds2 = lds_solve_doubles(rp, 2 * kNB) * sizeof(double);  // (workgroup 0 carries the identity rows of the solve kernel)
        if (lds2 > 48 * 1024)  // per function and per device: set whenever needed
            set_dynamic_lds(&posterior_logpdf_split_kernel, (size_t)(lds2));
        hipLaunchKernelGGL(posterior_logpdf_split_kernel, dim3(2), dim3(kSolveThreads), lds2, ctx->stream, (int)r, (int)rp, G, rhs, Stot, qte, fx,
                           out2, sync, epoch, keep_factor ? 1 : 0, nfac);
        return GINGR_OK;
    }
    if (!cached && rp > 384 && fx) {  // above padded rank 384: both systems through the multi-workgroup blocked solve, one after the other
                                      // (r = 512: 743 us against 1 024 for the two workgroups below; r = 300: 460 against 366, hence the limit)
        const DenseSpdWork ws(rp, DenseSpdWork::kRhsRows);
        const int64_t Mp = ws.Mp;
        double *work1 = work + ws.doubles();  // the second system behind the first
        double *Aw0 = work + ws.aw(), *Li0 = work + ws.linv(), *W0 = work + ws.w();
        double *Aw1 = work1 + ws.aw(), *Li1 = work1 + ws.linv(), *W1 = work1 + ws.w();
        int32_t *f0 = reinterpret_cast<int32_t *>(work + ws.flag()), *f1 = reinterpret_cast<int32_t *>(work1 + ws.flag());
        launch_spd_system(ctx->stream, (int)r, ws, SpdIdentityPlus{G, (int)rp}, SpdRhsRow{rhs}, Aw0, f0);
        dense_spd_solve3(ctx, Aw0, Mp, Li0, W0, f0);
        launch_spd_system(ctx->stream, (int)r, ws, LogpdfElem{G, Stot, (int)rp}, LogpdfRhsRow{rhs, qte}, Aw1, f1);
        dense_spd_solve3(ctx, Aw1, Mp, Li1, W1, f1);
        hipLaunchKernelGGL(logpdf_finish_kernel, dim3(1), dim3(512), 0, ctx->stream, (int)r, (int)rp, Mp, G, rhs, W0, W1, Aw1, f0, f1, fx, out2);
        return GINGR_OK;
    }
    if (!cached && !in_lds && fx && sync) {  // ranks above 112: the two factorisations side by side on the global workspaces
        const int64_t stride = wide_solve_work_doubles(rp);
        auto gow = [&](auto kern, int sw) {
            const size_t ldsw = (size_t)(rp + kNB) * (sw + 1) * sizeof(double);
            set_dynamic_lds(kern, (size_t)(ldsw));
            hipLaunchKernelGGL(kern, dim3(2), dim3(kWideSolveThreads), ldsw, ctx->stream, (int)r, (int)rp, G, rhs, Stot, qte, fx, out2, sync, epoch,
                               work, stride);
        };
        if (rp <= 256)
            gow(posterior_logpdf_wide_kernel<64>, 64);
        else
            gow(posterior_logpdf_wide_kernel<32>, 32);
        return GINGR_OK;
    }
    if (cached) {  // fx holds what an earlier launch for this state left
        if (in_lds) {
            if (lds > 48 * 1024)  // per function and per device: set whenever needed
                set_dynamic_lds(&posterior_logpdf_cached_kernel<false>, (size_t)(lds));
            hipLaunchKernelGGL(posterior_logpdf_cached_kernel<false>, dim3(1), dim3(kSolveThreads), lds, ctx->stream, (int)r, (int)rp, G, Stot,
                               qte, fx, out2, (double *)nullptr);
        } else {
            hipLaunchKernelGGL(posterior_logpdf_cached_kernel<true>, dim3(1), dim3(kSolveThreads), 0, ctx->stream, (int)r, (int)rp, G, Stot, qte,
                               fx, out2, work);
        }
        return GINGR_OK;
    }
    if (in_lds) {
        if (lds > 48 * 1024)  // per function and per device: set whenever needed
            set_dynamic_lds(&posterior_logpdf_lds_kernel<false>, (size_t)(lds));
        hipLaunchKernelGGL(posterior_logpdf_lds_kernel<false>, dim3(1), dim3(kSolveThreads), lds, ctx->stream, (int)r, (int)rp, G, rhs, Stot, qte,
                           fx, out2, (double *)nullptr);
    } else {
        hipLaunchKernelGGL(posterior_logpdf_lds_kernel<true>, dim3(1), dim3(kSolveThreads), 0, ctx->stream, (int)r, (int)rp, G, rhs, Stot, qte, fx,
                           out2, work);
    }
    return GINGR_OK;
}

void launch_posterior_sample_cached(gingr_ctx *ctx, int32_t r, int32_t rp, const double *nfac, const double *a_mean, const double *zrand,
                                    double *a, DevState *st) {
    const size_t lds = lds_solve_doubles(rp, kNB) * sizeof(double);
    if (lds > 48 * 1024)
        set_dynamic_lds(&posterior_sample_cached_kernel, (size_t)(lds));
    hipLaunchKernelGGL(posterior_sample_cached_kernel, dim3(1), dim3(kSolveThreads), lds, ctx->stream, (int)r, (int)rp, nfac, a_mean, zrand, a, st);
}

namespace {
// Binv = (Q^T Q / eps + I)^-1 on the matrix pipe (round 6; until then one workgroup with a column of the inverse per thread: 1.4 ms
// at r = 100, 80 ms at r = 512; then a blocked factor with a column per thread behind it: 11 ms at r = 512).  The system with an
// identity below it goes through the multi-workgroup blocked Cholesky, which leaves L^-T in place of the identity, and the inverse is
// one product of that triangle with itself (dense_spd.hip dense_spd_inverse).
struct BinvElem {  // M = Q^T Q / eps + I (identity on the padding; below it the identity the inverse grows from)
    const double *__restrict__ S;
    int rp;
    __device__ double operator()(int64_t row, int64_t c) const { return S[row * rp + c] / GINGR_COEFF_NOISE + (row == c ? 1.0 : 0.0); }
};
// Binv [rp][rp]: the r x r block of C, zero on the padding
__global__ __launch_bounds__(256) void binv_store_kernel(int r, int rp, int64_t Mp, const double *__restrict__ C, double *__restrict__ Binv) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rp * rp) return;
    const int row = idx / rp, c = idx - row * rp;
    Binv[idx] = (row < r && c < r) ? C[(int64_t)row * Mp + c] : 0.0;
}
}  // namespace

int64_t binv_work_doubles(int32_t rp) {
    return DenseSpdWork::doubles(rp, DenseSpdWork::kIdentity, true);  // the system over the identity, the product, the inverses of the diagonal blocks
}

void launch_binv(gingr_ctx *ctx, int32_t r, int32_t rp, const double *S, double *work, double *Binv, int32_t *err_flag) {
    const DenseSpdWork ws(rp, DenseSpdWork::kIdentity, true);
    const int64_t Mp = ws.Mp;
    double *Aw = work + ws.aw(), *C = work + ws.c(), *Linv = work + ws.linv();
    launch_spd_system(ctx->stream, (int)r, ws, BinvElem{S, (int)rp}, SpdIdentityBorder{}, Aw, err_flag);
    dense_spd_inverse(ctx, Aw, Mp, Linv, C, err_flag);
    hipLaunchKernelGGL(binv_store_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp, 256)), dim3(256), 0, ctx->stream, (int)r, (int)rp, Mp, C, Binv);
}


void launch_coeff_solve(gingr_ctx *ctx, int32_t r, int32_t rp, const double *Binv, const double *p, double *out) {
    hipLaunchKernelGGL(coeff_solve_kernel, dim3((unsigned)ceil_div(rp, 16)), dim3(256), 0, ctx->stream, (int)r, (int)rp, Binv,
                       p, out);
}
