// Building blocks of the one-workgroup Cholesky solves (gp.hip, chol_block64_kernel of dense_spd.hip): DPP and MFMA
// steps on a bordered matrix in LDS or in an L2-resident workspace.  Device only, internal to libgingr_hip.so.
#pragma once

#include "common.h"
#include "gp_device.h"

// ------------------------------------------------------------------------------------------------- small dense
// Blocked Cholesky solve in one workgroup (256 threads = one wave per SIMD, 16-wide panels); the bordered matrix is LDS resident
// for r <= 128 and lives in an L2-resident global workspace above that (same code through flat addressing).
// With one wave per SIMD the kernel is bound by the NUMBER of instructions it issues (5-8 cycles each), so everything is
// laid out to need no masks: the matrix is padded with an identity to n = rp (a multiple of 16: every panel is full), right-hand
// sides ride along as 16 extra rows of the bordered matrix (so the forward substitution is a by-product of the panel solves
// and trailing updates), loads are unconditional, and the three stages of a panel use the cross-lane hardware directly:
//   (1) wave 0 factors the 16x16 diagonal block in registers, one row per lane; the rank-1 updates fetch the pivot column
//       through the DPP of the FMA itself (v_fmac_f64_dpp row_newbcast) -- no LDS, no scalar round trip on the chain,
//   (2) the panel below it is solved by 16 lanes per matrix row with the same DPP recurrence, four rows interleaved,
//   (3) the trailing update runs on the matrix pipe, one wave per 16x16 tile (v_mfma_f64_16x16x4).
// The backward substitution is blocked the same way.  3 workgroup barriers per panel.
constexpr int kNB = 16;

// stage clock of tools/ubench_solve.hip (accumulates shader cycles per stage); nothing in the library build
#ifndef GINGR_STAGE_CLOCK
#define GINGR_STAGE_CLOCK(slot)
#endif


// value of lane J of the caller's 16-lane row, in every lane of that row: one v_mov_b64_dpp (gfx90a+ row_newbcast) instead of
// two v_readlane_b32 through the scalar file.  A VGPR written by a VALU instruction may be read through DPP only two wait
// states later and the compiler does not look into inline asm, hence the s_nop inside the statement.
template <int J>
__device__ __forceinline__ double row_bcast(double v) {
    double out;
    asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(v), "n"(J));
    return out;
}

// acc += (lane J's a) * b, one v_fmac_f64_dpp.  FRESH = true puts the two wait states into the same asm statement (use it
// whenever `a` could have been produced by the preceding instructions).
template <int J, bool FRESH>
__device__ __forceinline__ void fmac_row_bcast(double &acc, double a, double b) {
    if (FRESH)
        asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                     : "+v"(acc)
                     : "v"(a), "v"(b), "n"(J));
    else
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(b), "n"(J));
}

// One step of the panel recurrence for four interleaved matrix rows: t_u = x_u * rdl (lane K: the finished x_u[K]), then
// x_u += (lane K's t_u) * nl.  One asm statement: the four products are written four instructions before the DPP reads them, which
// covers the two wait states the DPP needs without any s_nop (the compiler cannot be trusted to keep plain multiplies away from
// an asm that follows them).
template <int K>
__device__ __forceinline__ void panel_step4(double (&x)[4], double rdl, double nl) {
    double t0, t1, t2, t3;
    asm volatile(
        "v_mul_f64 %4, %0, %8\n\t"
        "v_mul_f64 %5, %1, %8\n\t"
        "v_mul_f64 %6, %2, %8\n\t"
        "v_mul_f64 %7, %3, %8\n\t"
        "v_fmac_f64_dpp %0, %4, %9 row_newbcast:%10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %5, %9 row_newbcast:%10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %2, %6, %9 row_newbcast:%10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %3, %7, %9 row_newbcast:%10 row_mask:0xf bank_mask:0xf"
        : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
        : "v"(rdl), "v"(nl), "n"(K));
}

// sum over the 16-lane row of the caller, the same bits in every lane of the row: the butterfly 1, 2, 4, 8 on the DPP crossbar
// (quad permutes, half-row mirror, row mirror) -- __shfl_xor goes through ds_bpermute (~100 cycles per step), which is too long for
// the one-workgroup kernels where it sits on the critical path
__device__ __forceinline__ double row16_sum_dpp(double v) {
    auto step = [&](auto ctrl) {
        constexpr int c = decltype(ctrl)::value;
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, c, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), c, 0xf, 0xf, false);
        v += __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    };
    step(std::integral_constant<int, 0xB1>{});   // quad_perm [1, 0, 3, 2]
    step(std::integral_constant<int, 0x4E>{});   // quad_perm [2, 3, 0, 1]
    step(std::integral_constant<int, 0x141>{});  // row_half_mirror
    step(std::integral_constant<int, 0x140>{});  // row_mirror
    return v;
}

// ---- building blocks: all 256 threads call them.  A is (n + xr) x n in LDS, n and xr multiples of 16, odd leading dimension ld.

// doubles of LDS the blocks need for an r x r system with xr extra rows
__host__ __device__ inline int solve_ld(int n) { return n | 1; }  // odd leading dimension: column walks hit distinct banks
__host__ __device__ inline size_t lds_solve_doubles(int rp, int xr) { return (size_t)(rp + xr) * solve_ld(rp) + 2 * (size_t)rp; }

// A (lower triangle of the leading r x r) = ca * G + cs * S + ci * I from global r x rp matrices (S may be nullptr), identity
// on the padding r <= i < n.  16 x 16 element blocks, one element per thread and block, eight blocks in flight; the loads are
// unconditional (clamped indices), only the value is selected.
// HAS_S (round 6): whether the second matrix is there is known at every call site -- as a run-time test of the pointer it sat between
// the loads of the two matrices for each of the 36 blocks, and the request of the next block waited for the previous block's value
// (one memory round trip per block: 19k cycles of the transition-density kernel's 93k, tools/ubench_logpdf_split.hip).
// cols != nullptr (the LDS-resident case only): row / column i of the system is row / column cols[i] of G, whose row stride is ldg --
// one class of a coordinate-separable model out of the dense matrix (gp.h: SepMap); MAXB bounds n / 16 (blocks requested).
template <int NT, bool HAS_S = false, int MAXB = 8>
__device__ __forceinline__ void lds_load_spd(double *A, int ld, int r, int n, const double *__restrict__ G, double ca,
                                             const double *__restrict__ S, double cs, double ci, const int32_t *__restrict__ cols = nullptr,
                                             int ldg = 0) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    constexpr int RB = NT / 16;  // rows per block of 16 columns: one element per thread and block
    if (RB == 16 && n <= 16 * MAXB) {
        // The LDS-resident case: all (at most 36) lower blocks are requested before the first value is used.  A lone workgroup
        // sees the full memory latency per dependent batch; with batches of eight blocks this stage was four round trips.
        double v[MAXB * (MAXB + 1) / 2], vs[HAS_S ? MAXB * (MAXB + 1) / 2 : 1];
        int idx = 0;
#pragma unroll
        for (int bi = 0; bi < MAXB; ++bi)
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj, ++idx) {
                const int i = bi * 16 + ty, j = bj * 16 + tx;
                int g = min(min(i, r - 1), n - 1) * n + min(j, r - 1);  // the global matrices have row stride rp == n
                if (cols) g = cols[min(min(i, r - 1), n - 1)] * ldg + cols[min(j, r - 1)];
                v[idx] = G[g];  // (blocks past n: a clamped, valid address; the value is not stored)
                if (HAS_S) vs[idx] = S[g];
            }
        idx = 0;
#pragma unroll
        for (int bi = 0; bi < MAXB; ++bi)
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj, ++idx) {
                double t = ca * v[idx];
                if (HAS_S) t = __builtin_fma(cs, vs[idx], t);
                v[idx] = t;
            }
        idx = 0;
#pragma unroll
        for (int bi = 0; bi < MAXB; ++bi)
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj, ++idx) {
                const int i = bi * 16 + ty, j = bj * 16 + tx;
                if (bi * 16 < n && j <= i) {
                    double t = v[idx];
                    if (i == j) t += ci;
                    A[i * ld + j] = (i < r && j < r) ? t : (i == j ? 1.0 : 0.0);
                }
            }
        __syncthreads();
        return;
    }
    int ib = 0, jb = 0;          // block origin (workgroup-uniform)
    while (ib < n) {
        double v[8];
        int off[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = ib + ty, j = jb + tx;
            const int g = min(i, r - 1) * n + min(j, r - 1);  // the global matrices have row stride rp == n
            double t = ca * G[g];
            if (HAS_S) t = __builtin_fma(cs, S[g], t);
            if (i == j) t += ci;
            v[u] = (i < r && j < r) ? t : (i == j ? 1.0 : 0.0);
            off[u] = (ib < n && i < n && j <= i) ? i * ld + j : -1;
            jb += 16;
            if (jb > ib + RB - 16 || jb >= n) {  // past the last column any row of this block needs
                jb = 0;
                ib += RB;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (off[u] >= 0) A[off[u]] = v[u];
    }
    __syncthreads();
}

// in-place blocked Cholesky (lower) of the leading n x n; rd[k] = 1 / L[k][k]; *bad_spd (LDS) is set on a non-positive /
// non-finite pivot.  Rows n .. n+xr-1 hold right-hand sides b^T; they ride along through the panel solves and the trailing
// updates (Cholesky of the bordered matrix), so on return they hold (L^-1 b)^T.
// NT threads (a multiple of 256): the panel solves and the trailing updates spread over NT / 64 waves.  With one wave per SIMD
// every stage is bound by the number of instructions that wave issues (~5 cycles each).
// Round 3: look-ahead.  The diagonal block of step k + 1 only needs block COLUMN k + 1 of the trailing update of step k, and it is
// factored by one wave while the others have nothing to do; so the trailing update is split: first the tiles of column k + 1 (all
// waves), then -- behind one more barrier -- wave 0 factors diagonal block k + 1 WHILE waves 1 .. NW-1 update the remaining tiles.
// Per step max(diagonal block, remaining tiles) replaces their sum: 79k -> 67k cycles at r = 100 (tools/ubench_solve.hip), 38 -> 33 us.
// wr (round 4): that many further rows behind the xr bordered ones take part in the panel solves ONLY (no trailing update).  Set to
// the tiled identity (row c: ones in the columns c, 16 + c, 32 + c, ...) they come back holding W_k = L_kk^-T, the transposed inverse
// of every diagonal block, in the columns of block k -- what lds_backward_w multiplies with instead of running the 16-step recurrence.
// IDENT (round 6; chol_block64_kernel): the xr = n extra rows are the identity (they come back as L^-1).  Row n + c then stays zero in
// every column left of c, so panel kb only has to carry the rows n .. n + kb + 16: the others' panel solves and trailing updates are
// multiplications by zero (62 % of the riding work of four panels instead of all of it).
template <int NT, bool IDENT = false>
__device__ __forceinline__ void lds_cholesky(double *A, int ld, int n, double *rd, int *bad_spd, int xr, int wr = 0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;           // waves
    constexpr int PU = NT >= 1024 ? 2 : 4;  // matrix rows interleaved per 16-lane group in the panel solve
    constexpr int PR = (NT / 16) * PU;     // matrix rows per panel pass
    const int rows_all = n + xr;
    // (1) diagonal block in registers, ONE wave (all four 16-lane rows do the same work: DPP needs the source lanes active).
    // No masks anywhere: the upper part of the block is loaded, carried and stored as it comes -- lane i's entries right of the
    // diagonal only ever feed lane i's own entries right of the diagonal, and nobody reads the upper part of A (the selects,
    // compares and exec-mask juggling of a masked version were a third of this stage's instructions).  The stage is bound by
    // the NUMBER of instructions the one wave issues, not by the dependent chain: a fraction-free variant (no reciprocal square
    // root on the chain, one more multiply per entry) measured slower, 24.5k against 21.4k cycles for seven blocks.
    auto diag_block = [&](int kb) {
        const int l15 = lane & 15;
        double row[kNB];
#pragma unroll
        for (int k = 0; k < kNB; ++k) row[k] = A[(kb + l15) * ld + kb + k];
        static_for<0, kNB>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            // the pivot, from lane c of this 16-lane row.  A non-positive or non-finite pivot is not tested here (the test
            // would sit on the sequential chain): it turns lc into NaN (rsq(d <= 0) * d, rsq(inf) * inf), the NaN reaches every
            // later diagonal entry of the block, and the check after the loop sees it.
            const double d = row_bcast<c>(row[c]);
            // 1/sqrt(d) by v_rsq_f64 + two Newton steps; lane c's own element d * rsqrt(d) is sqrt(d): the IEEE sqrt and
            // divide sequences are ~40 dependent instructions and would sit on the sequential chain of every column
            double rdk = __builtin_amdgcn_rsq(d);
            const double hd = 0.5 * d;
            rdk = rdk * __builtin_fma(-hd * rdk, rdk, 1.5);
            rdk = rdk * __builtin_fma(-hd * rdk, rdk, 1.5);
            const double lc = row[c] * rdk;
            const double nlc = -lc;
            row[c] = lc;
            rd[kb + c] = rdk;  // 1 / L[c][c]; the same value from every lane
            // row[j] -= L[lane][c] * L[j][c]: L[j][c] is lane j's lc, fetched by the DPP of the FMA itself
            static_for<c + 1, kNB>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                fmac_row_bcast<j, j == c + 1>(row[j], lc, nlc);
            });
        });
        if (lane < kNB) {
#pragma unroll
            for (int k = 0; k < kNB; ++k) A[(kb + lane) * ld + kb + k] = row[k];
            // L[lane][lane] = row[lane]: a register array cannot be indexed by the lane; read it back
            const double diag = A[(kb + lane) * ld + kb + lane];
            if (!(diag > 0.0) || !finite_d(diag)) *bad_spd = 1;
        }
    };
    // (3) one 16x16 tile of the trailing update on the matrix pipe: D = C - L_I L_J^T as four v_mfma_f64_16x16x4 (k = 16).
    // Fragment layout as in gram_kernel: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; it holds
    // D[i = (l >> 4) + 4 reg][j = l & 15].  All tiles are full; the upper half of a diagonal tile is updated too (nobody reads it).
    // (measured in round 2: bound by the LDS traffic of the fragments -- C in, A, B, C out = 8 KB per tile -- not by latency)
    auto tile_update = [&](int kb, int ti, int tj) {
        const int t0 = kb + kNB;
        const int l15 = lane & 15, l4 = lane >> 4;
        const int i0 = t0 + 16 * ti, j0 = t0 + 16 * tj;
        const double *pa = A + (i0 + l15) * ld + kb + l4, *pb = A + (j0 + l15) * ld + kb + l4;
        double *pc = A + (i0 + l4) * ld + j0 + l15;
        v4f64 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = pc[4 * g * ld];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * q], pb[4 * q], acc, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) pc[4 * g * ld] = acc[g];
    };
    if (wave == 0) diag_block(0);
    __syncthreads();
    for (int kb = 0; kb < n; kb += kNB) {
        const int rows = IDENT ? n + min(xr, kb + kNB) : rows_all, prows = rows + wr;
        GINGR_STAGE_CLOCK(1)
        // (2) panel below the diagonal block: x L11^T = A[i][kb:kb+16].  Sixteen lanes per matrix row: lane c keeps x[c] and
        // row c of L11 in registers; at step k every lane with c > k takes x[k] / L[k][k] from lane k through the DPP of its
        // FMA.  No LDS traffic inside the recurrence; four matrix rows per 16-lane group are interleaved to fill the chain.
        {
            const int grp = tid >> 4, c16 = tid & 15;
            double nL[kNB];  // -L11[c16][k] for k < c16, else 0 (lanes c <= k must not move)
#pragma unroll
            for (int k = 0; k < kNB; ++k) {
                const double v = A[(kb + c16) * ld + kb + k];
                nL[k] = k < c16 ? -v : 0.0;
            }
            const double rdl = rd[kb + c16];
            for (int ib = kb + kNB; ib < prows; ib += PR) {  // workgroup-uniform trip count
                const int i0 = ib + grp;
                double x[PU];
#pragma unroll
                for (int u = 0; u < PU; ++u) x[u] = A[min(i0 + (NT / 16) * u, prows - 1) * ld + kb + c16];
                static_for<0, kNB>([&](auto kk) {
                    constexpr int k = decltype(kk)::value;
                    if constexpr (PU == 4) {
                        panel_step4<k>(x, rdl, nL[k]);
                    } else {
                        double t[PU];
#pragma unroll
                        for (int u = 0; u < PU; ++u) t[u] = x[u] * rdl;  // lane k: the finished x[k]
#pragma unroll
                        for (int u = 0; u < PU; ++u) fmac_row_bcast<k, true>(x[u], t[u], nL[k]);
                    }
                });
#pragma unroll
                for (int u = 0; u < PU; ++u)
                    if (i0 + (NT / 16) * u < prows) A[(i0 + (NT / 16) * u) * ld + kb + c16] = x[u] * rdl;
            }
        }
        __syncthreads();
        GINGR_STAGE_CLOCK(2)
        const int t0 = kb + kNB;
        const int nti = (rows - t0) >> 4, ntj = (n - t0) >> 4;
        // (3a) block column kb + 16 of the trailing matrix (tj = 0): what the next diagonal block and the next panel read
        if (ntj > 0)
            for (int ti = wave; ti < nti; ti += NW) tile_update(kb, ti, 0);
        __syncthreads();
        // (3b) wave 0 factors the next diagonal block while the other waves update the remaining tiles (tj >= 1).  One wave only
        // (NW == 1): everything in sequence.
        if (wave == 0 && ntj > 0) diag_block(t0);
        if (NW == 1 || wave > 0) {
            constexpr int NR = NW > 1 ? NW - 1 : 1;
            const int me = NW > 1 ? wave - 1 : 0;
            int tcount = 0;
            for (int ti = 1; ti < nti; ++ti)
                for (int tj = 1; tj <= ti && tj < ntj; ++tj, ++tcount)
                    if (tcount % NR == me) tile_update(kb, ti, tj);  // wave-uniform
        }
        __syncthreads();
        GINGR_STAGE_CLOCK(3)
    }
}

// y <- L^-T y for the n entries of y (blocked, bottom up; the 16x16 triangular solves run in registers of wave 0 with the DPP
// recurrence: lane c holds column c of the diagonal block)
template <int NT>
__device__ __forceinline__ void lds_backward(const double *A, int ld, int n, const double *rd, double *y) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int kb = n - kNB; kb >= 0; kb -= kNB) {
        if (wave == 0) {
            const int l15 = lane & 15;
            double ncol[kNB];  // -L11[k][lane] for k > lane, else 0 (lanes >= k must not move at step k)
#pragma unroll
            for (int k = 0; k < kNB; ++k) {
                const double v = A[(kb + k) * ld + kb + l15];
                ncol[k] = k > l15 ? -v : 0.0;
            }
            double yv = y[kb + l15];
            const double rdl = rd[kb + l15];
            static_for<0, kNB>([&](auto cc) {
                constexpr int c = kNB - 1 - decltype(cc)::value;
                const double t = yv * rdl;  // lane c: x_c (its yv is complete)
                fmac_row_bcast<c, true>(yv, t, ncol[c]);
            });
            if (lane < kNB) y[kb + lane] = yv * rdl;
        }
        __syncthreads();
        for (int i = tid; i < kb; i += NT) {
            double sacc = y[i];
#pragma unroll
            for (int k = 0; k < kNB; ++k) sacc = __builtin_fma(-A[(kb + k) * ld + i], y[kb + k], sacc);
            y[i] = sacc;
        }
        __syncthreads();
    }
}

// x = L^-T y with the transposed inverses of the diagonal blocks at hand (lds_cholesky, wr = 16: W points at the first identity row,
// W[c * ld + kb + j] = (L_kk^-T)[c][j], exact zeros left of the diagonal).  Per block a 16 x 16 mat-vec (one product per thread, DPP
// row sum) replaces the 16-step sequential recurrence of lds_backward, and x goes to its own array so that one barrier per stage is
// enough: 12k -> see tools/ubench_solve.hip (cycles of seven blocks at r = 100).  NT == 256; y is destroyed.
template <int NT>
__device__ __forceinline__ void lds_backward_w(const double *A, int ld, int n, const double *W, double *y, double *x) {
    static_assert(NT == 256, "one product of the 16 x 16 block per thread");
    const int tid = threadIdx.x, c = tid >> 4, j = tid & 15;
    for (int kb = n - kNB; kb >= 0; kb -= kNB) {
        const double p = row16_sum_dpp(W[c * ld + kb + j] * y[kb + j]);
        if (j == 0) x[kb + c] = p;
        __syncthreads();
        if (tid < kb) {  // y[i] -= sum_k L[kb + k][i] x[kb + k]: two interleaved chains of eight
            double s0 = y[tid], s1 = 0.0;
#pragma unroll
            for (int k = 0; k < kNB; k += 2) {
                s0 = __builtin_fma(-A[(kb + k) * ld + tid], x[kb + k], s0);
                s1 = __builtin_fma(-A[(kb + k + 1) * ld + tid], x[kb + k + 1], s1);
            }
            y[tid] = s0 + s1;
        }
        __syncthreads();
    }
}

// y <- L^-1 y for the n entries of y (blocked, top down): the mirror image of lds_backward -- lane c of wave 0 holds ROW c of the
// diagonal block, at step c every lane below takes x_c from lane c through the DPP of its FMA.
template <int NT>
__device__ __forceinline__ void lds_forward(const double *A, int ld, int n, const double *rd, double *y) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int kb = 0; kb < n; kb += kNB) {
        if (wave == 0) {
            const int l15 = lane & 15;
            double nrow[kNB];  // -L11[lane][k] for k < lane, else 0 (lanes <= k must not move at step k)
#pragma unroll
            for (int k = 0; k < kNB; ++k) {
                const double v = A[(kb + l15) * ld + kb + k];
                nrow[k] = k < l15 ? -v : 0.0;
            }
            double yv = y[kb + l15];
            const double rdl = rd[kb + l15];
            static_for<0, kNB>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                const double t = yv * rdl;  // lane c: x_c (its yv is complete)
                fmac_row_bcast<c, true>(yv, t, nrow[c]);
            });
            if (lane < kNB) y[kb + lane] = yv * rdl;
        }
        __syncthreads();
        for (int i = kb + kNB + tid; i < n; i += NT) {
            double sacc = y[i];
#pragma unroll
            for (int k = 0; k < kNB; ++k) sacc = __builtin_fma(-A[i * ld + kb + k], y[kb + k], sacc);
            y[i] = sacc;
        }
        __syncthreads();
    }
}

// nrows x ncols (ncols <= 128) doubles from a row-major global matrix into the LDS matrix A, sixteen loads per thread requested
// before the first store (round 6: as a plain load-store loop each element waits for its own memory round trip -- the lone
// workgroup of these kernels has nothing else to hide it behind; chol_block64_kernel's copy went from 8.6k to 2.8k cycles this way)
template <int NT>
__device__ __forceinline__ void lds_fill_rows(double *A, int ld, const double *__restrict__ src, int64_t ld_src, int nrows, int ncols) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int NW = NT / 64;
    for (int i0 = w; i0 < nrows; i0 += NW * 8) {  // (workgroup-uniform trip count)
        double v[8][2];
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = i0 + NW * q, j = l + 64 * h;
                v[q][h] = (i < nrows && j < ncols) ? src[(int64_t)i * ld_src + j] : 0.0;
            }
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = i0 + NW * q, j = l + 64 * h;
                if (i < nrows && j < ncols) A[i * ld + j] = v[q][h];
            }
    }
}

// Threads of the one-workgroup solve kernels.  Measured (tools/ubench_solve.hip, r = 100): 1024 threads shorten the load stage
// (9.9k -> 6.8k cycles) but lengthen the trailing update (25k -> 37k: every wave walks the whole tile list) and leave the panel
// solve where it is (its per-thread set-up is replicated in four times the waves): 46 us against 42 us at 256 threads.
constexpr int kSolveThreads = 256;
