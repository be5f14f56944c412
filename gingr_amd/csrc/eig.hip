// Eigen-decomposition of a small symmetric positive semi-definite matrix (n <= 192) with the matrix in REGISTERS.
//
// What it replaces: the breeze eigSym(L^T L) inside scalismo's LowRankGaussianProcess.approximateGPCholesky (the Karhunen-Loeve
// basis of a kernel model: G/api/registration/utils/GPMMHelper.scala:39-69, E/CreateBunnyGPMM.scala), and the eigenbasis of the
// model's moment S_tot = Q^T Q the uniform-weight posterior uses (gp.hip posterior_solve_eig_kernel).
//
// The two-sided cyclic Jacobi it takes over from (sym_eig.hip jacobi_eig_kernel, still the path above n = 192 and for numerically
// singular matrices) keeps A and V in global memory and spends a round trip to L2 per load-store of every rotation round: 40 us a
// round at n = 171, 61 ms a decomposition.  Here:
//   * G = C C^T first (right-looking Cholesky, a column at a time through LDS), then the ONE-SIDED (Hestenes) Jacobi on the columns
//     of C: rotations from the right make the columns of C V mutually orthogonal, so they are the eigenvectors of G scaled by the
//     roots of the eigenvalues -- eigenvalue = squared length, eigenvector = normalised column, no V to accumulate, and the
//     accuracy is governed by the condition number of C (the root of G's).  A failed pivot leaves the columns of G itself to rotate
//     (eigenvalue = length), and info[1] reports the matrix as numerically singular: the callers then take the two-sided kernel,
//     whose V starts from the identity and is complete whatever the spectrum.
//   * a column lives in the registers of ONE wave, E values per lane (row = e * 64 + lane); a wave owns P pairs of columns;
//   * a round = ONE dot product per pair (the squared norms travel with the columns, updated by the rotation formulas and
//     recomputed once a sweep), summed for all P pairs at once by v_permlane32_swap / v_permlane16_swap + DPP so that the lanes
//     8 j .. 8 j + 7 hold pair j's; these lanes work out the rotation (two v_rsq_f64 with Newton steps instead of three divisions
//     and three roots), which reaches the wave through scalar registers; then the round-robin tournament moves every column one
//     place: inside a wave a register rename, between neighbouring waves one column each way through LDS -- one barrier per round,
//     two LDS buffers;
//   * 16 waves x 6 pairs x 2 columns = 192 columns of 192 rows at most; one workgroup per problem: up to three problems by pointer
//     (sym_eig_cols_kernel) or any number of one size at fixed strides (sym_eig_cols_strided_kernel) per launch.
// Rotation threshold |p.q| > sqrt(n) eps |p| |q| (LAPACK dgesvj's), at most 60 sweeps (8 at n = 171; the two-sided kernel needs 10).
// n = 34 / 100 / 171: 0.26 / 1.3 / 3.2 ms (tools/ubench_sym_eig.hip, profiles/r06_ubench_sym_eig.txt).
#include "gp.h"

namespace {

constexpr int kEigSlots = 192;  // columns a workgroup holds at most (2 x waves x pairs per wave)

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// sum over the 64 lanes, the same bits in every lane (every step adds a value to its mirror image: a + b == b + a)
__device__ __forceinline__ double wave_allsum(double v) {
    v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);  // row_half_mirror
    v += dpp_f64<0x140>(v);  // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}


__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// x[l] + x[l ^ 32] of `lo` in the lanes 0 .. 31, of `hi` in the lanes 32 .. 63 (v_permlane32_swap: no LDS round trip)
__device__ __forceinline__ double halves_sum32(double lo, double hi) {
    const auto a = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(lo), (unsigned)__double2loint(hi), false, false);
    const auto b = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(lo), (unsigned)__double2hiint(hi), false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}
// x[l] + x[l ^ 16] of `lo` in the rows 0 and 2 (lanes with bit 4 clear), of `hi` in the rows 1 and 3
__device__ __forceinline__ double halves_sum16(double lo, double hi) {
    const auto a = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(lo), (unsigned)__double2loint(hi), false, false);
    const auto b = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(lo), (unsigned)__double2hiint(hi), false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

// v[j], j < P <= 8: one value per pair and lane.  Returns, in the lanes 8 j .. 8 j + 7, the sum of v[j] over the wave (the same bits
// in all eight): halving exchanges over the lane bits 5, 4, 3 (a lane keeps the half of the values its bit selects), then an
// all-reduce over the eight lanes by DPP.
template <int P>
__device__ __forceinline__ double pair_sums(const double (&v)[8], int lane) {
    const bool b3 = lane & 8;
    double u4[4], u2[2], u1;
#pragma unroll
    for (int k = 0; k < 4; ++k) u4[k] = P > 4 ? halves_sum32(v[k], v[4 + k]) : halves_sum32(v[k], v[k]);
#pragma unroll
    for (int k = 0; k < 2; ++k) u2[k] = P > 2 ? halves_sum16(u4[k], u4[2 + k]) : halves_sum16(u4[k], u4[k]);
    {
        const double mine = b3 ? u2[1] : u2[0], theirs = b3 ? u2[0] : u2[1];
        u1 = mine + dpp_f64<0x128>(theirs);  // row_ror:8
    }
    u1 += dpp_f64<0xB1>(u1);   // quad_perm [1,0,3,2]
    u1 += dpp_f64<0x4E>(u1);   // quad_perm [2,3,0,1]
    u1 += dpp_f64<0x141>(u1);  // row_half_mirror
    return u1;
}

// 1 / sqrt(x), x > 0: v_rsq_f64 and two Newton steps (a few ulp; the rotation only needs c^2 + s^2 = 1 to rounding)
__device__ __forceinline__ double rsqrt_nr(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = __builtin_fma(-(h * y), y, 0.5);
        y = __builtin_fma(y, e, y);
    }
    return y;
}

struct EigProblem {
    const double *G;  // n x n, row stride ldg (symmetric: column c is read as row c)
    int32_t ldg, n;
    double *H;       // work: [2 K][n] final columns, K = waves * P positions
    double *norms;   // work: [2 K]
    double *evals;   // out: [n] descending
    double *Vs;      // out: [n][n], eigenvector k in column k
    int32_t *info;   // out: [0] sweeps used, [1] 1 when numerically singular
};
struct EigBatch {
    EigProblem p[3];
};

// `count` problems of one size n at fixed strides (doubles; info: two words per problem), one workgroup each: the folds of
// gingr_pca_leave_one_out (pca_leave_one_out.hip)
struct EigStrided {
    const double *G;
    int64_t g_stride;
    int32_t ldg, n;
    double *work;  // per problem sym_eig_cols_work_doubles(n) doubles: H, then the norms
    int64_t work_stride;
    double *evals;
    int64_t e_stride;
    double *Vs;
    int64_t v_stride;
    int32_t *info;
};

// One decomposition by the workgroup: the body of both entries below
template <int E, int P, int W>
__device__ __forceinline__ void sym_eig_cols_body(const EigProblem &pr) {
    __shared__ double xT[2][W][E * 64], xB[2][W][E * 64];
    __shared__ double nrm[2][2][W * P];  // squared column norms by slot: [.][0] top row, [.][1] bottom row
    __shared__ int32_t rank_of[2 * W * P];
    const int n = pr.n;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // w: scalar
    const int positions = (n + 1) / 2;
    const int waves = (positions + P - 1) / P;  // waves in the ring
    const int K = waves * P;
    const bool in_ring = w < waves;
    const bool last = w == waves - 1;
    const int grp = lane >> 3;                   // the pair whose rotation this lane works out
    const int g = w * P + (grp < P ? grp : 0);   // its slot in the ring
    double top[P][E], bot[P][E];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int ct = w * P + j, cb = K + w * P + j;  // column of G that starts in the slot
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int row = e * 64 + lane;
            top[j][e] = (in_ring && ct < n && row < n) ? pr.G[(int64_t)ct * pr.ldg + row] : 0.0;
            bot[j][e] = (in_ring && cb < n && row < n) ? pr.G[(int64_t)cb * pr.ldg + row] : 0.0;
        }
    }
    // G = C C^T first (right-looking, a column at a time through LDS): the rotations then work on the columns of C, whose
    // condition number is the square root of G's; a pivot that fails (G numerically singular) leaves the columns of G to rotate
    __shared__ double colbuf[2][E * 64];
    __shared__ int32_t chol_failed;
    if (threadIdx.x == 0) chol_failed = 0;
    __syncthreads();
    auto pivot_column = [&](double (&col)[E], int k) {  // column k: scaled by 1 / sqrt(pivot), rows above the pivot zeroed, published
        double dsel = col[0];
#pragma unroll
        for (int e = 1; e < E; ++e)
            if ((k >> 6) == e) dsel = col[e];
        const double d = readlane_f64(dsel, k & 63);
        const bool ok = d > 0.0 && d <= 1.79769313486231570815e308;
        const double rs = ok ? 1.0 / sqrt(d) : 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int row = e * 64 + lane;
            col[e] = row >= k ? col[e] * rs : 0.0;
            colbuf[k & 1][row] = col[e];
        }
        if (!ok && lane == 0) chol_failed = 1;
    };
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (k < K && w * P + j == k) pivot_column(top[j], k);
            if (k >= K && K + w * P + j == k) pivot_column(bot[j], k);
        }
        __syncthreads();
        if (in_ring) {
            double cb[E];
#pragma unroll
            for (int e = 0; e < E; ++e) cb[e] = colbuf[k & 1][e * 64 + lane];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int ct = w * P + j, cbt = K + w * P + j;
                if (ct > k && ct < n) {
                    const double f = colbuf[k & 1][ct];
#pragma unroll
                    for (int e = 0; e < E; ++e) top[j][e] = __builtin_fma(-cb[e], f, top[j][e]);
                }
                if (cbt > k && cbt < n) {
                    const double f = colbuf[k & 1][cbt];
#pragma unroll
                    for (int e = 0; e < E; ++e) bot[j][e] = __builtin_fma(-cb[e], f, bot[j][e]);
                }
            }
        }
    }
    __syncthreads();
    const bool factored = __builtin_amdgcn_readfirstlane(chol_failed) == 0;
    if (factored) {  // the strict upper triangle never held the factor
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int row = e * 64 + lane;
                if (row < w * P + j) top[j][e] = 0.0;
                if (row < K + w * P + j) bot[j][e] = 0.0;
            }
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int ct = w * P + j, cbt = K + w * P + j;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int row = e * 64 + lane;
                top[j][e] = (in_ring && ct < n && row < n) ? pr.G[(int64_t)ct * pr.ldg + row] : 0.0;
                bot[j][e] = (in_ring && cbt < n && row < n) ? pr.G[(int64_t)cbt * pr.ldg + row] : 0.0;
            }
        }
    }
    const double tol2 = (double)n * 2.220446049250313e-16 * 2.220446049250313e-16;
    const int rounds = 2 * K - 1;
    int par = 0, sweep = 0;
    double app = 0.0, aqq = 0.0;  // squared norms of the lane's pair: exact at the start of a sweep, updated by the rotations
    for (; sweep < 60 && n > 1; ++sweep) {
        int rotated = 0;
        for (int rd = 0; rd < rounds; ++rd) {
            if (in_ring) {
                // p . q of every pair, summed so that the lanes 8 j .. 8 j + 7 hold that of pair j; these lanes work out the
                // rotation (all P of them at once), which then reaches the whole wave through scalar registers
                double vpq[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    vpq[j] = 0.0;
                    if (j < P) {
#pragma unroll
                        for (int e = 0; e < E; ++e) vpq[j] = __builtin_fma(top[j][e], bot[j][e], vpq[j]);
                    }
                }
                const double apq = pair_sums<P>(vpq, lane);
                if (rd == 0) {
#pragma unroll 1
                    for (int pass = 0; pass < 2; ++pass) {  // one row of the ring at a time: 16 registers instead of 32
                        double vxx[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            vxx[j] = 0.0;
                            if (j < P) {
#pragma unroll
                                for (int e = 0; e < E; ++e) {
                                    const double x = pass ? bot[j][e] : top[j][e];
                                    vxx[j] = __builtin_fma(x, x, vxx[j]);
                                }
                            }
                        }
                        const double sum = pair_sums<P>(vxx, lane);
                        if (pass)
                            aqq = sum;
                        else
                            app = sum;
                    }
                }
                // tan 2 theta = 2 apq / (aqq - app), |theta| <= pi / 4:  cos 2 theta = |alpha| / r,  sin 2 theta = sign(alpha) beta / r
                double c = 1.0, s = 0.0;
                const double alpha = aqq - app, beta = 2.0 * apq;
                const double r2 = __builtin_fma(alpha, alpha, beta * beta);
                if (apq * apq > tol2 * (app * aqq) && r2 > 0.0) {
                    const double ir = rsqrt_nr(r2);
                    const double c2 = __builtin_fma(0.5 * fabs(alpha), ir, 0.5);
                    const double ic = rsqrt_nr(c2);
                    c = c2 * ic;
                    s = (alpha >= 0.0 ? 0.5 : -0.5) * beta * ir * ic;
                    const double t = s * ic;
                    app = __builtin_fma(-t, apq, app);
                    aqq = __builtin_fma(t, apq, aqq);
                }
                if ((lane & 7) == 0 && grp < P) {
                    nrm[par][0][g] = app;
                    nrm[par][1][g] = aqq;
                }
                // the two columns that leave the wave first
#pragma unroll
                for (int jj = 0; jj < P; ++jj) {
                    const int j = jj == 0 ? P - 1 : jj - 1;
                    const double cj = readlane_f64(c, 8 * j), sj = readlane_f64(s, 8 * j);
                    if (sj != 0.0) {  // wave uniform
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            const double p = top[j][e], q = bot[j][e];
                            top[j][e] = __builtin_fma(cj, p, -(sj * q));
                            bot[j][e] = __builtin_fma(sj, p, cj * q);
                        }
                        rotated = 1;
                    }
                    if (jj == 0) {
#pragma unroll
                        for (int e = 0; e < E; ++e) xT[par][w][e * 64 + lane] = top[P - 1][e];
                    }
                    if (j == 0) {
#pragma unroll
                        for (int e = 0; e < E; ++e) xB[par][w][e * 64 + lane] = bot[0][e];
                    }
                }
            }
            // tournament: slot 0 of the top row stays, everything else moves one place round the ring
            __syncthreads();
            if (in_ring) {
                double inT[E], inB[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    // top slot w P: from the top row's slot w P - 1 (the neighbour's last)
                    inT[e] = w == 0 ? 0.0 : xT[par][w - 1][e * 64 + lane];
                    // bottom slot w P + P - 1: from the bottom row's next slot; the ring's last takes the top row's last
                    inB[e] = last ? top[P - 1][e] : xB[par][w + 1][e * 64 + lane];
                }
#pragma unroll
                for (int j = P - 1; j >= 1; --j)
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const bool from_bottom = w == 0 && j == 1;  // slot 1 of the ring takes the bottom row's slot 0
                        top[j][e] = from_bottom ? bot[0][e] : top[j - 1][e];
                    }
                if (w != 0) {
#pragma unroll
                    for (int e = 0; e < E; ++e) top[0][e] = inT[e];
                }
#pragma unroll
                for (int j = 0; j < P - 1; ++j)
#pragma unroll
                    for (int e = 0; e < E; ++e) bot[j][e] = bot[j + 1][e];
#pragma unroll
                for (int e = 0; e < E; ++e) bot[P - 1][e] = inB[e];
                // the norms follow their columns
                app = g == 0 ? nrm[par][0][0] : (g == 1 ? nrm[par][1][0] : nrm[par][0][g - 1]);
                aqq = g == K - 1 ? nrm[par][0][K - 1] : nrm[par][1][g + 1];
            }
            par ^= 1;
        }
        if (!__syncthreads_or(rotated)) {
            ++sweep;
            break;
        }
    }
    // columns and their norms to the work area; rank sort (descending, ties in slot order); normalised columns out
    if (in_ring) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int st = w * P + j, sb = K + w * P + j;
            double nt = 0.0, nb = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                nt = __builtin_fma(top[j][e], top[j][e], nt);
                nb = __builtin_fma(bot[j][e], bot[j][e], nb);
                const int row = e * 64 + lane;
                if (row < n) {
                    pr.H[(int64_t)st * n + row] = top[j][e];
                    pr.H[(int64_t)sb * n + row] = bot[j][e];
                }
            }
            nt = wave_allsum(nt);
            nb = wave_allsum(nb);
            if (lane == 0) {  // eigenvalue: the squared length of a column of C V, the length of one of G V
                pr.norms[st] = factored ? nt : sqrt(nt);
                pr.norms[sb] = factored ? nb : sqrt(nb);
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    const int slots = 2 * K;
    for (int i = threadIdx.x; i < slots; i += W * 64) {
        const double li = pr.norms[i];
        int rank = 0;
        for (int j = 0; j < slots; ++j) {
            const double lj = pr.norms[j];
            rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
        rank_of[i] = rank;
        if (rank < n) pr.evals[rank] = li;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double mx = 0.0, mn = __builtin_huge_val();
        for (int i = 0; i < slots; ++i)
            if (rank_of[i] < n) {
                mx = fmax(mx, pr.norms[i]);
                mn = fmin(mn, pr.norms[i]);
            }
        pr.info[0] = sweep;
        pr.info[1] = (!factored || !(mn > (double)n * 2.220446049250313e-16 * mx)) ? 1 : 0;
    }
    for (int idx = threadIdx.x; idx < slots * n; idx += W * 64) {
        const int i = idx / n, row = idx - i * n;
        const int rank = rank_of[i];
        if (rank >= n) continue;
        const double len = factored ? sqrt(pr.norms[i]) : pr.norms[i];
        pr.Vs[(int64_t)row * n + rank] = len > 0.0 ? pr.H[idx] / len : 0.0;
    }
}

template <int E, int P, int W>
__global__ __launch_bounds__(W * 64) void sym_eig_cols_kernel(EigBatch batch) {
    const EigProblem pr = batch.p[blockIdx.x];
    sym_eig_cols_body<E, P, W>(pr);
}

template <int E, int P, int W>
__global__ __launch_bounds__(W * 64) void sym_eig_cols_strided_kernel(EigStrided s) {
    const int64_t q = blockIdx.x;
    double *work = s.work + q * s.work_stride;
    const EigProblem pr{s.G + q * s.g_stride, s.ldg, s.n, work, work + (int64_t)kEigSlots * s.n, s.evals + q * s.e_stride, s.Vs + q * s.v_stride,
                        s.info + 2 * q};
    sym_eig_cols_body<E, P, W>(pr);
}

// ---- 193 .. 512 columns: the same decomposition (Cholesky, then one-sided Jacobi on the factor's columns) on many workgroups ----
//
// The register kernel ends at 192 columns (one workgroup's registers); the two-sided grid kernel of sym_eig.hip that served everything
// larger meets its 64 workgroups at a spin-wait barrier once a round.  Here every step is a launch of its own and the workgroups of
// a launch never wait for each other:
//   * the factor C (G = C C^T) is kept column-major, [columns padded to blocks of 16][rows padded to 64], zero padded;
//   * Cholesky right-looking in panels of 16 columns: one workgroup factors the panel, a grid applies its rank-16 update;
//   * a sweep is nblk - 1 launches (round-robin tournament of the nblk column blocks).  A workgroup owns one pair of blocks: it
//     takes their 32 columns into LDS (at most 32 x 512 x 8 B = 128 KB), and its 16 waves rotate 16 disjoint column pairs at a
//     time -- the 16 cross rounds (column i of one block against column i + s of the other), or, in the first launch of a sweep,
//     the 31 rounds of a full tournament of the 32 columns, which also meets the pairs inside a block: every pair of columns
//     once a sweep.  A pair's three dot products are summed by DPP (wave_allsum), the rotation is the register kernel's;
//   * launches count the rotations of a sweep in a word of their own; the host stops after a sweep without one;
//   * up to three problems side by side (blockIdx.y): the coordinate blocks of one model differ by at most one column.
// Eigenvalue = squared column length, eigenvector = normalised column, as above.  A failed Cholesky pivot or a numerically singular
// spectrum is reported in info[1]; the caller then takes the two-sided kernel, as it does for the register kernel.
constexpr int kEbCols = 16;      // columns of a block
constexpr int kEbThreads = 1024;  // 16 waves: one column pair each

struct EigbBatch {
    double *X[3];      // [nblk * 16][ldx]
    int32_t n[3];
};

__global__ __launch_bounds__(256) void eigb_load_kernel(EigbBatch b, const double *G0, const double *G1, const double *G2, int32_t ld0,
                                                        int32_t ld1, int32_t ld2, int32_t ldx, int32_t cols) {
    const int q = blockIdx.y;
    const double *G = q == 0 ? G0 : (q == 1 ? G1 : G2);
    const int ldg = q == 0 ? ld0 : (q == 1 ? ld1 : ld2);
    const int n = b.n[q];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cols * ldx) return;
    const int c = idx / ldx, r = idx - c * ldx;
    b.X[q][idx] = (c < n && r < n) ? G[(int64_t)c * ldg + r] : 0.0;  // (symmetric: column c is read as row c)
}

// columns k0 .. k0 + 15 of the factor, rows from the diagonal down; the rows above the diagonal are cleared at the end
__global__ __launch_bounds__(kEbThreads) void eigb_chol_panel_kernel(EigbBatch b, int32_t ldx, int32_t k0, int32_t *__restrict__ failed) {
    const int q = blockIdx.x;
    const int n = b.n[q];
    double *X = b.X[q];
    const int t = threadIdx.x;
    const int k1 = min(k0 + kEbCols, n);
    for (int j = k0; j < k1; ++j) {
        __syncthreads();
        const double d = X[(int64_t)j * ldx + j];
        const bool ok = d > 0.0 && d <= 1.79769313486231570815e308;
        const double rs = ok ? 1.0 / sqrt(d) : 0.0;
        __syncthreads();
        if (!ok && t == 0) failed[q] = 1;
        for (int r = j + t; r < n; r += kEbThreads) X[(int64_t)j * ldx + r] *= rs;
        __syncthreads();
        const int rows = n - j - 1;  // rows j + 1 .. n - 1 of the columns j + 1 .. k1 - 1
        for (int idx = t; idx < (k1 - j - 1) * rows; idx += kEbThreads) {
            const int c = j + 1 + idx / rows, r = j + 1 + idx % rows;
            if (r >= c) X[(int64_t)c * ldx + r] = __builtin_fma(-X[(int64_t)j * ldx + r], X[(int64_t)j * ldx + c], X[(int64_t)c * ldx + r]);
        }
    }
    __syncthreads();
    for (int idx = t; idx < (k1 - k0) * n; idx += kEbThreads) {
        const int c = k0 + idx / n, r = idx % n;
        if (r < c) X[(int64_t)c * ldx + r] = 0.0;
    }
}

// X[c][r] -= sum_{k0 <= k < k0 + 16} X[k][r] X[k][c]   for the columns c >= k0 + 16 (blockIdx.y), rows r >= c
__global__ __launch_bounds__(256) void eigb_chol_update_kernel(EigbBatch b, int32_t ldx, int32_t k0) {
    const int q = blockIdx.z;
    const int n = b.n[q];
    double *X = b.X[q];
    const int c = k0 + kEbCols + blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (c >= n || r >= n || r < c) return;
    double acc = X[(int64_t)c * ldx + r];
#pragma unroll
    for (int k = 0; k < kEbCols; ++k) acc = __builtin_fma(-X[(int64_t)(k0 + k) * ldx + r], X[(int64_t)(k0 + k) * ldx + c], acc);
    X[(int64_t)c * ldx + r] = acc;
}

// One launch of the tournament of column blocks: workgroup (m, q) rotates the columns of its pair of blocks of problem q against
// each other.  E = ldx / 64 values of a column per lane.  `full`: all pairs of the 32 columns, not only the cross pairs.  A problem
// whose Cholesky pivot failed (`failed[q]`) holds no factor to rotate: its workgroups return at once.
template <int E>
__global__ __launch_bounds__(kEbThreads) void eigb_round_kernel(EigbBatch b, int32_t nblk, int32_t rd, int32_t full,
                                                                int32_t *__restrict__ rotations, const int32_t *__restrict__ failed) {
    extern __shared__ double eb_cols[];  // [32][E * 64]
    constexpr int ldx = E * 64;
    const int q = blockIdx.y;
    if (failed[q]) return;  // (uniform over the workgroup, before its first barrier)
    const int n = b.n[q];
    double *X = b.X[q];
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ba = m == 0 ? nblk - 1 : (rd + m) % (nblk - 1), bb = (rd + nblk - 1 - m) % (nblk - 1);
    if ((full ? min(ba, bb) : max(ba, bb)) * kEbCols >= n) return;  // padding: no pair of columns to rotate
    for (int idx = threadIdx.x; idx < 2 * kEbCols * ldx; idx += kEbThreads) {
        const int j = idx / ldx, r = idx - j * ldx;
        const int c = (j < kEbCols ? ba * kEbCols + j : bb * kEbCols + j - kEbCols);
        eb_cols[idx] = X[(int64_t)c * ldx + r];
    }
    __syncthreads();
    const double tol2 = (double)n * 2.220446049250313e-16 * 2.220446049250313e-16;
    const int inner = full ? 2 * kEbCols - 1 : kEbCols;
    int rotated = 0;
    for (int s = 0; s < inner; ++s) {
        int p, r;  // this wave's pair of local columns
        if (full) {
            constexpr int np = 2 * kEbCols;
            p = w == 0 ? np - 1 : (s + w) % (np - 1);
            r = (s + np - 1 - w) % (np - 1);
        } else {
            p = w;
            r = kEbCols + ((w + s) & (kEbCols - 1));
        }
        const int cp = p < kEbCols ? ba * kEbCols + p : bb * kEbCols + p - kEbCols;
        const int cr = r < kEbCols ? ba * kEbCols + r : bb * kEbCols + r - kEbCols;
        if (cp < n && cr < n) {  // wave uniform
            double x[E], y[E];
            double vpp = 0.0, vqq = 0.0, vpq = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                x[e] = eb_cols[p * ldx + e * 64 + lane];
                y[e] = eb_cols[r * ldx + e * 64 + lane];
                vpp = __builtin_fma(x[e], x[e], vpp);
                vqq = __builtin_fma(y[e], y[e], vqq);
                vpq = __builtin_fma(x[e], y[e], vpq);
            }
            const double app = wave_allsum(vpp), aqq = wave_allsum(vqq), apq = wave_allsum(vpq);
            // tan 2 theta = 2 apq / (aqq - app), |theta| <= pi / 4 (the register kernel's rotation)
            const double alpha = aqq - app, beta = 2.0 * apq;
            const double r2 = __builtin_fma(alpha, alpha, beta * beta);
            if (apq * apq > tol2 * (app * aqq) && r2 > 0.0) {
                const double ir = rsqrt_nr(r2);
                const double c2 = __builtin_fma(0.5 * fabs(alpha), ir, 0.5);
                const double ic = rsqrt_nr(c2);
                const double c = c2 * ic;
                const double sn = (alpha >= 0.0 ? 0.5 : -0.5) * beta * ir * ic;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    eb_cols[p * ldx + e * 64 + lane] = __builtin_fma(c, x[e], -(sn * y[e]));
                    eb_cols[r * ldx + e * 64 + lane] = __builtin_fma(sn, x[e], c * y[e]);
                }
                rotated = 1;
            }
        }
        __syncthreads();
    }
    if (!__syncthreads_or(rotated)) return;  // nothing changed: nothing to write back
    for (int idx = threadIdx.x; idx < 2 * kEbCols * ldx; idx += kEbThreads) {
        const int j = idx / ldx, r = idx - j * ldx;
        const int c = (j < kEbCols ? ba * kEbCols + j : bb * kEbCols + j - kEbCols);
        X[(int64_t)c * ldx + r] = eb_cols[idx];
    }
    if (threadIdx.x == 0) atomicAdd(&rotations[q], 1);
}

// squared column lengths, their descending rank (ties in column order), the eigenvalues and the two words of info
__global__ __launch_bounds__(kEbThreads) void eigb_rank_kernel(EigbBatch b, int32_t ldx, double *e0, double *e1, double *e2, int32_t *i0,
                                                               int32_t *i1, int32_t *i2, int32_t *__restrict__ rank_of /* [3][512] */,
                                                               double *__restrict__ norms /* [3][512] */, int32_t sweeps,
                                                               const int32_t *__restrict__ failed) {
    __shared__ double nr[512];
    const int q = blockIdx.x;
    const int n = b.n[q];
    const double *X = b.X[q];
    double *evals = q == 0 ? e0 : (q == 1 ? e1 : e2);
    int32_t *info = q == 0 ? i0 : (q == 1 ? i1 : i2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < n; c += kEbThreads / 64) {
        double v = 0.0;
        for (int r = lane; r < n; r += 64) v = __builtin_fma(X[(int64_t)c * ldx + r], X[(int64_t)c * ldx + r], v);
        v = wave_allsum(v);
        if (lane == 0) nr[c] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kEbThreads) {
        const double li = nr[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = nr[j];
            rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
        rank_of[q * 512 + i] = rank;
        norms[q * 512 + i] = li;
        evals[rank] = li;
    }
    if (threadIdx.x == 0) {
        double mx = 0.0, mn = __builtin_huge_val();
        for (int i = 0; i < n; ++i) {
            mx = fmax(mx, nr[i]);
            mn = fmin(mn, nr[i]);
        }
        info[0] = sweeps;
        info[1] = (failed[q] || !(mn > (double)n * 2.220446049250313e-16 * mx)) ? 1 : 0;
    }
}

// Vs[row][rank of column i] = C V [row][i] / its length
__global__ __launch_bounds__(256) void eigb_vectors_kernel(EigbBatch b, int32_t ldx, double *v0, double *v1, double *v2,
                                                           const int32_t *__restrict__ rank_of, const double *__restrict__ norms) {
    const int q = blockIdx.y;
    const int n = b.n[q];
    double *Vs = q == 0 ? v0 : (q == 1 ? v1 : v2);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, row = idx - i * n;
    const double len = sqrt(norms[q * 512 + i]);
    Vs[(int64_t)row * n + rank_of[q * 512 + i]] = len > 0.0 ? b.X[q][(int64_t)i * ldx + row] / len : 0.0;
}

template <int E>
void launch_eigb_round(gingr_ctx *ctx, const EigbBatch &b, int count, int nblk, int rd, int32_t *rotations, const int32_t *failed) {
    const size_t lds = (size_t)2 * kEbCols * E * 64 * sizeof(double);
    set_dynamic_lds(eigb_round_kernel<E>, lds);
    hipLaunchKernelGGL((eigb_round_kernel<E>), dim3(nblk / 2, count), dim3(kEbThreads), lds, ctx->stream, b, nblk, rd, rd == 0 ? 1 : 0,
                       rotations, failed);
}

}  // namespace

int64_t sym_eig_blocks_work_doubles(int32_t n) {
    const int64_t nblk = (ceil_div(n, kEbCols) + 1) & ~(int64_t)1;
    return nblk * kEbCols * round_up(n, 64);
}

// Up to three decompositions side by side, every n in kSymEigColsMaxN + 1 .. 512.  work[q]: sym_eig_blocks_work_doubles(largest n)
// doubles; info[q]: two int32 on the device (sweeps of the call, singular flag of the problem), valid when the call returns.  A
// problem with a failed pivot is reported singular (its evals / Vs are not a decomposition) and is no concern of the other problems
// of the call, which are rotated and reported as they are in a call where nothing fails.  Synchronises the stream.
int sym_eig_blocks(gingr_ctx *ctx, int count, const double *const *G, const int32_t *ldg, const int32_t *n, double *const *work,
                   double *const *evals, double *const *Vs, int32_t *const *info) {
    int32_t nmax = 0;
    EigbBatch b;
    for (int q = 0; q < 3; ++q) {
        const int s = q < count ? q : 0;
        if (n[s] <= kSymEigColsMaxN || n[s] > 512) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sym_eig_blocks: n = %d outside %d..512", (int)n[s], kSymEigColsMaxN + 1);
        b.X[q] = work[s], b.n[q] = n[s];
        nmax = std::max(nmax, n[s]);
    }
    const int32_t ldx = (int32_t)round_up(nmax, 64);
    const int nblk = (int)((ceil_div(nmax, kEbCols) + 1) & ~(int64_t)1);
    const int cols = nblk * kEbCols;
    constexpr int kMaxSweeps = 60;
    DevBuf words, ranks, norms;  // [0..2] failed pivots, [3 + 3 sweep + q] rotations of a sweep
    HIP_TRY(ctx, words.alloc((size_t)(3 + 3 * kMaxSweeps) * sizeof(int32_t)));
    HIP_TRY(ctx, ranks.alloc((size_t)3 * 512 * sizeof(int32_t)));
    HIP_TRY(ctx, norms.alloc((size_t)3 * 512 * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(words.p, 0, words.bytes, ctx->stream));
    int32_t *failed = words.as<int32_t>();
    hipLaunchKernelGGL(eigb_load_kernel, dim3((unsigned)ceil_div((int64_t)cols * ldx, 256), count), dim3(256), 0, ctx->stream, b, G[0],
                       G[count > 1 ? 1 : 0], G[count > 2 ? 2 : 0], ldg[0], ldg[count > 1 ? 1 : 0], ldg[count > 2 ? 2 : 0], ldx, cols);
    for (int k0 = 0; k0 < nmax; k0 += kEbCols) {
        hipLaunchKernelGGL(eigb_chol_panel_kernel, dim3(count), dim3(kEbThreads), 0, ctx->stream, b, ldx, k0, failed);
        if (k0 + kEbCols < nmax)
            hipLaunchKernelGGL(eigb_chol_update_kernel, dim3((unsigned)ceil_div(nmax, 256), nmax - k0 - kEbCols, count), dim3(256), 0,
                               ctx->stream, b, ldx, k0);
    }
    HIP_TRY(ctx, hipGetLastError());
    int32_t hfail[3] = {0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(hfail, failed, sizeof(hfail), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // A failed pivot concerns its own problem only: the workgroups of that problem leave eigb_round_kernel at once (`failed`), the
    // sweeps run as long as one problem of the call factored, and the problems that factored keep their arithmetic -- and their
    // bits -- whatever their neighbours did.  (Of the two remedies for the sweeps once skipped for the whole call, this is the first:
    // the failed words go to the round kernel; info[1] is not raised for the problems that factored.)  The failed problem comes
    // back with info[1] = 1 and the caller's other kernel decomposes its G itself.
    bool any_factored = false;
    for (int q = 0; q < count; ++q) any_factored = any_factored || !hfail[q];
    int sweep = 0;
    if (any_factored) {
        for (; sweep < kMaxSweeps; ++sweep) {
            int32_t *rot = words.as<int32_t>() + 3 + 3 * sweep;
            for (int rd = 0; rd < nblk - 1; ++rd) switch (ldx / 64) {
                    case 4: launch_eigb_round<4>(ctx, b, count, nblk, rd, rot, failed); break;
                    case 5: launch_eigb_round<5>(ctx, b, count, nblk, rd, rot, failed); break;
                    case 6: launch_eigb_round<6>(ctx, b, count, nblk, rd, rot, failed); break;
                    case 7: launch_eigb_round<7>(ctx, b, count, nblk, rd, rot, failed); break;
                    default: launch_eigb_round<8>(ctx, b, count, nblk, rd, rot, failed); break;
                }
            HIP_TRY(ctx, hipGetLastError());
            int32_t h[3] = {0, 0, 0};
            HIP_TRY(ctx, hipMemcpyAsync(h, rot, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (!(h[0] | h[1] | h[2])) {
                ++sweep;
                break;
            }
        }
    }
    hipLaunchKernelGGL(eigb_rank_kernel, dim3(count), dim3(kEbThreads), 0, ctx->stream, b, ldx, evals[0], evals[count > 1 ? 1 : 0],
                       evals[count > 2 ? 2 : 0], info[0], info[count > 1 ? 1 : 0], info[count > 2 ? 2 : 0], ranks.as<int32_t>(),
                       norms.as<double>(), (int32_t)sweep, failed);
    hipLaunchKernelGGL(eigb_vectors_kernel, dim3((unsigned)ceil_div((int64_t)nmax * nmax, 256), count), dim3(256), 0, ctx->stream, b, ldx,
                       Vs[0], Vs[count > 1 ? 1 : 0], Vs[count > 2 ? 2 : 0], ranks.as<int32_t>(), norms.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the work buffers go out of scope
    return GINGR_OK;
}

int64_t sym_eig_cols_work_doubles(int32_t n) {
    return (int64_t)kEigSlots * n + kEigSlots;
}

// up to three decompositions side by side (one workgroup each); every n in 1 .. kSymEigColsMaxN.  work[q]: sym_eig_cols_work_doubles(n[q])
// doubles; info[q]: two int32 (sweeps, singular flag).
void launch_sym_eig_cols(gingr_ctx *ctx, int count, const double *const *G, const int32_t *ldg, const int32_t *n, double *const *work,
                         double *const *evals, double *const *Vs, int32_t *const *info) {
    EigBatch b;
    int32_t nmax = 0;
    for (int q = 0; q < count; ++q) {
        b.p[q] = EigProblem{G[q], ldg[q], n[q], work[q], work[q] + (int64_t)kEigSlots * n[q], evals[q], Vs[q], info[q]};
        nmax = n[q] > nmax ? n[q] : nmax;
    }
    for (int q = count; q < 3; ++q) b.p[q] = b.p[0];
    if (nmax <= 64)
        hipLaunchKernelGGL((sym_eig_cols_kernel<1, 2, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, b);
    else if (nmax <= 128)
        hipLaunchKernelGGL((sym_eig_cols_kernel<2, 4, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, b);
    else
        hipLaunchKernelGGL((sym_eig_cols_kernel<3, 6, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, b);
}

// `count` decompositions of one size n <= kSymEigColsMaxN in one launch, one workgroup each: problem q reads G + q g_stride (row stride
// ldg) and writes evals + q n, Vs + q n n, info + 2 q; work: count * sym_eig_cols_work_doubles(n) doubles.  The kernel of
// launch_sym_eig_cols, the same arithmetic in the same order.
void launch_sym_eig_cols_strided(gingr_ctx *ctx, int count, const double *G, int64_t g_stride, int32_t ldg, int32_t n, double *work, double *evals,
                                 double *Vs, int32_t *info) {
    const EigStrided s{G, g_stride, ldg, n, work, sym_eig_cols_work_doubles(n), evals, (int64_t)n, Vs, (int64_t)n * n, info};
    if (n <= 64)
        hipLaunchKernelGGL((sym_eig_cols_strided_kernel<1, 2, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, s);
    else if (n <= 128)
        hipLaunchKernelGGL((sym_eig_cols_strided_kernel<2, 4, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, s);
    else
        hipLaunchKernelGGL((sym_eig_cols_strided_kernel<3, 6, 16>), dim3(count), dim3(16 * 64), 0, ctx->stream, s);
}
