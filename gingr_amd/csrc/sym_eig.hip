// Eigen-decomposition of a small symmetric positive semi-definite matrix (n <= kJacMaxN): the front door sym_eig, which deals the
// problems of a call to the register kernel and the block kernel of eig.hip, and the two-sided cyclic Jacobi behind both -- the path of a
// numerically singular matrix, of a decomposition eig.hip reports as not converged, and of everything above kSymEigColsMaxN columns
// when the block kernel is not asked for.  Callers: the GPMM construction (gpmm.hip), model finalisation (model.hip), the PCA, augmented
// and posterior models (pca_model.hip, augment_model.hip, posterior_model.hip).
#include "gp.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

namespace {

// Cyclic Jacobi eigen-decomposition of the leading n x n block of G (row stride ldg), one workgroup, matrices in global
// memory (L2 resident).  Round-robin ordering: n' - 1 rounds of n'/2 disjoint rotations; a round is applied as
// A <- A J (columns), then A <- J^T A (rows), V <- V J.  Output: evals descending, Vs[:, rank] the matching eigenvectors.
constexpr int kJacThreads = 1024;

__global__ __launch_bounds__(kJacThreads) void jacobi_eig_kernel(const double *__restrict__ G, int32_t ldg, int32_t n,
                                                                 double *__restrict__ A, double *__restrict__ V,
                                                                 double *__restrict__ evals, double *__restrict__ Vs,
                                                                 int32_t *__restrict__ sweeps_out) {
    __shared__ double cs[kJacMaxN / 2][2];
    __shared__ int32_t pq[kJacMaxN / 2][2];
    __shared__ int32_t nrot;
    const int t = threadIdx.x;
    for (int idx = t; idx < n * n; idx += kJacThreads) {
        const int i = idx / n, j = idx - i * n;
        A[idx] = G[(int64_t)i * ldg + j];
        V[idx] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    const int np = (n + 1) & ~1;  // even number of players; index np-1 >= n is a bye
    const int half = np / 2;
    int sweep = 0;
    for (; sweep < 60 && n > 1; ++sweep) {
        if (t == 0) nrot = 0;
        __syncthreads();
        for (int rd = 0; rd < np - 1; ++rd) {
            if (t < half) {
                int a = t == 0 ? np - 1 : (rd + t) % (np - 1);
                int b = (rd + np - 1 - t) % (np - 1);
                if (a > b) {
                    const int tmp = a;
                    a = b;
                    b = tmp;
                }
                double c = 1.0, s = 0.0;
                if (b < n) {
                    const double app = A[a * n + a], aqq = A[b * n + b], apq = A[a * n + b];
                    if (fabs(apq) > 1.1102230246251565e-16 * sqrt(fabs(app) * fabs(aqq)) && apq != 0.0) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        s = tt * c;
                        atomicAdd(&nrot, 1);
                    }
                } else {
                    b = -1;
                }
                cs[t][0] = c;
                cs[t][1] = s;
                pq[t][0] = a;
                pq[t][1] = b;
            }
            __syncthreads();
            // columns of A and V
            for (int idx = t; idx < half * n; idx += kJacThreads) {
                const int i = idx / half, m = idx - i * half;  // neighbouring lanes: one row, different pairs
                const int p = pq[m][0], q = pq[m][1];
                const double c = cs[m][0], s = cs[m][1];
                if (q < 0 || s == 0.0) continue;
                const double aip = A[i * n + p], aiq = A[i * n + q];
                A[i * n + p] = c * aip - s * aiq;
                A[i * n + q] = s * aip + c * aiq;
                const double vip = V[i * n + p], viq = V[i * n + q];
                V[i * n + p] = c * vip - s * viq;
                V[i * n + q] = s * vip + c * viq;
            }
            __syncthreads();
            // rows of A
            for (int idx = t; idx < half * n; idx += kJacThreads) {
                const int m = idx / n, j = idx - m * n;
                const int p = pq[m][0], q = pq[m][1];
                const double c = cs[m][0], s = cs[m][1];
                if (q < 0 || s == 0.0) continue;
                const double apj = A[p * n + j], aqj = A[q * n + j];
                A[p * n + j] = c * apj - s * aqj;
                A[q * n + j] = s * apj + c * aqj;
            }
            __syncthreads();
        }
        const int done = nrot == 0;
        __syncthreads();
        if (done) break;
    }
    if (t == 0 && sweeps_out) *sweeps_out = sweep;
    // sort descending (rank sort; ties keep index order)
    for (int i = t; i < n; i += kJacThreads) {
        const double li = A[i * n + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = A[j * n + j];
            rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
        evals[rank] = li;
        for (int r = 0; r < n; ++r) Vs[r * n + rank] = V[r * n + i];
    }
}

// The same decomposition on several workgroups (n > 128: beyond the register kernel of eig.hip the one-workgroup form above moves
// 3 n^2 entries per round through ONE compute unit's path to L2 -- 150 ms at n = 301).  Every workgroup works out all rotations of a
// round itself (the same numbers from the same entries), then forms its share of A' = J^T (A J) entry by entry from the round's
// source buffer into the other one (an entry needs the four entries at (i | partner of i, j | partner of j); first the column
// combination, then the row combination: the one-workgroup kernel's arithmetic in its order, so the same bits) and rotates its share
// of V in place (row-local).  One barrier over the grid per round instead of three workgroup barriers; the grid is far smaller than
// the device (64 workgroups of 256 threads) so that all of it is resident.  A barrier that is not met within two seconds (a device
// shared with something that never yields) raises the flag in sync[1]: the call reports a failure instead of hanging.
constexpr int kJacGridThreads = 256;
constexpr int kJacGridWgs = 64;

// One wave's thread does the device-scope part for its workgroup (as a cooperative-groups grid barrier does): the workgroup barrier
// in front has every wave's stores completed, the release fence then writes the compute unit's and the XCD's dirty lines back ONCE,
// and the acquire fence behind the wait drops the stale lines for the whole compute unit -- with the two fences in every thread the
// cache maintenance ran eight times per workgroup and round (22 us a round at n = 301 against 12).
__device__ __forceinline__ bool jac_grid_barrier(unsigned *sync, unsigned target, int *s_ok) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(&sync[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long t0 = wall_clock64();  // (100 MHz)
        int good = 1;
        unsigned spins = 0;
        while (__hip_atomic_load(&sync[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 255u) == 0u) {
                if (__hip_atomic_load(&sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    good = 0;
                    break;
                }
                if (wall_clock64() - t0 > 200000000LL) {
                    __hip_atomic_store(&sync[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    good = 0;
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        *s_ok = good;
    }
    __syncthreads();
    return *s_ok != 0;
}

__global__ __launch_bounds__(kJacGridThreads) void jacobi_eig_grid_kernel(const double *__restrict__ G, int32_t ldg, int32_t n, double *A0,
                                                                          double *A1, double *V, double *__restrict__ evals,
                                                                          double *__restrict__ Vs, int32_t *__restrict__ sweeps_out,
                                                                          unsigned *sync) {
    __shared__ double cs[kJacMaxN / 2][2];
    __shared__ int32_t pq[kJacMaxN / 2][2];
    __shared__ int16_t pair_of[kJacMaxN];  // index -> its pair of the round, -1: none (the bye, or a pair that does not rotate)
    __shared__ int32_t nrot;
    __shared__ int s_ok;
    const int t = threadIdx.x;
    const unsigned nwg = gridDim.x;
    const unsigned gtid = blockIdx.x * kJacGridThreads + t, gthreads = nwg * kJacGridThreads;  // (n <= 512: 32-bit index arithmetic)
    const unsigned nn = (unsigned)n * (unsigned)n, un = (unsigned)n;
    unsigned epoch = 0;
    for (unsigned idx = gtid; idx < nn; idx += gthreads) {
        const int i = (int)(idx / un), j = (int)(idx - (unsigned)i * un);
        A0[idx] = G[(int64_t)i * ldg + j];
        V[idx] = i == j ? 1.0 : 0.0;
    }
    if (!jac_grid_barrier(sync, ++epoch * nwg, &s_ok)) return;
    double *A = A0, *B = A1;  // source and destination of the round
    const int np = (n + 1) & ~1;
    const int half = np / 2;
    int sweep = 0;
    for (; sweep < 60 && n > 1; ++sweep) {
        if (t == 0) nrot = 0;
        __syncthreads();
        for (int rd = 0; rd < np - 1; ++rd) {
            for (int i = t; i < n; i += kJacGridThreads) pair_of[i] = -1;
            __syncthreads();
            if (t < half) {  // (the one-workgroup kernel's pairing and rotation, statement by statement)
                int a = t == 0 ? np - 1 : (rd + t) % (np - 1);
                int b = (rd + np - 1 - t) % (np - 1);
                if (a > b) {
                    const int tmp = a;
                    a = b;
                    b = tmp;
                }
                double c = 1.0, s = 0.0;
                if (b < n) {
                    const double app = A[a * n + a], aqq = A[b * n + b], apq = A[a * n + b];
                    if (fabs(apq) > 1.1102230246251565e-16 * sqrt(fabs(app) * fabs(aqq)) && apq != 0.0) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        s = tt * c;
                        atomicAdd(&nrot, 1);
                    }
                } else {
                    b = -1;
                }
                cs[t][0] = c;
                cs[t][1] = s;
                pq[t][0] = a;
                pq[t][1] = b;
                if (b >= 0 && s != 0.0) {
                    pair_of[a] = (int16_t)t;
                    pair_of[b] = (int16_t)t;
                }
            }
            __syncthreads();
            // A' = J^T (A J), entry by entry
            for (unsigned idx = gtid; idx < nn; idx += gthreads) {
                const int i = (int)(idx / un), j = (int)(idx - (unsigned)i * un);
                const int mi = pair_of[i], mj = pair_of[j];
                // the column combination at row r: (A J)[r][j]
                auto col = [&](int r) -> double {
                    if (mj < 0) return A[r * n + j];
                    const int p = pq[mj][0], q = pq[mj][1];
                    const double c = cs[mj][0], sn = cs[mj][1];
                    const double arp = A[r * n + p], arq = A[r * n + q];
                    return j == p ? c * arp - sn * arq : sn * arp + c * arq;
                };
                double out;
                if (mi < 0) {
                    out = col(i);
                } else {
                    const int p = pq[mi][0], q = pq[mi][1];
                    const double c = cs[mi][0], sn = cs[mi][1];
                    const double apj = col(p), aqj = col(q);
                    out = i == p ? c * apj - sn * aqj : sn * apj + c * aqj;
                }
                B[idx] = out;
            }
            // V <- V J, in place (an item touches the two entries of its row and pair only)
            for (unsigned idx = gtid; idx < (unsigned)half * un; idx += gthreads) {
                const int i = (int)(idx / (unsigned)half), m = (int)(idx - (unsigned)i * (unsigned)half);
                const int p = pq[m][0], q = pq[m][1];
                const double c = cs[m][0], sn = cs[m][1];
                if (q < 0 || sn == 0.0) continue;
                const double vip = V[i * n + p], viq = V[i * n + q];
                V[i * n + p] = c * vip - sn * viq;
                V[i * n + q] = sn * vip + c * viq;
            }
            if (!jac_grid_barrier(sync, ++epoch * nwg, &s_ok)) return;
            double *tmp = A;
            A = B;
            B = tmp;
        }
        const int done = nrot == 0;
        __syncthreads();
        if (done) break;
    }
    if (gtid == 0 && sweeps_out) *sweeps_out = sweep;
    // sort descending (rank sort; ties keep index order)
    for (int i = (int)gtid; i < n; i += (int)gthreads) {
        const double li = A[i * n + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = A[j * n + j];
            rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
        evals[rank] = li;
        for (int r = 0; r < n; ++r) Vs[r * n + rank] = V[r * n + i];
    }
}

// One decomposition with the two-sided kernel (any n <= kJacMaxN; the fallback of sym_eig, and its path above kSymEigColsMaxN)
int jacobi_two_sided(gingr_ctx *ctx, const double *G, int32_t ldg, int32_t n, double *evals, double *Vs, int32_t *sweeps) {
    const bool grid = n > 128;  // the same arithmetic on 64 workgroups (a second buffer for A, a barrier word and a failure flag)
    DevBuf wA, wV, wB, sync;
    HIP_TRY(ctx, wA.alloc((size_t)n * n * sizeof(double)));
    HIP_TRY(ctx, wV.alloc((size_t)n * n * sizeof(double)));
    unsigned h[2] = {0, 0};
    if (grid) {
        HIP_TRY(ctx, wB.alloc((size_t)n * n * sizeof(double)));
        HIP_TRY(ctx, sync.alloc(2 * sizeof(unsigned)));
        HIP_TRY(ctx, hipMemsetAsync(sync.p, 0, 2 * sizeof(unsigned), ctx->stream));
        hipLaunchKernelGGL(jacobi_eig_grid_kernel, dim3(kJacGridWgs), dim3(kJacGridThreads), 0, ctx->stream, G, ldg, n, wA.as<double>(),
                           wB.as<double>(), wV.as<double>(), evals, Vs, sweeps, sync.as<unsigned>());
    } else {
        hipLaunchKernelGGL(jacobi_eig_kernel, dim3(1), dim3(kJacThreads), 0, ctx->stream, G, ldg, n, wA.as<double>(), wV.as<double>(), evals,
                           Vs, sweeps);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (grid) HIP_TRY(ctx, hipMemcpyAsync(h, sync.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the work buffers go out of scope
    if (h[1])
        return gingr_set_error(ctx, GINGR_ERR_STATE, "sym_eig: the workgroups of the decomposition did not meet within two seconds (n = %d)", (int)n);
    return GINGR_OK;
}

// The problems of a call that one of the kernels of eig.hip takes, in that kernel's argument form; of[f] = the caller's index of problem f
struct EigProblems {
    DevBuf buf[3];
    const double *G[3];
    int32_t ldg[3], n[3], *info[3];
    double *work[3], *evals[3], *Vs[3];
    int of[3], count = 0;
};

// p = the problems q with pick(q), each with a work buffer of work_doubles(q) doubles and its two words of `info`
template <typename Pick, typename WorkDoubles>
int gather_problems(gingr_ctx *ctx, int count, const double *const *G, const int32_t *ldg, const int32_t *n, double *const *evals,
                    double *const *Vs, int32_t *info, Pick pick, WorkDoubles work_doubles, EigProblems &p) {
    for (int q = 0; q < count; ++q) {
        if (!pick(q)) continue;
        const int f = p.count++;
        HIP_TRY(ctx, p.buf[f].alloc((size_t)work_doubles(q) * sizeof(double)));
        p.G[f] = G[q], p.ldg[f] = ldg[q], p.n[f] = n[q], p.work[f] = p.buf[f].as<double>(), p.evals[f] = evals[q], p.Vs[f] = Vs[q];
        p.info[f] = info + 2 * q;
        p.of[f] = q;
    }
    return GINGR_OK;
}

}  // namespace

// Eigen-decompositions of up to three symmetric positive semi-definite matrices (leading n[q] x n[q] block of G[q], row stride ldg[q]):
// evals[q] descending, Vs[q][:, k] the matching eigenvectors.  Up to kSymEigColsMaxN the register kernel of eig.hip, all problems in
// one launch; a problem it reports as numerically singular or not converged -- and anything larger -- goes through the two-sided
// kernel.  `blocks`: problems above kSymEigColsMaxN go through the block kernel of eig.hip first (sym_eig_blocks; the scalar route of
// gingr_gpmm_build_diagonal_ex, whose blocks no earlier entry could reach) -- without it they take the two-sided kernel directly, as
// every model with such a problem always has.  GINGR_EIG_TWO_SIDED=1 in the environment switches `blocks` off (same-box timing of the
// two kernels).  Synchronises the stream.  GINGR_ERR_NONFINITE when a decomposition does not converge.
int sym_eig(gingr_ctx *ctx, int count, const double *const *G, const int32_t *ldg, const int32_t *n, double *const *evals,
            double *const *Vs, bool blocks) {
    if (count < 1 || count > 3) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sym_eig: 1..3 problems");
    DevBuf info;
    HIP_TRY(ctx, info.alloc(3 * 2 * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemsetAsync(info.p, 0, 3 * 2 * sizeof(int32_t), ctx->stream));
    bool redo[3] = {false, false, false};
    int32_t nmax = 0;  // the largest problem above the register kernel's size
    for (int q = 0; q < count; ++q) {
        if (n[q] < 1 || n[q] > kJacMaxN) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sym_eig: n = %d outside 1..%d", (int)n[q], kJacMaxN);
        redo[q] = n[q] > kSymEigColsMaxN;
        if (redo[q]) nmax = std::max(nmax, n[q]);
    }
    auto failed = [](const int32_t *h, int q) { return h[2 * q] >= 60 || h[2 * q + 1] != 0; };  // (sweeps, numerically singular)
    EigProblems fast;
    GINGR_TRY(gather_problems(ctx, count, G, ldg, n, evals, Vs, info.as<int32_t>(), [&](int q) { return n[q] <= kSymEigColsMaxN; },
                              [&](int q) { return sym_eig_cols_work_doubles(n[q]); }, fast));
    if (fast.count) {
        launch_sym_eig_cols(ctx, fast.count, fast.G, fast.ldg, fast.n, fast.work, fast.evals, fast.Vs, fast.info);
        HIP_TRY(ctx, hipGetLastError());
        int32_t h[6];
        HIP_TRY(ctx, hipMemcpyAsync(h, info.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int f = 0; f < fast.count; ++f) redo[fast.of[f]] = failed(h, fast.of[f]);
    }
    static const bool two_sided_only = getenv("GINGR_EIG_TWO_SIDED") != nullptr;
    // GINGR_EIG_TIMING=1 (tools/bench_gpmm_to_tolerance.py): wall time of the problems above kSymEigColsMaxN, one line on stderr
    static const bool timing_on = getenv("GINGR_EIG_TIMING") != nullptr;
    const bool timing = timing_on && nmax > 0;
    std::chrono::steady_clock::time_point t0;
    if (timing) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        t0 = std::chrono::steady_clock::now();
    }
    EigProblems big;  // the problems above the register kernel's size, side by side
    if (blocks && !two_sided_only)
        GINGR_TRY(gather_problems(ctx, count, G, ldg, n, evals, Vs, info.as<int32_t>(), [&](int q) { return n[q] > kSymEigColsMaxN; },
                                  [&](int) { return sym_eig_blocks_work_doubles(nmax); }, big));
    if (big.count) {
        GINGR_TRY(sym_eig_blocks(ctx, big.count, big.G, big.ldg, big.n, big.work, big.evals, big.Vs, big.info));
        int32_t h[6];
        HIP_TRY(ctx, hipMemcpy(h, info.p, sizeof(h), hipMemcpyDeviceToHost));
        for (int f = 0; f < big.count; ++f) redo[big.of[f]] = failed(h, big.of[f]);
    }
    for (int q = 0; q < count; ++q) {
        if (!redo[q]) continue;
        GINGR_TRY(jacobi_two_sided(ctx, G[q], ldg[q], n[q], evals[q], Vs[q], info.as<int32_t>() + 2 * q));
        int32_t sw = 0;
        HIP_TRY(ctx, hipMemcpy(&sw, info.as<int32_t>() + 2 * q, sizeof(sw), hipMemcpyDeviceToHost));
        if (sw >= 60) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "sym_eig: Jacobi did not converge (n = %d)", (int)n[q]);
    }
    if (timing) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        int fell_back = 0;
        for (int q = 0; q < count; ++q) fell_back += redo[q] ? 1 : 0;
        fprintf(stderr, "sym_eig_timing n=%d,%d,%d kernel=%s two_sided_runs=%d ms=%.3f\n", (int)n[0], count > 1 ? (int)n[1] : 0,
                count > 2 ? (int)n[2] : 0, blocks && !two_sided_only ? "blocks" : "two_sided", fell_back, ms);
    }
    return GINGR_OK;
}

int launch_jacobi_eig(gingr_ctx *ctx, const double *G, int32_t ldg, int32_t n, double *evals, double *Vs, bool blocks) {
    return sym_eig(ctx, 1, &G, &ldg, &n, &evals, &Vs, blocks);
}

// `count` decompositions of one size n (1 .. kJacMaxN) side by side: problem q is the n x n matrix at G + q n n (row stride n), its
// results go to evals + q n and Vs + q n n.  Up to kSymEigColsMaxN columns the register kernel of eig.hip, one workgroup per problem and
// all of them in one launch (timing hook 22: that launch alone); a problem it reports as numerically singular or not converged takes
// the two-sided kernel, as in sym_eig.  Larger problems go through sym_eig(..., blocks = true), three at a time.  Synchronises the
// stream.
int sym_eig_strided(gingr_ctx *ctx, int count, const double *G, int32_t n, double *evals, double *Vs) {
    if (count < 1) return GINGR_OK;
    if (n < 1 || n > kJacMaxN) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sym_eig: n = %d outside 1..%d", (int)n, kJacMaxN);
    const int64_t nn = (int64_t)n * n;
    if (n > kSymEigColsMaxN) {
        for (int q0 = 0; q0 < count; q0 += 3) {
            const int c = std::min(3, count - q0);
            const double *g[3];
            double *e[3], *v[3];
            int32_t ld[3], nq[3];
            for (int q = 0; q < c; ++q) g[q] = G + (q0 + q) * nn, e[q] = evals + (int64_t)(q0 + q) * n, v[q] = Vs + (q0 + q) * nn, ld[q] = nq[q] = n;
            GINGR_TRY(sym_eig(ctx, c, g, ld, nq, e, v, true));
        }
        return GINGR_OK;
    }
    DevBuf info, work;
    HIP_TRY(ctx, info.alloc((size_t)count * 2 * sizeof(int32_t)));
    HIP_TRY(ctx, work.alloc((size_t)count * sym_eig_cols_work_doubles(n) * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(info.p, 0, (size_t)count * 2 * sizeof(int32_t), ctx->stream));
    {
        TimerScope ts(ctx, 22);
        launch_sym_eig_cols_strided(ctx, count, G, nn, n, n, work.as<double>(), evals, Vs, info.as<int32_t>());
    }
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> h((size_t)count * 2);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), info.p, (size_t)count * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < count; ++q) {
        if (h[2 * (size_t)q] < 60 && h[2 * (size_t)q + 1] == 0) continue;
        GINGR_TRY(jacobi_two_sided(ctx, G + q * nn, n, n, evals + (int64_t)q * n, Vs + q * nn, info.as<int32_t>() + 2 * q));
        int32_t sw = 0;
        HIP_TRY(ctx, hipMemcpy(&sw, info.as<int32_t>() + 2 * q, sizeof(sw), hipMemcpyDeviceToHost));
        if (sw >= 60) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "sym_eig: Jacobi did not converge (n = %d)", (int)n);
    }
    return GINGR_OK;
}
