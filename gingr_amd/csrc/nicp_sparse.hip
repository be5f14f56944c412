// Optimal-step non-rigid ICP past dense sizes: the least-squares step of NonRigidOptimalStepICP.scala as a matrix-free block-Jacobi
// preconditioned conjugate gradient on the device.  The system is the one gingr_nicp_solve (nicp_dense.hip) forms densely,
//   N-ICP-T   (alpha^2 Lg + W^2 + E_L) X = W^2 (U - V) + E_L^T beta (UL - VL)                               unknown n x 3
//   N-ICP-A   (alpha^2 Lg (x) G^2 + D^T W^2 D + beta^2 DL^T DL) X = D^T W^2 U + beta^2 DL^T UL             unknown 4n x 3
// with both quirks of the reference kept (N-ICP-T's landmark ones sit in the first L columns, unscaled by beta; N-ICP-A zeroes the
// weights of the landmark vertices), and it is never stored: the row block of vertex i is
//   s_i q_i q_i^T + alpha^2 deg_i G^2   on the diagonal        (q_i = [v_i, 1], G^2 = diag(1, 1, 1, gamma^2);  N-ICP-T: q = [1], G^2 = [1])
//   -alpha^2 G^2                        at every neighbour of the template's edge graph (CSR, nicp_graph.h)
// so one code path, templated on the K = 1 or 4 unknowns per vertex and column, serves both kinds.
//
// The three right-hand sides (x, y, z) are three independent CG recurrences sharing every pass over the graph.  One iteration is three
// launches on the context's stream,
//   apply      Ap = A p, block partials of p.Ap
//   update     alpha = r.z / p.Ap;  x += alpha p;  r -= alpha Ap;  z = B^-1 r;  block partials of r.z and r.r
//   direction  beta = r.z' / r.z;  p = z + beta p;  the stop test;  the scalars of the next iteration
// and every workgroup adds the block partials up itself, in one fixed order (thread-strided, then block_sum.h): no floating-point
// atomics, the same bits on every run.  The CG scalars, the per-column stop flags and `done` live in a control block on the device;
// what a launch reads of them was written by an EARLIER launch (the scalars alternate between two slots by the iteration's parity),
// with one exception: `done` and `error` may be set by workgroup 0 of the launch that reads them.  A workgroup that sees the early
// store returns at once, one that does not computes something nobody reads (p behind the stop, nothing behind a breakdown); the
// word is read by one thread and handed to the workgroup through LDS, so a workgroup never splits at a barrier.  The host enqueues
// kChunk iterations at a time and reads the control block between chunks through the pinned-word read-back of fitter.hip.
//
// The stop rule |r| <= rel_tol |b| is tested on the recurrence residual.  Behind the stop one more operator pass computes the true
// residual b - A x, which is the figure reported; it is the same pass that starts a recurrence (r, z = B^-1 r, p = z), so where a
// column's true residual misses the rule by the recurrence's drift, CG simply goes on from it: `converged` certifies the true residual.
#include "fitter.h"
#include "block_sum.h"
#include "nicp_graph.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;                 // iterations enqueued per look at `done`
constexpr double kDefaultRelTol = 1e-12;
constexpr int32_t kDefaultMaxIterations = 20000;
constexpr int kSlots = 12, kSlotBB = 0, kSlotRZ = 3, kSlotRR = 6, kSlotPAP = 9;

// the control block, all doubles (it travels through pull_small)
enum : int {
    CTL_DONE = 0,
    CTL_ITERATIONS = 1,
    CTL_CONVERGED = 2,
    CTL_ERROR = 3,
    CTL_RR = 4,      // [3] recurrence |r|^2 of the last iteration
    CTL_BB = 7,      // [3] |b|^2
    CTL_TRUE_RR = 10,  // [3] |b - A x|^2 of the last starting / closing pass
    CTL_RZ = 13,     // [2][3] r.z, slot = parity of the iteration that reads it
    CTL_FROZEN = 19,  // [2][3] column has met the stop rule (it is left alone from then on), same slots
    CTL_DOUBLES = 25
};

struct SparseArgs {
    int64_t n;
    const int32_t *row_ptr, *col;
    const double *v;    // template, SoA [3][n]
    const double *s;    // [n] scale of q q^T: T: w^2 + (1 for i < L);  A: w^2 + beta^2 (landmarks at the vertex)
    const double *t;    // SoA [3][n]: b_(c,a) = q_a t_c.  T: w^2 (u - v) + beta (UL_i - V[id_i]) for i < L;  A: w^2 u + beta^2 sum UL
    double alpha2, gamma2, tol2;
    double *x, *r, *z, *p, *ap;  // [3 K][n]: plane (c K + a)
    double *minv;                // [K (K + 1) / 2][n]: the inverse of the diagonal block, lower triangle row by row
    double *part;                // [blocks][kSlots] block partials: |b|^2 (set-up) | r.z | r.r | p.Ap, three columns each
    double *ctl;
    int32_t blocks;
};

template <int K>
__device__ __forceinline__ void load_q(const SparseArgs &a, int64_t i, double q[K]) {
    if (K == 4) {
        q[0] = a.v[i];
        q[1] = a.v[a.n + i];
        q[2] = a.v[2 * a.n + i];
    }
    q[K - 1] = 1.0;
}

template <int K>
__device__ __forceinline__ double g2_of(const SparseArgs &a, int c) {
    return (K == 4 && c == 3) ? a.gamma2 : 1.0;
}

// out = (A vec)_i, own = vec_i
template <int K>
__device__ __forceinline__ void apply_row(const SparseArgs &a, int64_t i, const double *__restrict__ vec, const double q[K], double own[3 * K],
                                          double out[3 * K]) {
    const int32_t k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
    double sum[3 * K];
#pragma unroll
    for (int m = 0; m < 3 * K; ++m) {
        own[m] = vec[(int64_t)m * a.n + i];
        sum[m] = 0.0;
    }
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t j = a.col[k];
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) sum[m] += vec[(int64_t)m * a.n + j];
    }
    const double deg = (double)(k1 - k0), s = a.s[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double d = 0.0;
#pragma unroll
        for (int e = 0; e < K; ++e) d += q[e] * own[c * K + e];
        d *= s;
#pragma unroll
        for (int e = 0; e < K; ++e) out[c * K + e] = d * q[e] + a.alpha2 * g2_of<K>(a, e) * (deg * own[c * K + e] - sum[c * K + e]);
    }
}

// z = B^-1 r for the three columns
template <int K>
__device__ __forceinline__ void precondition(const SparseArgs &a, int64_t i, const double r[3 * K], double z[3 * K]) {
    double m[K * (K + 1) / 2];
#pragma unroll
    for (int e = 0; e < K * (K + 1) / 2; ++e) m[e] = a.minv[(int64_t)e * a.n + i];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < K; ++e) {
            double acc = 0.0;
#pragma unroll
            for (int f = 0; f < K; ++f) acc += m[e >= f ? e * (e + 1) / 2 + f : f * (f + 1) / 2 + e] * r[c * K + f];
            z[c * K + e] = acc;
        }
}

// one value per workgroup into part[block][stride] at `slot`
__device__ __forceinline__ void put_partial(const SparseArgs &a, int slot, double value, double *sh) {
    __syncthreads();  // sh is reused
    const double total = block_sum<kThreads>(value, sh);
    if (threadIdx.x == 0) a.part[(int64_t)blockIdx.x * kSlots + slot] = total;
}

// the sum of one slot over all workgroups, the same bits in every thread of every workgroup
__device__ __forceinline__ double sum_partials(const SparseArgs &a, int slot, double *sh) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < a.blocks; b += kThreads) acc += a.part[(int64_t)b * kSlots + slot];
    __syncthreads();  // sh is reused
    return block_sum<kThreads>(acc, sh);
}

// ctl[word], read once and shared: the same answer in every thread of the workgroup whatever another workgroup stores meanwhile
__device__ __forceinline__ bool stopped(const SparseArgs &a, double *sh) {
    __syncthreads();
    if (threadIdx.x == 0) sh[0] = *reinterpret_cast<const volatile double *>(a.ctl + CTL_DONE);
    __syncthreads();
    const bool yes = sh[0] != 0.0;
    __syncthreads();
    return yes;
}

// the diagonal blocks and their inverses (Cholesky per vertex), the starting point, |b|^2
template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_setup_kernel(SparseArgs a) {
    __shared__ double sh[kThreads];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double bb[3] = {0.0, 0.0, 0.0};
    if (i < a.n) {
        double q[K];
        load_q<K>(a, i, q);
        const double s = a.s[i], lap = a.alpha2 * (double)(a.row_ptr[i + 1] - a.row_ptr[i]);
        // B = s q q^T + lap G^2 = L L^T, lower triangle row by row
        double L[K * (K + 1) / 2];
        bool ok = true;
#pragma unroll
        for (int e = 0; e < K; ++e)
#pragma unroll
            for (int f = 0; f <= e; ++f) {
                double val = s * q[e] * q[f] + (e == f ? lap * g2_of<K>(a, e) : 0.0);
#pragma unroll
                for (int g = 0; g < f; ++g) val -= L[e * (e + 1) / 2 + g] * L[f * (f + 1) / 2 + g];
                if (e == f) {
                    if (!(val > 0.0) || !(val <= kDblMax)) ok = false;
                    L[e * (e + 1) / 2 + f] = sqrt(val);
                } else {
                    L[e * (e + 1) / 2 + f] = val / L[f * (f + 1) / 2 + f];
                }
            }
        if (!ok) a.ctl[CTL_ERROR] = (double)GINGR_ERR_NOT_SPD;  // (every writer stores the same value)
        // J = L^-1 (lower), then B^-1 = J^T J
        double J[K * (K + 1) / 2];
#pragma unroll
        for (int f = 0; f < K; ++f)
#pragma unroll
            for (int e = f; e < K; ++e) {
                double val = e == f ? 1.0 : 0.0;
#pragma unroll
                for (int g = f; g < e; ++g) val -= L[e * (e + 1) / 2 + g] * J[g * (g + 1) / 2 + f];
                J[e * (e + 1) / 2 + f] = val / L[e * (e + 1) / 2 + e];
            }
#pragma unroll
        for (int e = 0; e < K; ++e)
#pragma unroll
            for (int f = 0; f <= e; ++f) {
                double val = 0.0;
#pragma unroll
                for (int g = e; g < K; ++g) val += J[g * (g + 1) / 2 + e] * J[g * (g + 1) / 2 + f];
                a.minv[(int64_t)(e * (e + 1) / 2 + f) * a.n + i] = val;
            }
        // X0: zero displacement (T), the identity map [I3; 0] (A)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = a.t[(int64_t)c * a.n + i];
#pragma unroll
            for (int e = 0; e < K; ++e) {
                a.x[(int64_t)(c * K + e) * a.n + i] = (K == 4 && e == c) ? 1.0 : 0.0;
                const double b = q[e] * t;
                bb[c] += b * b;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotBB + c, bb[c], sh);
}

// the start of a recurrence and the closing pass in one: r = b - A x, z = B^-1 r, p = z, block partials of r.z and r.r
template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_residual_kernel(SparseArgs a) {
    __shared__ double sh[kThreads];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double rz[3] = {0.0, 0.0, 0.0}, rr[3] = {0.0, 0.0, 0.0};
    if (i < a.n) {
        double q[K], own[3 * K], r[3 * K], z[3 * K];
        load_q<K>(a, i, q);
        apply_row<K>(a, i, a.x, q, own, r);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = a.t[(int64_t)c * a.n + i];
#pragma unroll
            for (int e = 0; e < K; ++e) {
                r[c * K + e] = q[e] * t - r[c * K + e];
                rr[c] += r[c * K + e] * r[c * K + e];
            }
        }
        precondition<K>(a, i, r, z);
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) {
            a.r[(int64_t)m * a.n + i] = r[m];
            a.z[(int64_t)m * a.n + i] = z[m];
            a.p[(int64_t)m * a.n + i] = z[m];
            rz[m / K] += r[m] * z[m];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotRZ + c, rz[c], sh);
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotRR + c, rr[c], sh);
}

// one workgroup, behind the residual pass: the true residual, which columns still miss the stop rule, and the scalars in front of
// iteration `first` (the slot of its parity)
__global__ __launch_bounds__(kThreads) void nicp_sparse_start_kernel(SparseArgs a, int first) {
    __shared__ double sh[kThreads];
    double v[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) v[q] = sum_partials(a, q, sh);  // |b|^2, r.z, r.r
    if (threadIdx.x != 0) return;
    const int slot = 3 * (first & 1);
    bool all = true, finite = true;
    for (int c = 0; c < 3; ++c) {
        const bool frozen = v[kSlotRR + c] <= a.tol2 * v[kSlotBB + c];
        a.ctl[CTL_BB + c] = v[kSlotBB + c];
        a.ctl[CTL_RZ + slot + c] = v[kSlotRZ + c];
        a.ctl[CTL_RR + c] = v[kSlotRR + c];
        a.ctl[CTL_TRUE_RR + c] = v[kSlotRR + c];
        a.ctl[CTL_FROZEN + slot + c] = frozen ? 1.0 : 0.0;
        all = all && frozen;
        finite = finite && (v[kSlotBB + c] <= kDblMax) && (v[kSlotRR + c] <= kDblMax);
    }
    if (a.ctl[CTL_ERROR] == 0.0 && !finite) a.ctl[CTL_ERROR] = (double)GINGR_ERR_NONFINITE;
    const bool failed = a.ctl[CTL_ERROR] != 0.0;
    a.ctl[CTL_CONVERGED] = (all && !failed) ? 1.0 : 0.0;
    a.ctl[CTL_DONE] = (all || failed) ? 1.0 : 0.0;
}

template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_apply_kernel(SparseArgs a) {
    __shared__ double sh[kThreads];
    if (stopped(a, sh)) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double pap[3] = {0.0, 0.0, 0.0};
    if (i < a.n) {
        double q[K], own[3 * K], out[3 * K];
        load_q<K>(a, i, q);
        apply_row<K>(a, i, a.p, q, own, out);
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) {
            a.ap[(int64_t)m * a.n + i] = out[m];
            pap[m / K] += own[m] * out[m];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotPAP + c, pap[c], sh);
}

template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_update_kernel(SparseArgs a, int parity) {
    __shared__ double sh[kThreads];
    if (stopped(a, sh)) return;
    double step[3];
    bool broken = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double pap = sum_partials(a, kSlotPAP + c, sh);
        if (a.ctl[CTL_FROZEN + 3 * parity + c] != 0.0) {
            step[c] = 0.0;  // a column that has met the stop rule keeps its x and r to the bit
        } else {
            if (!(pap > 0.0) || !(pap <= kDblMax)) broken = true;  // A is not positive definite along p
            step[c] = a.ctl[CTL_RZ + 3 * parity + c] / pap;
        }
    }
    if (broken) {  // (the same verdict in every workgroup: nothing is updated)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.ctl[CTL_ERROR] = (double)GINGR_ERR_NOT_SPD;
            a.ctl[CTL_DONE] = 1.0;
        }
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double rz[3] = {0.0, 0.0, 0.0}, rr[3] = {0.0, 0.0, 0.0};
    if (i < a.n) {
        double r[3 * K], z[3 * K];
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) {
            const int64_t at = (int64_t)m * a.n + i;
            a.x[at] += step[m / K] * a.p[at];
            r[m] = a.r[at] - step[m / K] * a.ap[at];
            a.r[at] = r[m];
        }
        precondition<K>(a, i, r, z);
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) {
            a.z[(int64_t)m * a.n + i] = z[m];
            rz[m / K] += r[m] * z[m];
            rr[m / K] += r[m] * r[m];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotRZ + c, rz[c], sh);
#pragma unroll
    for (int c = 0; c < 3; ++c) put_partial(a, kSlotRR + c, rr[c], sh);
}

// `iteration`: the number of this iteration, from 0; parity = iteration & 1
template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_direction_kernel(SparseArgs a, int iteration) {
    __shared__ double sh[kThreads];
    if (stopped(a, sh)) return;
    const int parity = iteration & 1;
    double rz[3], rr[3], mix[3];
    bool frozen[3], all = true, finite = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rz[c] = sum_partials(a, kSlotRZ + c, sh);
        rr[c] = sum_partials(a, kSlotRR + c, sh);
        const bool was = a.ctl[CTL_FROZEN + 3 * parity + c] != 0.0;
        const double before = a.ctl[CTL_RZ + 3 * parity + c];
        frozen[c] = was || rr[c] <= a.tol2 * a.ctl[CTL_BB + c];
        mix[c] = (was || !(before > 0.0)) ? 0.0 : rz[c] / before;
        all = all && frozen[c];
        finite = finite && (rr[c] <= kDblMax);
    }
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.n) {
#pragma unroll
        for (int m = 0; m < 3 * K; ++m) {
            const int64_t at = (int64_t)m * a.n + i;
            a.p[at] = a.z[at] + mix[m / K] * a.p[at];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int c = 0; c < 3; ++c) {
            a.ctl[CTL_RZ + 3 * (parity ^ 1) + c] = rz[c];
            a.ctl[CTL_FROZEN + 3 * (parity ^ 1) + c] = frozen[c] ? 1.0 : 0.0;
            a.ctl[CTL_RR + c] = rr[c];
        }
        a.ctl[CTL_ITERATIONS] = (double)(iteration + 1);
        if (!finite) a.ctl[CTL_ERROR] = (double)GINGR_ERR_NONFINITE;
        if (all && finite) a.ctl[CTL_CONVERGED] = 1.0;
        if (all || !finite) a.ctl[CTL_DONE] = 1.0;
    }
}

// T: out = V + X;  A: out_i = [v_i, 1] X_i  (D X);  SoA [3][n]
template <int K>
__global__ __launch_bounds__(kThreads) void nicp_sparse_moved_kernel(SparseArgs a, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double r;
        if (K == 1) {
            r = a.v[(int64_t)c * a.n + i] + a.x[(int64_t)c * a.n + i];
        } else {
            const double *x = a.x + (int64_t)(c * 4) * a.n + i;
            r = ((a.v[i] * x[0] + a.v[a.n + i] * x[a.n]) + a.v[2 * a.n + i] * x[2 * a.n]) + x[3 * a.n];
        }
        out[(int64_t)c * a.n + i] = r;
    }
}

template <int K>
void enqueue_setup(gingr_ctx *ctx, const SparseArgs &a) {
    hipLaunchKernelGGL(nicp_sparse_setup_kernel<K>, dim3((unsigned)a.blocks), dim3(kThreads), 0, ctx->stream, a);
}

template <int K>
void enqueue_start(gingr_ctx *ctx, const SparseArgs &a, int first) {
    hipLaunchKernelGGL(nicp_sparse_residual_kernel<K>, dim3((unsigned)a.blocks), dim3(kThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(nicp_sparse_start_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, a, first);
}

template <int K>
void enqueue_iterations(gingr_ctx *ctx, const SparseArgs &a, int first, int count) {
    const dim3 grid((unsigned)a.blocks), block(kThreads);
    for (int k = first; k < first + count; ++k) {
        hipLaunchKernelGGL(nicp_sparse_apply_kernel<K>, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(nicp_sparse_update_kernel<K>, grid, block, 0, ctx->stream, a, k & 1);
        hipLaunchKernelGGL(nicp_sparse_direction_kernel<K>, grid, block, 0, ctx->stream, a, k);
    }
}

template <int K>
void enqueue_moved(gingr_ctx *ctx, const SparseArgs &a, double *out_soa) {
    hipLaunchKernelGGL(nicp_sparse_moved_kernel<K>, dim3((unsigned)a.blocks), dim3(kThreads), 0, ctx->stream, a, out_soa);
}

}  // namespace

struct gingr_nicp {
    gingr_ctx *ctx = nullptr;
    int device = 0;  // (destroy does not look at the context: a host language's finalizer may run it behind the context's own)
    int32_t kind = 0;
    int64_t n = 0;
    NicpGraph graph;
    std::vector<int32_t> lm_ids;
    // host staging of a step, sized once
    std::vector<double> hv, hs, ht, hx;
    bool solved = false;  // x holds the unknowns of a step that returned them
    std::vector<uint8_t> has_term, seen;
    DevBuf row_ptr, col, v, s, t, x, r, z, p, ap, minv, part, ctl, out, stage, done;
    PinnedWords pin;  // the control block's way to the host (pull_small, fitter.hip)
};

extern "C" {

void gingr_nicp_destroy(gingr_nicp *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);  // every step returns synchronised: nothing of the handle is in flight
    if (h->pin.pin) (void)hipHostFree(h->pin.pin);
    delete h;
}

int gingr_nicp_create(gingr_ctx *ctx, int32_t kind, int64_t n, int64_t n_edges, const int32_t *edges, int32_t n_lm, const int32_t *lm_ids,
                      gingr_nicp **out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (out) *out = nullptr;
    if (!out || (kind != 0 && kind != 1) || n < 1 || n_edges < 0 || n_lm < 0 || (n_edges > 0 && !edges) || (n_lm > 0 && !lm_ids) || n_lm > n)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: bad argument");
    if (n > (int64_t)INT32_MAX / 16) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: more than %d vertices", INT32_MAX / 16);
    for (int32_t l = 0; l < n_lm; ++l)
        if (lm_ids[l] < 0 || lm_ids[l] >= n) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: landmark id out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gingr_nicp *h = new gingr_nicp;
    h->ctx = ctx;
    h->device = ctx->device;
    h->kind = kind;
    h->n = n;
    auto fail = [&](int rc) {
        gingr_nicp_destroy(h);
        return rc;
    };
    int64_t bad = -1;
    const int grc = nicp_graph_build(n, n_edges, edges, &h->graph, &bad);
    if (grc == NICP_GRAPH_BAD_EDGE) return fail(gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: edge %lld is not p1 < p2 < n", (long long)bad));
    if (grc == NICP_GRAPH_DUPLICATE_EDGE)
        return fail(gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: edge %lld repeats an earlier edge", (long long)bad));
    if (grc != NICP_GRAPH_OK) return fail(gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_create: too many edges"));
    h->lm_ids.assign(lm_ids, lm_ids + n_lm);
    h->hv.resize((size_t)3 * n);
    h->hs.resize((size_t)n);
    h->ht.resize((size_t)3 * n);
    h->has_term.resize((size_t)n);
    h->hx.resize((size_t)(kind == 0 ? 3 : 12) * n);
    const size_t K = kind == 0 ? 1 : 4, planes = 3 * K * (size_t)n * sizeof(double);
    const int64_t blocks = ceil_div(n, kThreads);
    HANDLE_TRY(ctx, fail, h->row_ptr.alloc(h->graph.row_ptr.size() * sizeof(int32_t)));
    HANDLE_TRY(ctx, fail, h->col.alloc(h->graph.col.size() * sizeof(int32_t)));
    HANDLE_TRY(ctx, fail, h->v.alloc((size_t)3 * n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->s.alloc((size_t)n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->t.alloc((size_t)3 * n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->x.alloc(planes));
    HANDLE_TRY(ctx, fail, h->r.alloc(planes));
    HANDLE_TRY(ctx, fail, h->z.alloc(planes));
    HANDLE_TRY(ctx, fail, h->p.alloc(planes));
    HANDLE_TRY(ctx, fail, h->ap.alloc(planes));
    HANDLE_TRY(ctx, fail, h->minv.alloc((K * (K + 1) / 2) * (size_t)n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->part.alloc((size_t)blocks * kSlots * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->ctl.alloc(CTL_DOUBLES * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->out.alloc((size_t)3 * n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->stage.alloc((size_t)3 * n * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->done.alloc(sizeof(int32_t)));
    h->pin.pin_doubles = CTL_DOUBLES + 1;  // the last word is the flag
    HANDLE_TRY(ctx, fail, hipHostMalloc(reinterpret_cast<void **>(&h->pin.pin), h->pin.pin_doubles * sizeof(double), hipHostMallocDefault));
    memset(h->pin.pin, 0, h->pin.pin_doubles * sizeof(double));
    h->pin.done = h->done.as<int32_t>();
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&h->pin.pin_dev), h->pin.pin, 0) != hipSuccess) {
        (void)hipGetLastError();
        h->pin.pin_dev = nullptr;  // (pull_small then copies and synchronises)
    }
    HANDLE_TRY(ctx, fail, hipMemsetAsync(h->done.p, 0, sizeof(int32_t), ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->row_ptr.p, h->graph.row_ptr.data(), h->graph.row_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (!h->graph.col.empty())
        HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->col.p, h->graph.col.data(), h->graph.col.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HANDLE_TRY(ctx, fail, hipStreamSynchronize(ctx->stream));
    *out = h;
    return GINGR_OK;
}

int gingr_nicp_step(gingr_nicp *h, const double *moving_xyz, const double *w, const double *cp_xyz, const double *lm_target_xyz, double alpha,
                    double beta, double gamma, double rel_tol, int32_t max_iterations, double *out_xyz, double *out_lm_xyz,
                    gingr_nicp_info *info) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (info) memset(info, 0, sizeof(*info));
    const int64_t n = h->n;
    const int32_t n_lm = (int32_t)h->lm_ids.size();
    if (!moving_xyz || !w || !cp_xyz || !out_xyz || (n_lm > 0 && !lm_target_xyz) || !(alpha >= 0.0) || !(beta >= 0.0) || !(gamma >= 0.0) ||
        !(rel_tol <= 1.0))  // (also refuses a NaN)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_step: bad argument");
    h->solved = false;
    if (!(rel_tol > 0.0)) rel_tol = kDefaultRelTol;
    if (max_iterations <= 0) max_iterations = kDefaultMaxIterations;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // host side: the SoA template, the scale of q q^T and the core of the right-hand side per vertex (see SparseArgs)
    double *hv = h->hv.data(), *hs = h->hs.data(), *ht = h->ht.data();
    uint8_t *has_term = h->has_term.data();
    for (int64_t i = 0; i < n; ++i) {
        const double w2 = w[i] * w[i];
        hs[i] = w2;
        has_term[i] = w[i] != 0.0;
        for (int d = 0; d < 3; ++d) {
            hv[d * n + i] = moving_xyz[3 * i + d];
            ht[d * n + i] = h->kind == 0 ? w2 * (cp_xyz[3 * i + d] - moving_xyz[3 * i + d]) : w2 * cp_xyz[3 * i + d];
        }
    }
    if (h->kind == 0) {  // row l of the reference's A3 has its one in COLUMN l; B3 row l = beta (UL_l - V[id_l])
        for (int32_t l = 0; l < n_lm; ++l) {
            const int64_t id = h->lm_ids[(size_t)l];
            hs[l] += 1.0;
            has_term[l] = 1;
            for (int d = 0; d < 3; ++d) ht[d * n + l] += beta * (lm_target_xyz[3 * l + d] - moving_xyz[3 * id + d]);
        }
    } else {  // W(i, i) = 0 at the landmark vertices (:251-253), then beta^2 per landmark of the vertex
        for (int32_t l = 0; l < n_lm; ++l) {
            const int64_t id = h->lm_ids[(size_t)l];
            hs[id] = 0.0;
            has_term[id] = 0;
            for (int d = 0; d < 3; ++d) ht[d * n + id] = 0.0;
        }
        for (int32_t l = 0; l < n_lm; ++l) {
            const int64_t id = h->lm_ids[(size_t)l];
            hs[id] += beta * beta;
            if (beta > 0.0) has_term[id] = 1;
            for (int d = 0; d < 3; ++d) ht[d * n + id] += beta * beta * lm_target_xyz[3 * l + d];
        }
    }
    // a singular system is reported, not iterated on.  (alpha = 0 uncouples the vertices; the per-vertex Cholesky reports that case)
    if (alpha > 0.0 && nicp_graph_unanchored_component(h->graph, has_term, h->seen) >= 0)
        return gingr_set_error(ctx, GINGR_ERR_NOT_SPD,
                               "nicp_step: the normal equations are not positive definite (a mesh component without any weighted vertex or landmark)");
    SparseArgs a{};
    a.n = n;
    a.row_ptr = h->row_ptr.as<int32_t>();
    a.col = h->col.as<int32_t>();
    a.v = h->v.as<double>();
    a.s = h->s.as<double>();
    a.t = h->t.as<double>();
    a.alpha2 = alpha * alpha;
    a.gamma2 = gamma * gamma;
    a.tol2 = rel_tol * rel_tol;
    a.x = h->x.as<double>();
    a.r = h->r.as<double>();
    a.z = h->z.as<double>();
    a.p = h->p.as<double>();
    a.ap = h->ap.as<double>();
    a.minv = h->minv.as<double>();
    a.part = h->part.as<double>();
    a.ctl = h->ctl.as<double>();
    a.blocks = (int32_t)ceil_div(n, kThreads);
    HIP_TRY(ctx, hipMemcpyAsync(h->v.p, hv, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h->s.p, hs, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h->t.p, ht, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(h->ctl.p, 0, CTL_DOUBLES * sizeof(double), ctx->stream));  // also clears the error word of a failed step
    if (h->kind == 0) enqueue_setup<1>(ctx, a); else enqueue_setup<4>(ctx, a);
    double *ctl = h->pin.pin;
    for (int first = 0;;) {  // one round = a recurrence from the true residual of the current x; the last round is the closing pass alone
        if (h->kind == 0) enqueue_start<1>(ctx, a, first); else enqueue_start<4>(ctx, a, first);
        GINGR_TRY(check_launch(ctx));
        GINGR_TRY(pull_small(ctx, h->pin, a.ctl, CTL_DOUBLES, ctl));
        if (ctl[CTL_DONE] != 0.0 || first >= max_iterations) break;
        for (int enqueued = first;;) {
            const int count = std::min<int>(kChunk, max_iterations - enqueued);
            if (h->kind == 0) enqueue_iterations<1>(ctx, a, enqueued, count); else enqueue_iterations<4>(ctx, a, enqueued, count);
            enqueued += count;
            GINGR_TRY(check_launch(ctx));
            GINGR_TRY(pull_small(ctx, h->pin, a.ctl, CTL_DOUBLES, ctl));
            if (ctl[CTL_DONE] != 0.0 || enqueued >= max_iterations) break;
        }
        if (ctl[CTL_ERROR] != 0.0) break;
        first = (int)ctl[CTL_ITERATIONS];  // (the iterations behind `done` in the last chunk did nothing)
    }
    if (h->kind == 0) enqueue_moved<1>(ctx, a, h->out.as<double>()); else enqueue_moved<4>(ctx, a, h->out.as<double>());
    GINGR_TRY(check_launch(ctx));
    if (info) {
        info->iterations = (int32_t)ctl[CTL_ITERATIONS];
        info->converged = ctl[CTL_CONVERGED] != 0.0;
        for (int c = 0; c < 3; ++c) {
            info->residual[c] = sqrt(ctl[CTL_TRUE_RR + c]);
            info->rhs_norm[c] = sqrt(ctl[CTL_BB + c]);
        }
    }
    const int err = (int)ctl[CTL_ERROR];
    if (err == GINGR_ERR_NOT_SPD)
        return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "nicp_step: the normal equations are not positive definite (a vertex block or a search direction)");
    if (err) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "nicp_step: non-finite residual");
    GINGR_TRY(download_cloud(ctx, h->stage.as<double>(), h->out.as<double>(), n, out_xyz));
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(out_xyz[i])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "nicp_step: non-finite result");
    if (out_lm_xyz)  // N-ICP-A: DL X = the moved landmark vertices (:278-282); N-ICP-T has no such output: the moved vertices too
        for (int32_t l = 0; l < n_lm; ++l)
            for (int d = 0; d < 3; ++d) out_lm_xyz[3 * l + d] = out_xyz[3 * (int64_t)h->lm_ids[(size_t)l] + d];
    h->solved = true;
    if (ctl[CTL_CONVERGED] == 0.0)
        return gingr_set_error(ctx, GINGR_ERR_NOT_CONVERGED, "nicp_step: %d iterations without reaching the relative residual %g", (int)ctl[CTL_ITERATIONS],
                               rel_tol);
    return GINGR_OK;
}

int gingr_nicp_get_solution(gingr_nicp *h, double *x) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (!x) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "nicp_get_solution: null argument");
    if (!h->solved) return gingr_set_error(ctx, GINGR_ERR_STATE, "nicp_get_solution: no step has returned a solution");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n = h->n, K = h->kind == 0 ? 1 : 4;
    HIP_TRY(ctx, hipMemcpyAsync(h->hx.data(), h->x.p, h->hx.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n; ++i)  // device plane (c K + a) -> row (K i + a), column c
        for (int64_t e = 0; e < K; ++e)
            for (int64_t c = 0; c < 3; ++c) x[3 * (K * i + e) + c] = h->hx[(size_t)((c * K + e) * n + i)];
    return GINGR_OK;
}

}  // extern "C"
