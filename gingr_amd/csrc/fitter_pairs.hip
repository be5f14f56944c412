// Correspondences given by the caller -- flavour 3, "pairs" (C ABI in include/gingr_hip.h): the lists a host's getCorrespondence /
// getUncertainty produce, brought into the form phase 1 of the fitter already reads.
//   isotropic pairs   (pid, point, variance) x K  ->  one observation per vertex, once per gingr_fitter_set_pairs:
//                     keys kernel (global pid -> device row, or the sentinel M for another shard's rows), stable radix sort over the
//                     bits a key can have, one gather thread per local vertex that walks its run in ascending pair position.
//   covariance pairs  (pid, point, 3 x 3)          ->  in front of the landmarks in the list the landmark pass sums (gp_obs.hip)
//   dense covariance pairs (pid, point, 3 x 3) x K ->  one precision and one precision-weighted point per vertex, once per
//                     gingr_fitter_set_pairs_cov_dense: the same keys kernel and sort, a gather thread that adds the inverses;
//                     summed every iteration by the 3 x 3-weighted Gram pass (gp_gram_cov.hip)
//   point-to-plane pairs, made here           ->  the same planes written by one kernel from what the forward surface scan leaves
//                     (gingr_fitter_set_pairs_plane_async), and the loop around them with ICP's sigma2 schedule on the device
//                     (gingr_fitter_update_plane_async): no list, no transfer, no synchronisation
//   ... against a point cloud                 ->  the same again from what the forward point-cloud search leaves and a normal per target
//                     point (gingr_fitter_set_pairs_plane_cloud_async, gingr_fitter_update_plane_cloud_async)
//   ... robustly weighted                     ->  with gingr_fitter_set_plane_robust on, both routes put a residual kernel, the exact median
//                     (robust_select.hip) and the robust variant of their plane kernel behind the correspondence: a variance
//                     inflation u_i per vertex, still nothing but launches
// The phases themselves are in fitter_phases.hip (run_phase), the probabilistic queries next to their siblings.
#include "fitter.h"
#include "robust_select_plan.h"
#include "svd3.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace {

// keys[k] = device row of pair k when this shard owns its vertex, else `M` (sorts last); vals[k] = k.  pid: GLOBAL ids, checked on the
// host against [0, M_total)
__global__ __launch_bounds__(256) void pairs_keys_kernel(int64_t K, const int32_t *__restrict__ pid, int64_t row_begin, int64_t M,
                                                         const int32_t *__restrict__ iperm, int32_t *__restrict__ keys,
                                                         int32_t *__restrict__ vals) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int64_t l = (int64_t)pid[k] - row_begin;
    keys[k] = (l >= 0 && l < M) ? iperm[l] : (int32_t)M;
    vals[k] = (int32_t)k;
}

// Per local vertex i (device row): its pairs are a run of the stably sorted keys, walked in ascending pair position.
//   weight_in[i] = sum 1 / var_k,   obs[.][i] = (sum x_k / var_k) / weight_in[i];   no pair (or total weight 0): weight 0, obs 0
// -- k isotropic observations of one point are one observation of their precision-weighted mean (the identity the reversed ICP
// direction uses with equal weights: reversal_gather_kernel, surface_reversal.hip).  Non-finite values are passed on: they fail the posterior.
__global__ __launch_bounds__(256) void pairs_gather_kernel(int64_t M, int64_t K, const int32_t *__restrict__ skeys,
                                                           const int32_t *__restrict__ svals, const double *__restrict__ xyz,
                                                           const double *__restrict__ var, double *__restrict__ obs,
                                                           double *__restrict__ weight_in) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    int64_t lo = 0, hi = K;  // first position with key >= i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < (int32_t)i)
            lo = mid + 1;
        else
            hi = mid;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    for (int64_t p = lo; p < K && skeys[p] == (int32_t)i; ++p) {
        const int64_t k = svals[p];
        const double v = var[k];
        sw += 1.0 / v;
        sx += xyz[3 * k] / v;
        sy += xyz[3 * k + 1] / v;
        sz += xyz[3 * k + 2] / v;
    }
    const bool none = sw == 0.0;
    obs[i] = none ? 0.0 : sx / sw;
    obs[M + i] = none ? 0.0 : sy / sw;
    obs[2 * M + i] = none ? 0.0 : sz / sw;
    weight_in[i] = sw;
}

// The dense covariance list, per local vertex i (device row), over the same kind of sorted run:
//   prec6[.][i] = Lambda_i = sum_k Sigma_k^-1 (planes xx, xy, xz, yy, yz, zz),   obs[.][i] = Lambda_i^-1 sum_k Sigma_k^-1 x_k
// -- k observations of one point with their own covariances are one observation of their precision-weighted mean.  Both sums in
// ascending pair position; a single pair keeps its point bit for bit; no pair: all zero.  spd3_inverse (svd3.h) makes NaN of a matrix
// that is no covariance, which is passed on: it fails the posterior.
__global__ __launch_bounds__(256) void pairs_gather_cov_kernel(int64_t M, int64_t K, const int32_t *__restrict__ skeys,
                                                               const int32_t *__restrict__ svals, const double *__restrict__ xyz,
                                                               const double *__restrict__ cov, double *__restrict__ obs,
                                                               double *__restrict__ prec6) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    int64_t lo = 0, hi = K;  // first position with key >= i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < (int32_t)i)
            lo = mid + 1;
        else
            hi = mid;
    }
    double L[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, x1[3] = {0, 0, 0};
    int64_t n = 0;
    for (int64_t p = lo; p < K && skeys[p] == (int32_t)i; ++p, ++n) {
        const int64_t k = svals[p];
        double Ci[9];
        spd3_inverse(cov + 9 * k, Ci);
        const double x = xyz[3 * k], y = xyz[3 * k + 1], z = xyz[3 * k + 2];
        L[0] += Ci[0], L[1] += Ci[1], L[2] += Ci[2], L[3] += Ci[4], L[4] += Ci[5], L[5] += Ci[8];
        b[0] += Ci[0] * x + Ci[1] * y + Ci[2] * z;
        b[1] += Ci[3] * x + Ci[4] * y + Ci[5] * z;
        b[2] += Ci[6] * x + Ci[7] * y + Ci[8] * z;
        x1[0] = x, x1[1] = y, x1[2] = z;
    }
    if (n > 1) {
        const double Lf[9] = {L[0], L[1], L[2], L[1], L[3], L[4], L[2], L[4], L[5]};
        double Li[9];
        spd3_inverse(Lf, Li);
        x1[0] = Li[0] * b[0] + Li[1] * b[1] + Li[2] * b[2];
        x1[1] = Li[3] * b[0] + Li[4] * b[1] + Li[5] * b[2];
        x1[2] = Li[6] * b[0] + Li[7] * b[1] + Li[8] * b[2];
    }
    obs[i] = x1[0];
    obs[M + i] = x1[1];
    obs[2 * M + i] = x1[2];
#pragma unroll
    for (int q = 0; q < 6; ++q) prec6[q * M + i] = L[q];
}

// L = (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T (planes xx, xy, xz, yy, yz, zz) with v_t = ratio v_n: the closed-form inverse of
// v_t I + (v_n - v_t) n n^T for a unit n.  A normal that is zero or non-finite gives (1 / v_t) I; ratio 1 gives (1 / v_n) I exactly.
// The ONE body both point-to-plane kernels below share.
__device__ __forceinline__ void plane_precision(double nx, double ny, double nz, double vn, double ratio, double L[6]) {
    const double vt = ratio * vn;
    const double a = 1.0 / vt, b = 1.0 / vn - a;
    const double nn = (nx * nx + ny * ny) + nz * nz;  // (NaN fails both comparisons)
    if (!(nn > 0.0 && nn <= 1.79769313486231570815e308)) nx = ny = nz = 0.0;
    const double bx = b * nx, by = b * ny, bz = b * nz;
    L[0] = a + bx * nx, L[1] = bx * ny, L[2] = bx * nz;
    L[3] = a + by * ny, L[4] = by * nz, L[5] = a + bz * nz;
}

// Point-to-plane pairs made on the device, per local vertex i (device row), from what the forward surface scan left (phase0_surface):
// the closest surface point cp [3][M], the winning triangle's position in the target's triangle array and the 0/1 rejection weight.
// With n the stored unit normal of that triangle (tcn [3][Tt]), v_n = sigma2 along it and v_t = ratio sigma2 across it,
//   prec6[.][i] = (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T   (planes xx, xy, xz, yy, yz, zz),   obs[.][i] = cp[.][i] bit for bit
// -- the closed-form inverse of v_t I + (v_n - v_t) n n^T, nothing is inverted numerically; ratio 1 gives (1 / sigma2) I exactly.  A
// normal that is zero or non-finite (a degenerate target triangle) gives (1 / v_t) I.  reject != 0 and weight 0: no observation, all
// zero; reject == 0: every vertex is observed and w01 is set to 1, so that the surface getter reports the weights that were used.
// Thread 0 also notes in *live whether the state can still move (neither failed nor stopped): plane_schedule_kernel looks at it
// behind the update.
__global__ __launch_bounds__(256) void plane_pairs_kernel(int64_t M, int64_t Tt, const double *__restrict__ cp, const int32_t *__restrict__ tri_pos,
                                                          double *__restrict__ w01, const double *__restrict__ tcn, const DevState *__restrict__ st,
                                                          double ratio, int reject, double *__restrict__ obs, double *__restrict__ prec6,
                                                          int32_t *__restrict__ live) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *live = !(st->status == GINGR_FIT_MODEL_FLEXIBILITY_ERROR || st->stopped);
    if (i >= M) return;
    double x = 0.0, y = 0.0, z = 0.0, L[6] = {0, 0, 0, 0, 0, 0};
    const bool observed = !reject || w01[i] != 0.0;
    if (!reject) w01[i] = 1.0;
    if (observed) {
        x = cp[i], y = cp[M + i], z = cp[2 * M + i];
        const int64_t t = tri_pos[i];
        double nx = 0.0, ny = 0.0, nz = 0.0;
        if (t >= 0 && t < Tt) nx = tcn[t], ny = tcn[Tt + t], nz = tcn[2 * Tt + t];
        plane_precision(nx, ny, nz, st->sigma2, ratio, L);
    }
    obs[i] = x;
    obs[M + i] = y;
    obs[2 * M + i] = z;
#pragma unroll
    for (int q = 0; q < 6; ++q) prec6[q * M + i] = L[q];
}

// The same planes against a point cloud, per local vertex i (device row), from what the forward point-cloud search left
// (phase0_nearest_vertex): nn [M] the nearest target point as a position in the target's device order, nnd2 [M] its squared distance.
// obs[.][i] = that target point bit for bit, the normal is the one stored for it (tn [3][N]).  max2 > 0: a vertex with nnd2 > max2 is
// not observed (all zero); a match outside the target (never, for a finite fit) is not observed either.  *live as above.
__global__ __launch_bounds__(256) void plane_cloud_pairs_kernel(int64_t M, int64_t N, const double *__restrict__ tgt, const int32_t *__restrict__ nn,
                                                                const double *__restrict__ nnd2, const double *__restrict__ tn,
                                                                const DevState *__restrict__ st, double ratio, double max2,
                                                                double *__restrict__ obs, double *__restrict__ prec6, int32_t *__restrict__ live) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *live = !(st->status == GINGR_FIT_MODEL_FLEXIBILITY_ERROR || st->stopped);
    if (i >= M) return;
    double x = 0.0, y = 0.0, z = 0.0, L[6] = {0, 0, 0, 0, 0, 0};
    const int64_t t = nn[i];
    if (t >= 0 && t < N && !(max2 > 0.0 && nnd2[i] > max2)) {
        x = tgt[t], y = tgt[N + t], z = tgt[2 * N + t];
        plane_precision(tn[t], tn[N + t], tn[2 * N + t], st->sigma2, ratio, L);
    }
    obs[i] = x;
    obs[M + i] = y;
    obs[2 * M + i] = z;
#pragma unroll
    for (int q = 0; q < 6; ++q) prec6[q * M + i] = L[q];
}

// ---- robust weighting (C ABI: gingr_fitter_set_plane_robust).  The residual of an observed vertex in the metric of its observation,
//   s = e_n^2 + max(|d|^2 - e_n^2, 0) / ratio,   d = fit vertex - observed point,   e_n = n . d
// = sigma2 d^T Lambda d of the plane plane_precision writes: ratio 1 gives |d|^2 exactly, a normal that is zero or non-finite |d|^2 / ratio.
__device__ __forceinline__ double plane_residual(double dx, double dy, double dz, double nx, double ny, double nz, double ratio) {
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (ratio == 1.0) return d2;
    const double nn = (nx * nx + ny * ny) + nz * nz;  // (NaN fails both comparisons)
    if (!(nn > 0.0 && nn <= 1.79769313486231570815e308)) nx = ny = nz = 0.0;
    const double en = (nx * dx + ny * dy) + nz * dz, en2 = en * en;
    double tang = d2 - en2;  // (a normal is unit to rounding only: a few ulp below zero for d along it)
    if (tang < 0.0) tang = 0.0;
    return en2 + tang / ratio;
}

// The variance inflation u >= 1 of a residual s at scale c; 0: Tukey removes the vertex.  c == 0 (no observed vertex, or a perfect fit
// under the median scale): 1.  loss: 1 Cauchy, 2 Huber, 3 Tukey.
__device__ __forceinline__ double robust_inflation(int loss, double s, double c) {
    if (!(c > 0.0)) return 1.0;
    if (loss == 2) {
        const double q = sqrt(s) / c;
        return q > 1.0 ? q : 1.0;
    }
    const double r = (s / c) / c;  // (c * c may overflow or underflow where this does not)
    if (loss == 1) return 1.0 + r;
    if (s >= c * c || r >= 1.0) return 0.0;
    const double w = 1.0 - r;
    return 1.0 / (w * w);
}

// s, its selection key (the sentinel for a row that is not observed) and this workgroup's number of observed rows, one store each
__device__ __forceinline__ void residual_store(int64_t i, int64_t M, bool observed, double r, double *__restrict__ s, uint64_t *__restrict__ key,
                                               int32_t *__restrict__ parts) {
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    if (i < M) {
        s[i] = r;
        key[i] = observed ? robust_select_plan::key_of(r) : robust_select_plan::kSentinel;
    }
    if (observed) atomicAdd(&count, 1);
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = count;
}

// Residuals of the surface route, per device row, from what plane_pairs_kernel reads (w01 is only read here) and the fit [3][M]
__global__ __launch_bounds__(256) void plane_residual_kernel(int64_t M, int64_t Tt, const double *__restrict__ fit, const double *__restrict__ cp,
                                                             const int32_t *__restrict__ tri_pos, const double *__restrict__ w01,
                                                             const double *__restrict__ tcn, double ratio, int reject, double *__restrict__ s,
                                                             uint64_t *__restrict__ key, int32_t *__restrict__ parts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool observed = i < M && (!reject || w01[i] != 0.0);
    double r = 0.0;
    if (observed) {
        const int64_t t = tri_pos[i];
        double nx = 0.0, ny = 0.0, nz = 0.0;
        if (t >= 0 && t < Tt) nx = tcn[t], ny = tcn[Tt + t], nz = tcn[2 * Tt + t];
        r = plane_residual(fit[i] - cp[i], fit[M + i] - cp[M + i], fit[2 * M + i] - cp[2 * M + i], nx, ny, nz, ratio);
    }
    residual_store(i, M, observed, r, s, key, parts);
}

// ... and of the cloud route, from what plane_cloud_pairs_kernel reads
__global__ __launch_bounds__(256) void plane_cloud_residual_kernel(int64_t M, int64_t N, const double *__restrict__ fit, const double *__restrict__ tgt,
                                                                   const int32_t *__restrict__ nn, const double *__restrict__ nnd2,
                                                                   const double *__restrict__ tn, double ratio, double max2,
                                                                   double *__restrict__ s, uint64_t *__restrict__ key, int32_t *__restrict__ parts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = i < M ? (int64_t)nn[i] : -1;
    const bool observed = i < M && t >= 0 && t < N && !(max2 > 0.0 && nnd2[i] > max2);
    double r = 0.0;
    if (observed)
        r = plane_residual(fit[i] - tgt[t], fit[M + i] - tgt[N + t], fit[2 * M + i] - tgt[2 * N + t], tn[t], tn[N + t], tn[2 * N + t], ratio);
    residual_store(i, M, observed, r, s, key, parts);
}

// plane_pairs_kernel with the variance of every observed vertex inflated: v_n = sigma2 u_i, u_i = robust_inflation(s[i], c), c the scale
// the selection left in sel[3].  u [M]: what was used, 0 for a vertex that is not observed or that Tukey removes (all-zero planes).
__global__ __launch_bounds__(256) void plane_pairs_robust_kernel(int64_t M, int64_t Tt, const double *__restrict__ cp, const int32_t *__restrict__ tri_pos,
                                                                 double *__restrict__ w01, const double *__restrict__ tcn,
                                                                 const DevState *__restrict__ st, double ratio, int reject, int loss,
                                                                 const double *__restrict__ s, const uint64_t *__restrict__ sel,
                                                                 double *__restrict__ u, double *__restrict__ obs, double *__restrict__ prec6,
                                                                 int32_t *__restrict__ live) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *live = !(st->status == GINGR_FIT_MODEL_FLEXIBILITY_ERROR || st->stopped);
    if (i >= M) return;
    double x = 0.0, y = 0.0, z = 0.0, L[6] = {0, 0, 0, 0, 0, 0}, ui = 0.0;
    const bool observed = !reject || w01[i] != 0.0;
    if (!reject) w01[i] = 1.0;
    if (observed) ui = robust_inflation(loss, s[i], robust_select_plan::value_of(sel[3]));
    if (ui != 0.0) {
        x = cp[i], y = cp[M + i], z = cp[2 * M + i];
        const int64_t t = tri_pos[i];
        double nx = 0.0, ny = 0.0, nz = 0.0;
        if (t >= 0 && t < Tt) nx = tcn[t], ny = tcn[Tt + t], nz = tcn[2 * Tt + t];
        plane_precision(nx, ny, nz, st->sigma2 * ui, ratio, L);
    }
    u[i] = ui;
    obs[i] = x;
    obs[M + i] = y;
    obs[2 * M + i] = z;
#pragma unroll
    for (int q = 0; q < 6; ++q) prec6[q * M + i] = L[q];
}

// ... and plane_cloud_pairs_kernel likewise
__global__ __launch_bounds__(256) void plane_cloud_pairs_robust_kernel(int64_t M, int64_t N, const double *__restrict__ tgt, const int32_t *__restrict__ nn,
                                                                       const double *__restrict__ nnd2, const double *__restrict__ tn,
                                                                       const DevState *__restrict__ st, double ratio, double max2, int loss,
                                                                       const double *__restrict__ s, const uint64_t *__restrict__ sel,
                                                                       double *__restrict__ u, double *__restrict__ obs, double *__restrict__ prec6,
                                                                       int32_t *__restrict__ live) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *live = !(st->status == GINGR_FIT_MODEL_FLEXIBILITY_ERROR || st->stopped);
    if (i >= M) return;
    double x = 0.0, y = 0.0, z = 0.0, L[6] = {0, 0, 0, 0, 0, 0}, ui = 0.0;
    const int64_t t = nn[i];
    const bool observed = t >= 0 && t < N && !(max2 > 0.0 && nnd2[i] > max2);
    if (observed) ui = robust_inflation(loss, s[i], robust_select_plan::value_of(sel[3]));
    if (ui != 0.0) {
        x = tgt[t], y = tgt[N + t], z = tgt[2 * N + t];
        plane_precision(tn[t], tn[N + t], tn[2 * N + t], st->sigma2 * ui, ratio, L);
    }
    u[i] = ui;
    obs[i] = x;
    obs[M + i] = y;
    obs[2 * M + i] = z;
#pragma unroll
    for (int q = 0; q < 6; ++q) prec6[q * M + i] = L[q];
}

// ICP's sigma2 schedule behind a flavour-3 update (ICP.scala:65, :96-99; one thread), exactly where post_solve_kernel applies it for
// the ICP flavours: only a state that took the update (*live) and only an update that committed (pad == 0) moves sigma2, and the run's
// stopping rule compares sigma2 before and after -- the pairs update itself keeps sigma2, so its verdict is replaced here.
__global__ void plane_schedule_kernel(DevState *st, const int32_t *live, double step, double end, double stop_threshold) {
    if (!*live) return;
    const double before = st->sigma2;
    double after = before;
    if (st->pad == 0) {
        const double ns = before - step;
        after = ns > end ? ns : end;
        st->sigma2 = after;
    }
    st->stopped = (stop_threshold >= 0.0 && fabs(before - after) < stop_threshold) ? 1 : 0;
}

// sigma2 of the device state and of the scalars it was initialised from (one thread)
__global__ void set_sigma2_kernel(DevState *st, gingr_state_scalars *hs, double sigma2) {
    st->sigma2 = sigma2;
    hs->sigma2 = sigma2;
}

// bits of the largest sort key (device rows 0 .. M - 1 and the sentinel M)
int pair_key_bits(int64_t M) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) <= M) ++b;
    return b;
}

size_t pair_sort_temp_bytes(int64_t K) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                             (int32_t *)nullptr, (int)K);
    return bytes;
}

void free_pair_list(gingr_fitter *f) {
    void *ptrs[] = {f->ppid, f->pkeys, f->pvals, f->pskeys, f->psvals, f->pxyz, f->pvar, f->psort};
    for (void *q : ptrs) dev_free(q);
    f->ppid = f->pkeys = f->pvals = f->pskeys = f->psvals = nullptr;
    f->pxyz = f->pvar = nullptr;
    f->psort = nullptr;
    f->psort_bytes = 0;
    f->pairs_cap = -1;
}

// room for K pairs (grow only); failure-atomic as far as the capacity goes: pairs_cap is raised once everything exists
int reserve_pairs(gingr_fitter *f, int64_t K) {
    if (K <= f->pairs_cap) return GINGR_OK;
    gingr_ctx *ctx = f->ctx;
    free_pair_list(f);
    f->n_pairs = 0;
    const size_t n = (size_t)K;
    GINGR_TRY(dev_alloc(ctx, &f->ppid, n));
    GINGR_TRY(dev_alloc(ctx, &f->pkeys, n));
    GINGR_TRY(dev_alloc(ctx, &f->pvals, n));
    GINGR_TRY(dev_alloc(ctx, &f->pskeys, n));
    GINGR_TRY(dev_alloc(ctx, &f->psvals, n));
    GINGR_TRY(dev_alloc(ctx, &f->pxyz, 3 * n));
    GINGR_TRY(dev_alloc(ctx, &f->pvar, n));
    f->psort_bytes = pair_sort_temp_bytes(K);
    HIP_TRY(ctx, hipMalloc(&f->psort, f->psort_bytes ? f->psort_bytes : 8));
    f->pairs_cap = K;
    return GINGR_OK;
}

void free_dense_list(gingr_fitter *f) {
    void *ptrs[] = {f->dpid, f->dkeys, f->dvals, f->dskeys, f->dsvals, f->dxyz, f->dcov, f->dsort};
    for (void *q : ptrs) dev_free(q);
    f->dpid = f->dkeys = f->dvals = f->dskeys = f->dsvals = nullptr;
    f->dxyz = f->dcov = nullptr;
    f->dsort = nullptr;
    f->dsort_bytes = 0;
    f->dense_cap = -1;
}

// room for K dense covariance pairs (grow only), as reserve_pairs
int reserve_dense(gingr_fitter *f, int64_t K) {
    if (K <= f->dense_cap) return GINGR_OK;
    gingr_ctx *ctx = f->ctx;
    free_dense_list(f);
    f->n_dense = 0;
    const size_t n = (size_t)K;
    GINGR_TRY(dev_alloc(ctx, &f->dpid, n));
    GINGR_TRY(dev_alloc(ctx, &f->dkeys, n));
    GINGR_TRY(dev_alloc(ctx, &f->dvals, n));
    GINGR_TRY(dev_alloc(ctx, &f->dskeys, n));
    GINGR_TRY(dev_alloc(ctx, &f->dsvals, n));
    GINGR_TRY(dev_alloc(ctx, &f->dxyz, 3 * n));
    GINGR_TRY(dev_alloc(ctx, &f->dcov, 9 * n));
    f->dsort_bytes = pair_sort_temp_bytes(K);
    HIP_TRY(ctx, hipMalloc(&f->dsort, f->dsort_bytes ? f->dsort_bytes : 8));
    f->dense_cap = K;
    return GINGR_OK;
}

// dobs / dprec and the pass's workspace exist (the planes all zero before the first list)
int dense_ensure_planes(gingr_fitter *f) {
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    if (!f->dobs) {
        GINGR_TRY(dev_alloc(ctx, &f->dobs, (size_t)3 * M));
        HIP_TRY(ctx, hipMemsetAsync(f->dobs, 0, (size_t)3 * M * sizeof(double), ctx->stream));
    }
    if (!f->dprec) {
        GINGR_TRY(dev_alloc(ctx, &f->dprec, (size_t)6 * M));
        HIP_TRY(ctx, hipMemsetAsync(f->dprec, 0, (size_t)6 * M * sizeof(double), ctx->stream));
    }
    HIP_TRY(ctx, ensure(f->dense_ws, (size_t)gram_cov_ws_doubles(M, f->m->rp) * sizeof(double)));
    return GINGR_OK;
}

}  // namespace

int pairs_ensure_planes(gingr_fitter *f) {
    if (f->pobs && f->pwin) return GINGR_OK;
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    if (!f->pobs) GINGR_TRY(dev_alloc(ctx, &f->pobs, (size_t)3 * M));
    if (!f->pwin) GINGR_TRY(dev_alloc(ctx, &f->pwin, (size_t)M));
    HIP_TRY(ctx, hipMemsetAsync(f->pobs, 0, (size_t)3 * M * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(f->pwin, 0, (size_t)M * sizeof(double), ctx->stream));
    return GINGR_OK;
}

int pairs_rebuild_cov_list(gingr_fitter *f) {
    gingr_ctx *ctx = f->ctx;
    const size_t npc = (size_t)f->n_pc, nlm = f->h_lm_row.size(), n = npc + nlm;
    std::vector<int32_t> row(n ? n : 1);
    std::vector<double> xyz(3 * n + 1), cov(9 * n + 1);
    for (size_t k = 0; k < npc; ++k) {  // a vertex a landmark overrides loses its pairs (GingrAlgorithm.scala:288-296)
        const int32_t r = f->h_pc_row[k];
        row[k] = (r >= 0 && !f->h_lm_mask.empty() && f->h_lm_mask[(size_t)r]) ? -1 : r;
    }
    std::copy(f->h_pc_xyz.begin(), f->h_pc_xyz.end(), xyz.begin());
    std::copy(f->h_pc_cov.begin(), f->h_pc_cov.end(), cov.begin());
    std::copy(f->h_lm_row.begin(), f->h_lm_row.end(), row.begin() + npc);
    std::copy(f->h_lm_xyz.begin(), f->h_lm_xyz.end(), xyz.begin() + 3 * npc);
    std::copy(f->h_lm_cov.begin(), f->h_lm_cov.end(), cov.begin() + 9 * npc);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an update in flight may still read the old list)
    f->n_cat = 0;
    HIP_TRY(ctx, ensure(f->cat_pid, (n ? n : 1) * sizeof(int32_t)));
    HIP_TRY(ctx, ensure(f->cat_xyz, (3 * n + 1) * sizeof(double)));
    HIP_TRY(ctx, ensure(f->cat_cov, (9 * n + 1) * sizeof(double)));
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpy(f->cat_pid.p, row.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(f->cat_xyz.p, xyz.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(f->cat_cov.p, cov.data(), 9 * n * sizeof(double), hipMemcpyHostToDevice));
    }
    f->n_cat = (int32_t)n;
    return GINGR_OK;
}

void free_pairs(gingr_fitter *f) {
    free_pair_list(f);
    dev_free(f->pobs), dev_free(f->pwin);
    f->pobs = f->pwin = nullptr;
    f->n_pairs = 0;
    f->n_pc = 0;
    free_dense_list(f);
    dev_free(f->dobs), dev_free(f->dprec);
    f->dobs = f->dprec = nullptr;
    f->dense_ws.release();
    f->n_dense = 0;
    dev_free(f->plane_live);
    f->plane_live = nullptr;
    void *robust[] = {f->rs_s, f->rs_u, f->rs_key, f->rs_sel, f->rs_parts, f->rs_counts};
    for (void *q : robust) dev_free(q);
    f->rs_s = f->rs_u = nullptr;
    f->rs_key = f->rs_sel = nullptr;
    f->rs_parts = nullptr;
    f->rs_counts = nullptr;
    f->rs_fresh = false;
}

namespace {

// the buffers of the robust weighting exist (allocated on the first robust refresh, kept)
int robust_ensure(gingr_fitter *f) {
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    if (!f->rs_s) GINGR_TRY(dev_alloc(ctx, &f->rs_s, (size_t)M));
    if (!f->rs_u) GINGR_TRY(dev_alloc(ctx, &f->rs_u, (size_t)M));
    if (!f->rs_key) GINGR_TRY(dev_alloc(ctx, &f->rs_key, (size_t)M));
    if (!f->rs_parts) GINGR_TRY(dev_alloc(ctx, &f->rs_parts, (size_t)ceil_div(M, 256)));
    if (!f->rs_counts) GINGR_TRY(dev_alloc(ctx, &f->rs_counts, (size_t)robust_select_plan::count_words(M)));
    if (!f->rs_sel) GINGR_TRY(dev_alloc(ctx, &f->rs_sel, (size_t)kRobustSelWords));
    return GINGR_OK;
}

// the observed rows' lower median of rs_s and the scale c into rs_sel, behind a residual kernel
void robust_scale(gingr_fitter *f) {
    const int64_t M = f->m->M;
    robust_select_enqueue(f->ctx, M, f->rs_key, ceil_div(M, 256), f->rs_parts, 0, 0, f->rs_counts, f->rs_sel, &f->robust);
}

// what both point-to-plane entry points refuse, in the order of correspondence.h: ready, parameters, then what the flavour needs
int plane_check(gingr_fitter *f, const gingr_plane_params *p, const char *who) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (!p) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null parameters", who);
    if (!(p->tangent_over_normal >= 1.0 && p->tangent_over_normal <= 1.79769313486231570815e308))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: tangent_over_normal must be finite and >= 1", who);
    if (p->reject != 0 && p->reject != 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: reject must be 0 or 1", who);
    if (!f->Tm || !f->Tt || !f->surf_cp) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: no meshes set (gingr_fitter_set_meshes)", who);
    if (f->sharded() || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: single shard only", who);
    if (f->surface_method != 0 || f->reversed)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: the TriangularClosestPoint method in the forward direction only", who);
    return GINGR_OK;
}

// the forward surface scan of the current fit, then its planes; asynchronous.  The caller has run plane_check.
int plane_refresh(gingr_fitter *f, const gingr_plane_params &p) {
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    f->forget_posteriors();  // the same state with other pairs is another posterior
    f->n_dense = 0;  // (until everything below is in place)
    GINGR_TRY(dense_ensure_planes(f));
    if (!f->plane_live) GINGR_TRY(dev_alloc(ctx, &f->plane_live, 1));
    fitter_surface_scan(f);
    if (f->robust.loss != 0) {
        GINGR_TRY(robust_ensure(f));
        hipLaunchKernelGGL(plane_residual_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->Tt, f->fit, f->surf_cp,
                           f->surf_tri_pos, f->surf_w01, f->tcn, p.tangent_over_normal, (int)p.reject, f->rs_s, f->rs_key, f->rs_parts);
        robust_scale(f);
        hipLaunchKernelGGL(plane_pairs_robust_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->Tt, f->surf_cp,
                           f->surf_tri_pos, f->surf_w01, f->tcn, f->st, p.tangent_over_normal, (int)p.reject, (int)f->robust.loss, f->rs_s,
                           f->rs_sel, f->rs_u, f->dobs, f->dprec, f->plane_live);
        GINGR_TRY(check_launch(ctx));
        f->rs_fresh = true;
        f->n_dense = M;
        return GINGR_OK;
    }
    hipLaunchKernelGGL(plane_pairs_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->Tt, f->surf_cp, f->surf_tri_pos,
                       f->surf_w01, f->tcn, f->st, p.tangent_over_normal, (int)p.reject, f->dobs, f->dprec, f->plane_live);
    GINGR_TRY(check_launch(ctx));
    f->n_dense = M;  // one pair per vertex; the uploaded list's arrays are not read by an update
    return GINGR_OK;
}

// what the point-cloud entry points refuse, in the order of plane_check: ready, parameters, then what the flavour needs
int plane_cloud_check(gingr_fitter *f, const gingr_plane_cloud_params *p, const char *who) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (!p) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null parameters", who);
    if (!(p->tangent_over_normal >= 1.0 && p->tangent_over_normal <= 1.79769313486231570815e308))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: tangent_over_normal must be finite and >= 1", who);
    if (p->max_distance != p->max_distance) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: max_distance is NaN", who);
    if (!f->tnormals)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: no target normals (gingr_fitter_set_target_normals / _estimate_target_normals)", who);
    if (f->sharded() || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: single shard only", who);
    return GINGR_OK;
}

// the forward point-cloud search of the current fit, then its planes; asynchronous.  The caller has run plane_cloud_check.
int plane_cloud_refresh(gingr_fitter *f, const gingr_plane_cloud_params &p) {
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    f->forget_posteriors();  // the same state with other pairs is another posterior
    f->n_dense = 0;  // (until everything below is in place)
    GINGR_TRY(dense_ensure_planes(f));
    if (!f->plane_live) GINGR_TRY(dev_alloc(ctx, &f->plane_live, 1));
    fitter_cloud_scan(f);
    const double max2 = p.max_distance > 0.0 ? p.max_distance * p.max_distance : 0.0;
    if (f->robust.loss != 0) {
        GINGR_TRY(robust_ensure(f));
        hipLaunchKernelGGL(plane_cloud_residual_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->N, f->fit, f->target,
                           f->nn_idx, f->nn_d2, f->tnormals, p.tangent_over_normal, max2, f->rs_s, f->rs_key, f->rs_parts);
        robust_scale(f);
        hipLaunchKernelGGL(plane_cloud_pairs_robust_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->N, f->target,
                           f->nn_idx, f->nn_d2, f->tnormals, f->st, p.tangent_over_normal, max2, (int)f->robust.loss, f->rs_s, f->rs_sel,
                           f->rs_u, f->dobs, f->dprec, f->plane_live);
        GINGR_TRY(check_launch(ctx));
        f->rs_fresh = true;
        f->n_dense = M;
        return GINGR_OK;
    }
    hipLaunchKernelGGL(plane_cloud_pairs_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, f->N, f->target, f->nn_idx, f->nn_d2,
                       f->tnormals, f->st, p.tangent_over_normal, max2, f->dobs, f->dprec, f->plane_live);
    GINGR_TRY(check_launch(ctx));
    f->n_dense = M;  // one pair per vertex; the uploaded list's arrays are not read by an update
    return GINGR_OK;
}

// the loop both point-to-plane updates run: n_iterations times { refresh the planes; one pairs update; ICP's schedule on the device }
template <typename Refresh>
int plane_loop(gingr_fitter *f, const gingr_icp_params *schedule, int32_t n_iterations, const char *who, Refresh refresh) {
    gingr_ctx *ctx = f->ctx;
    if (n_iterations < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n_iterations < 1", who);
    if (!schedule || schedule->max_iterations < 1)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the schedule needs max_iterations >= 1", who);
    const double step = (schedule->initial_sigma - schedule->end_sigma) / (double)schedule->max_iterations;  // ICP.scala:65
    const Correspondence pairs = abi_correspondence(3, nullptr, nullptr);
    for (int32_t it = 0; it < n_iterations; ++it) {
        GINGR_TRY(refresh());
        GINGR_TRY(fitter_update(f, pairs, 1));
        hipLaunchKernelGGL(plane_schedule_kernel, dim3(1), dim3(1), 0, ctx->stream, f->st, f->plane_live, step, schedule->end_sigma,
                           f->stop_threshold);
        f->forget_posteriors();  // sigma2 is part of the state the memo is keyed by
    }
    return check_launch(ctx);
}

}  // namespace

extern "C" {

int gingr_fitter_set_pairs(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *var) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (K < 0 || K > INT32_MAX || (K > 0 && (!pid || !xyz || !var))) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs: bad argument");
    for (int64_t k = 0; k < K; ++k)
        if (pid[k] < 0 || pid[k] >= m->M_total)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs: point id %d of pair %lld outside the model's %lld points", pid[k],
                                   (long long)k, (long long)m->M_total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    f->forget_posteriors();  // the same state with other pairs is another posterior
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an update in flight reads the planes)
    GINGR_TRY(pairs_ensure_planes(f));
    const int64_t M = m->M;
    if (K > 0) {
        GINGR_TRY(reserve_pairs(f, K));
        HIP_TRY(ctx, hipMemcpyAsync(f->ppid, pid, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f->pxyz, xyz, (size_t)3 * K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f->pvar, var, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(pairs_keys_kernel, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, ctx->stream, K, f->ppid, m->row_begin, M, m->iperm,
                           f->pkeys, f->pvals);
        // LSD radix sort: stable, so equal keys keep ascending pair positions; only the bits a key can have (keys <= M, the sentinel)
        HIP_TRY(ctx, hipcub::DeviceRadixSort::SortPairs(f->psort, f->psort_bytes, f->pkeys, f->pskeys, f->pvals, f->psvals, (int)K, 0,
                                                        pair_key_bits(M), ctx->stream));
    }
    f->n_pairs = K;
    // (K = 0: no run is found, every vertex gets weight 0; the list pointers are not read)
    hipLaunchKernelGGL(pairs_gather_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, K, f->pskeys, f->psvals, f->pxyz, f->pvar,
                       f->pobs, f->pwin);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller's arrays are free again
    return GINGR_OK;
}

int gingr_fitter_set_pairs_cov(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *cov) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (K < 0 || K > (1 << 24) || (K > 0 && (!pid || !xyz || !cov))) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs_cov: bad argument");
    for (int64_t k = 0; k < K; ++k)
        if (pid[k] < 0 || pid[k] >= m->M_total)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs_cov: point id %d of pair %lld outside the model's %lld points", pid[k],
                                   (long long)k, (long long)m->M_total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    f->forget_posteriors();
    f->h_pc_row.assign((size_t)K, -1);
    for (int64_t k = 0; k < K; ++k) {
        const int64_t lp = (int64_t)pid[k] - m->row_begin;
        if (lp >= 0 && lp < m->M) f->h_pc_row[(size_t)k] = m->hiperm[(size_t)lp];  // device row of the original point
    }
    f->h_pc_xyz.clear(), f->h_pc_cov.clear();
    if (K > 0) {
        f->h_pc_xyz.assign(xyz, xyz + 3 * K);
        f->h_pc_cov.assign(cov, cov + 9 * K);
    }
    f->n_pc = (int32_t)K;
    return pairs_rebuild_cov_list(f);
}

int gingr_fitter_set_pairs_cov_dense(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *cov) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (K < 0 || K > (1 << 24) || (K > 0 && (!pid || !xyz || !cov)))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs_cov_dense: bad argument");
    for (int64_t k = 0; k < K; ++k)
        if (pid[k] < 0 || pid[k] >= m->M_total)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_pairs_cov_dense: point id %d of pair %lld outside the model's %lld points",
                                   pid[k], (long long)k, (long long)m->M_total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    f->forget_posteriors();  // the same state with other pairs is another posterior
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an update in flight reads the planes)
    const int64_t M = m->M;
    if (K == 0) {  // no list: nothing of it is launched again; the planes, where they exist, read as "no pair"
        f->n_dense = 0;
        if (f->dobs) HIP_TRY(ctx, hipMemsetAsync(f->dobs, 0, (size_t)3 * M * sizeof(double), ctx->stream));
        if (f->dprec) HIP_TRY(ctx, hipMemsetAsync(f->dprec, 0, (size_t)6 * M * sizeof(double), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return GINGR_OK;
    }
    f->n_dense = 0;  // (until everything below is in place)
    GINGR_TRY(dense_ensure_planes(f));
    GINGR_TRY(reserve_dense(f, K));
    HIP_TRY(ctx, hipMemcpyAsync(f->dpid, pid, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(f->dxyz, xyz, (size_t)3 * K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(f->dcov, cov, (size_t)9 * K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pairs_keys_kernel, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, ctx->stream, K, f->dpid, m->row_begin, M, m->iperm,
                       f->dkeys, f->dvals);
    // the stable sort of gingr_fitter_set_pairs: equal keys keep ascending pair positions
    HIP_TRY(ctx, hipcub::DeviceRadixSort::SortPairs(f->dsort, f->dsort_bytes, f->dkeys, f->dskeys, f->dvals, f->dsvals, (int)K, 0,
                                                    pair_key_bits(M), ctx->stream));
    hipLaunchKernelGGL(pairs_gather_cov_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, K, f->dskeys, f->dsvals, f->dxyz,
                       f->dcov, f->dobs, f->dprec);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller's arrays are free again
    f->n_dense = K;
    return GINGR_OK;
}

int gingr_fitter_get_pair_precisions(gingr_fitter *f, double *obs_xyz, double *prec6) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    if (!f->dobs || !f->dprec) {  // never set: no pair anywhere
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (obs_xyz) std::fill(obs_xyz, obs_xyz + 3 * M, 0.0);
        if (prec6) std::fill(prec6, prec6 + 6 * M, 0.0);
        return GINGR_OK;
    }
    DevBuf tmp;
    HIP_TRY(ctx, tmp.alloc((size_t)6 * M * sizeof(double)));
    if (obs_xyz) {  // back to the caller's point order
        launch_soa_to_aos(ctx, f->dobs, M, tmp.as<double>(), f->m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(obs_xyz, tmp.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (prec6) {  // planes in the caller's order on the device, interleaved per vertex here
        for (int q = 0; q < 6; ++q) launch_scatter(ctx, f->dprec + (int64_t)q * M, M, f->m->perm, tmp.as<double>() + (int64_t)q * M);
        std::vector<double> planes((size_t)6 * M);
        HIP_TRY(ctx, hipMemcpyAsync(planes.data(), tmp.p, (size_t)6 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < M; ++i)
            for (int q = 0; q < 6; ++q) prec6[6 * i + q] = planes[(size_t)q * M + i];
    }
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_fitter_get_pair_observations(gingr_fitter *f, double *obs_xyz, double *weight) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GINGR_TRY(pairs_ensure_planes(f));
    const int64_t M = f->m->M;
    DevBuf tmp, tmpw;
    if (obs_xyz) {  // back to the caller's point order
        HIP_TRY(ctx, tmp.alloc((size_t)3 * M * sizeof(double)));
        launch_soa_to_aos(ctx, f->pobs, M, tmp.as<double>(), f->m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(obs_xyz, tmp.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (weight) {
        HIP_TRY(ctx, tmpw.alloc((size_t)M * sizeof(double)));
        launch_scatter(ctx, f->pwin, M, f->m->perm, tmpw.as<double>());
        HIP_TRY(ctx, hipMemcpyAsync(weight, tmpw.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_fitter_set_sigma2(gingr_fitter *f, double sigma2) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!f->has_state) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_sigma2: no state set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(set_sigma2_kernel, dim3(1), dim3(1), 0, ctx->stream, f->st, f->hs_dev, sigma2);
    f->forget_posteriors();  // sigma2 is part of the state the memo is keyed by
    f->mh_saved = false;
    // a state the host knows by value stays known: its key ends in sigma2 (state_key_values)
    if (f->state_key_valid && f->state_key.v.size() == (size_t)f->m->r + 11)
        f->state_key.v.back() = sigma2;
    else
        f->state_key_valid = false;
    return check_launch(ctx);
}

int gingr_fitter_set_pairs_plane_async(gingr_fitter *f, const gingr_plane_params *p) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    GINGR_TRY(plane_check(f, p, "set_pairs_plane_async"));
    return plane_refresh(f, *p);
}

int gingr_fitter_update_plane_async(gingr_fitter *f, const gingr_plane_params *p, const gingr_icp_params *schedule, int32_t n_iterations) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    GINGR_TRY(plane_check(f, p, "update_plane_async"));
    return plane_loop(f, schedule, n_iterations, "update_plane_async", [&] { return plane_refresh(f, *p); });
}

int gingr_fitter_set_plane_robust(gingr_fitter *f, const gingr_robust_params *p) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    gingr_robust_params next = {0, 0, 0.0, 0.0};
    if (p && p->loss != 0) {
        if (p->loss < 0 || p->loss > 3) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_plane_robust: loss %d outside 0..3", (int)p->loss);
        if (p->scale_mode != 0 && p->scale_mode != 1)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_plane_robust: scale_mode %d outside 0..1", (int)p->scale_mode);
        if (!(p->scale > 0.0 && p->scale <= kDblMax)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_plane_robust: scale must be finite and > 0");
        if (!(p->min_scale >= 0.0 && p->min_scale <= kDblMax))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_plane_robust: min_scale must be finite and >= 0");
        if (f->sharded() || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_plane_robust: single shard only");
        next = *p;
    }
    f->robust = next;
    f->rs_fresh = false;  // what the buffers hold belongs to the setting before
    f->forget_posteriors();
    return GINGR_OK;
}

int gingr_fitter_get_plane_robust(gingr_fitter *f, double *s, double *u, double *selected, double *c, int64_t *n_observed) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (f->robust.loss == 0 || !f->rs_fresh) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_plane_robust: no robust refresh yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    DevBuf tmp;
    HIP_TRY(ctx, tmp.alloc((size_t)2 * M * sizeof(double)));
    if (s) {  // back to the caller's point order
        launch_scatter(ctx, f->rs_s, M, f->m->perm, tmp.as<double>());
        HIP_TRY(ctx, hipMemcpyAsync(s, tmp.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (u) {
        launch_scatter(ctx, f->rs_u, M, f->m->perm, tmp.as<double>() + M);
        HIP_TRY(ctx, hipMemcpyAsync(u, tmp.as<double>() + M, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    uint64_t words[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(words, f->rs_sel, sizeof words, hipMemcpyDeviceToHost, ctx->stream));
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_observed) *n_observed = (int64_t)words[0];
    if (selected) *selected = robust_select_plan::value_of(words[2]);
    if (c) *c = robust_select_plan::value_of(words[3]);
    return GINGR_OK;
}

int gingr_fitter_set_target_normals(gingr_fitter *f, const double *normals) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!normals) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_target_normals: null argument");
    if (!f->target || !f->aos) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_target_normals: no target set");
    const int64_t N = f->N;
    std::vector<double> unit((size_t)3 * N);
    for (int64_t j = 0; j < N; ++j) {
        const double x = normals[3 * j], y = normals[3 * j + 1], z = normals[3 * j + 2];
        if (!(fabs(x) <= kDblMax && fabs(y) <= kDblMax && fabs(z) <= kDblMax))
            return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "set_target_normals: normal %lld is not finite", (long long)j);
        const double big = std::max(fabs(x), std::max(fabs(y), fabs(z)));  // (scaled: no overflow, no underflow of the squares)
        double ux = 0.0, uy = 0.0, uz = 0.0;
        if (big > 0.0) {
            const double n2 = (x * x + y * y) + z * z;
            if (fabs(n2 - 1.0) <= 0x1p-48) {  // already unit to rounding: taken as it is
                ux = x, uy = y, uz = z;
            } else {
                const double sx = x / big, sy = y / big, sz = z / big, len = sqrt((sx * sx + sy * sy) + sz * sz);
                ux = sx / len, uy = sy / len, uz = sz / len;
            }
        }
        unit[(size_t)3 * j] = ux, unit[(size_t)3 * j + 1] = uy, unit[(size_t)3 * j + 2] = uz;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an update in flight reads the normals and the staging buffer)
    f->forget_posteriors();
    if (!f->tnormals) GINGR_TRY(dev_alloc(ctx, &f->tnormals, (size_t)3 * N));
    return upload_cloud(ctx, reinterpret_cast<double *>(f->aos), unit.data(), N, f->tnormals, f->tperm);
}

int gingr_fitter_estimate_target_normals(gingr_fitter *f, int32_t k, const double *viewpoint, gingr_cloud_knn_info *info) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!f->target) return gingr_set_error(ctx, GINGR_ERR_STATE, "estimate_target_normals: no target set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an update in flight reads the normals)
    f->forget_posteriors();
    const int64_t N = f->N;
    DevBuf fresh;  // (a refused call leaves the normals the fitter holds as they are)
    HIP_TRY(ctx, fresh.alloc((size_t)3 * N * sizeof(double)));
    GINGR_TRY(cloud_normals_device(ctx, cloud_of(f->target, N), f->tperm, k, viewpoint, fresh.as<double>(), 1, N, nullptr, info,
                                   "estimate_target_normals"));
    dev_free(f->tnormals);
    f->tnormals = fresh.as<double>();
    fresh.p = nullptr, fresh.bytes = 0;  // (the fitter owns it now)
    return GINGR_OK;
}

int gingr_fitter_get_target_normals(gingr_fitter *f, double *normals) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!normals) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "get_target_normals: null argument");
    if (!f->tnormals) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_target_normals: no target normals");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf stage;
    HIP_TRY(ctx, stage.alloc((size_t)3 * f->N * sizeof(double)));
    return download_cloud(ctx, stage.as<double>(), f->tnormals, f->N, normals, f->tperm);
}

int gingr_fitter_set_pairs_plane_cloud_async(gingr_fitter *f, const gingr_plane_cloud_params *p) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    GINGR_TRY(plane_cloud_check(f, p, "set_pairs_plane_cloud_async"));
    return plane_cloud_refresh(f, *p);
}

int gingr_fitter_update_plane_cloud_async(gingr_fitter *f, const gingr_plane_cloud_params *p, const gingr_icp_params *schedule,
                                          int32_t n_iterations) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    GINGR_TRY(plane_cloud_check(f, p, "update_plane_cloud_async"));
    return plane_loop(f, schedule, n_iterations, "update_plane_cloud_async", [&] { return plane_cloud_refresh(f, *p); });
}

}  // extern "C"
