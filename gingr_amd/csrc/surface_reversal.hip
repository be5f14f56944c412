// The reversed correspondence direction of the surface ICP: one sort of the target vertices by the template vertex they map to,
// then one observation (or one row of sums) per template vertex.  One of the four users of hipcub (with fitter_pairs.hip, mesh_decimate.hip and cloud_knn.hip).
#include "surface.h"

#include <hipcub/hipcub.hpp>

namespace {

// ---- reversed correspondence direction (ClosestPointRegistrator.scala:34-49): N entries (template vertex, target vertex, w)
// keys[j] = template vertex of target j when accepted, else `sentinel` (sorts last); vals[j] = j
__global__ __launch_bounds__(256) void reversal_keys_kernel(int64_t N, const int32_t *__restrict__ nn_vertex,
                                                            const int32_t *__restrict__ pre, const int32_t *__restrict__ hit,
                                                            int32_t sentinel, int32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                            double *__restrict__ w01) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const bool rejected = (pre && pre[j]) || (hit && hit[j]) || nn_vertex[j] < 0;
    keys[j] = rejected ? sentinel : nn_vertex[j];
    vals[j] = (int32_t)j;
    if (w01) w01[j] = rejected ? 0.0 : 1.0;
}

// The accepted target vertices that map to template vertex i are a run of the (stably) sorted keys, summed in ascending target
// position: deterministic.
struct RunSum { double sx, sy, sz; int64_t k; };
__device__ __forceinline__ RunSum reversal_run_sum(int64_t i, int64_t N, const int32_t *skeys, const int32_t *svals, Cloud tgt) {
    int64_t lo = 0, hi = N;  // first position with key >= i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < (int32_t)i)
            lo = mid + 1;
        else
            hi = mid;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t k = 0;
    for (int64_t p = lo; p < N && skeys[p] == (int32_t)i; ++p, ++k) {
        const int32_t j = svals[p];
        sx += tgt.x[j];
        sy += tgt.y[j];
        sz += tgt.z[j];
    }
    return RunSum{sx, sy, sz, k};
}

// Per template vertex i: the mean of its run is the observed point and its length times 1 / sigma2 the observation weight (k isotropic
// observations of one point = one observation of their mean with k-fold precision).
__global__ __launch_bounds__(256) void reversal_gather_kernel(int64_t M, int64_t N, const int32_t *__restrict__ skeys,
                                                              const int32_t *__restrict__ svals, Cloud tgt,
                                                              const double *__restrict__ sigma2, double *__restrict__ obs,
                                                              double *__restrict__ weight_in) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const RunSum s = reversal_run_sum(i, N, skeys, svals, tgt);
    const double kk = s.k > 0 ? (double)s.k : 1.0;
    obs[i] = s.sx / kk;
    obs[M + i] = s.sy / kk;
    obs[2 * M + i] = s.sz / kk;
    weight_in[i] = (double)s.k / sigma2[0];
}

// Row shard (round 5): the same runs, for a RANGE of the target queries, left as sums -- out[4][M] = {sum x, sum y, sum z, count} per
// template vertex of the WHOLE template -- so that the shards' ranges add up to the totals with one all-reduce; every entry is
// written (zeros where no accepted query of the range maps to the vertex).
__global__ __launch_bounds__(256) void reversal_sums_kernel(int64_t M, int64_t N, const int32_t *__restrict__ skeys,
                                                            const int32_t *__restrict__ svals, Cloud tgt, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const RunSum s = reversal_run_sum(i, N, skeys, svals, tgt);
    out[i] = s.sx;
    out[M + i] = s.sy;
    out[2 * M + i] = s.sz;
    out[3 * M + i] = (double)s.k;
}

}  // namespace

// bits of the largest sort key of the reversed direction (template vertex ids 0 .. M - 1 and the sentinel M)
static int key_bits(int64_t M) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) <= M) ++b;
    return b;
}

size_t reversal_sort_temp_bytes(int64_t N) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                             (int32_t *)nullptr, (int)N);
    return bytes;
}

void launch_reversal_observations(gingr_ctx *ctx, int64_t M, Cloud tgt, const int32_t *nn_vertex, const int32_t *pre,
                                  const int32_t *hit, const double *sigma2_dev, int32_t *keys, int32_t *vals, int32_t *skeys,
                                  int32_t *svals, void *sort_temp, size_t sort_temp_bytes, double *w01_targets, double *obs_soa,
                                  double *weight_in) {
    const int64_t N = tgt.n;
    hipLaunchKernelGGL(reversal_keys_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, nn_vertex, pre, hit,
                       (int32_t)M, keys, vals, w01_targets);
    // LSD radix sort: stable, so equal keys keep ascending target positions; only the bits a key can have (keys <= M, the sentinel)
    (void)hipcub::DeviceRadixSort::SortPairs(sort_temp, sort_temp_bytes, keys, skeys, vals, svals, (int)N, 0, key_bits(M), ctx->stream);
    hipLaunchKernelGGL(reversal_gather_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, N, skeys, svals, tgt,
                       sigma2_dev, obs_soa, weight_in);
}

void launch_reversal_sums(gingr_ctx *ctx, int64_t M, Cloud tgt, const int32_t *nn_vertex, const int32_t *pre, const int32_t *hit,
                          int32_t *keys, int32_t *vals, int32_t *skeys, int32_t *svals, void *sort_temp, size_t sort_temp_bytes,
                          double *w01_targets, double *sums4) {
    const int64_t N = tgt.n;
    if (N > 0) {
        hipLaunchKernelGGL(reversal_keys_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, N, nn_vertex, pre, hit,
                           (int32_t)M, keys, vals, w01_targets);
        (void)hipcub::DeviceRadixSort::SortPairs(sort_temp, sort_temp_bytes, keys, skeys, vals, svals, (int)N, 0, key_bits(M), ctx->stream);
    }
    hipLaunchKernelGGL(reversal_sums_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, N, skeys, svals, tgt, sums4);
}
