// The exact order statistic of non-negative doubles on the device (C ABI in include/gingr_hip.h: gingr_order_statistic; the robust
// scale of the point-to-plane pairs, fitter_pairs.hip).  Plan, key and digits: robust_select_plan.h.
//   rank kernel     one workgroup: the number of keys that take part (the sum of the residual kernel's per-workgroup counts, or the
//                   caller's n) and the rank asked for (the lower median's, or the caller's k)
//   pass kernel     kPasses launches, most significant digit first.  Every workgroup first re-derives, from the partial counts of the
//                   pass before, the bucket that pass chose -- the same integers summed by every workgroup, so the same bucket -- then
//                   counts the next digit of the keys that carry the chosen digits in an LDS histogram and writes its counts
//   finish kernel   one workgroup: the last bucket; the chosen digits are the key of rank k.  With robust parameters also the scale c
// A kernel boundary is the only synchronisation between passes: no flag, no atomic on global memory, no float atomic, nothing read by
// the host.  Counts are integers, so the sums do not depend on an order; they are taken in ascending workgroup order all the same.
#include "fitter.h"
#include "robust_select_plan.h"

namespace rsp = robust_select_plan;

// sel: [0] n, [1] k, [2] the selected key, [3] c, then per pass p the record [4 + 2 p], [5 + 2 p] it starts from
static_assert(kRobustSelWords >= 4 + 2 * rsp::kPasses, "the selection's words");

namespace {

// The bucket pass q chose, in every thread of the workgroup: (digits 0 .. q of the key of rank k, the rank left within that bucket).
// sel[4 + 2 q], sel[5 + 2 q]: the digits chosen before pass q and the rank among the keys that carry them.  sh [kBins], out [2]: LDS.
__device__ __forceinline__ void derive_bucket(int q, const uint32_t *__restrict__ counts, int G, const uint64_t *__restrict__ sel,
                                              uint32_t *sh, uint64_t *out, uint64_t &prefix, uint64_t &rank) {
    const int t = threadIdx.x;
    uint32_t total = 0;
    for (int g = 0; g < G; ++g) total += counts[((int64_t)q * G + g) * rsp::kBins + t];
    const uint64_t before = sel[4 + 2 * q], k = sel[5 + 2 * q];
    sh[t] = total;
    if (t == 0) out[0] = (before << rsp::kDigitBits) | (uint64_t)(rsp::kBins - 1), out[1] = 0;  // (a rank past the keys: never, for k < n)
    __syncthreads();
    for (int off = 1; off < rsp::kBins; off <<= 1) {  // inclusive scan over the bins
        const uint32_t v = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    const uint64_t incl = sh[t], excl = incl - total;
    if (excl <= k && k < incl) out[0] = (before << rsp::kDigitBits) | (uint64_t)t, out[1] = k - excl;
    __syncthreads();
    prefix = out[0], rank = out[1];
    __syncthreads();  // (sh and out are used again by the caller)
}

// sel[0] = n, sel[1] = k, and the record pass 0 starts from.  parts != nullptr: n = the sum of parts [nparts], k = the lower median's rank
// (0 for n = 0: the selection then runs over sentinels and the finish kernel reports "no value").  One workgroup.
__global__ __launch_bounds__(rsp::kThreads) void select_rank_kernel(int64_t nparts, const int32_t *__restrict__ parts, int64_t n_fixed,
                                                                    int64_t k_fixed, uint64_t *__restrict__ sel) {
    __shared__ unsigned long long sum;
    const int t = threadIdx.x;
    if (t == 0) sum = 0;
    __syncthreads();
    if (parts) {
        unsigned long long mine = 0;
        for (int64_t j = t; j < nparts; j += rsp::kThreads) mine += (unsigned long long)parts[j];
        atomicAdd(&sum, mine);  // (LDS, integers: the same total in any order)
    }
    __syncthreads();
    if (t != 0) return;
    const int64_t n = parts ? (int64_t)sum : n_fixed;
    const int64_t k = parts ? (n > 0 ? rsp::lower_median_rank(n) : 0) : k_fixed;
    sel[0] = (uint64_t)n, sel[1] = (uint64_t)k;
    sel[4] = 0, sel[5] = (uint64_t)k;
}

// Pass p over keys [n]; counts [kPasses][G][kBins], G = gridDim.x
__global__ __launch_bounds__(rsp::kThreads) void select_pass_kernel(int p, int64_t n, const uint64_t *__restrict__ keys,
                                                                    uint32_t *__restrict__ counts, uint64_t *__restrict__ sel) {
    __shared__ uint32_t hist[rsp::kBins], sh[rsp::kBins];
    __shared__ uint64_t out[2];
    const int t = threadIdx.x, G = (int)gridDim.x;
    uint64_t prefix = 0, rank = 0;
    if (p > 0) {
        derive_bucket(p - 1, counts, G, sel, sh, out, prefix, rank);
        if (blockIdx.x == 0 && t == 0) sel[4 + 2 * p] = prefix, sel[5 + 2 * p] = rank;  // read by pass p + 1, behind the kernel boundary
    }
    hist[t] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * rsp::kThreads + t; i < n; i += (int64_t)G * rsp::kThreads) {
        const uint64_t key = keys[i];
        if (rsp::prefix_of(key, p) == prefix) atomicAdd(&hist[rsp::digit_of(key, p)], 1u);
    }
    __syncthreads();
    counts[((int64_t)p * G + blockIdx.x) * rsp::kBins + t] = hist[t];
}

// sel[2] = the key of rank k (0 when nothing takes part), sel[3] = the scale c as a double's bits (robust != 0):
//   scale_mode 0: c = scale;  1: c = (scale * 1.4826) * sqrt(selected);  then c = max(c, min_scale);  nothing takes part: c = 0
__global__ __launch_bounds__(rsp::kThreads) void select_finish_kernel(const uint32_t *__restrict__ counts, int G, uint64_t *__restrict__ sel,
                                                                      int robust, int scale_mode, double scale, double min_scale) {
    __shared__ uint32_t sh[rsp::kBins];
    __shared__ uint64_t out[2];
    uint64_t key, rank;
    derive_bucket(rsp::kPasses - 1, counts, G, sel, sh, out, key, rank);
    if (threadIdx.x != 0) return;
    const int64_t n = (int64_t)sel[0];
    if (n <= 0) key = 0;
    sel[2] = key;
    if (!robust) return;
    double c = scale_mode == 0 ? scale : (scale * 1.4826) * sqrt(rsp::value_of(key));
    c = c >= min_scale ? c : min_scale;
    if (n <= 0) c = 0.0;
    sel[3] = rsp::key_of(c);
}

// keys of the stateless operator: the bits of v + 0 (-0 becomes +0; the host has refused what is negative or NaN)
__global__ __launch_bounds__(256) void order_keys_kernel(int64_t n, const double *__restrict__ v, uint64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = rsp::key_of(v[i] + 0.0);
}

}  // namespace

void robust_select_enqueue(gingr_ctx *ctx, int64_t n_keys, const uint64_t *keys, int64_t nparts, const int32_t *parts, int64_t n_fixed,
                           int64_t k_fixed, uint32_t *counts, uint64_t *sel, const gingr_robust_params *robust) {
    const int G = rsp::groups(n_keys);
    hipLaunchKernelGGL(select_rank_kernel, dim3(1), dim3(rsp::kThreads), 0, ctx->stream, nparts, parts, n_fixed, k_fixed, sel);
    for (int p = 0; p < rsp::kPasses; ++p)
        hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)G), dim3(rsp::kThreads), 0, ctx->stream, p, n_keys, keys, counts, sel);
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(rsp::kThreads), 0, ctx->stream, counts, G, sel, robust ? 1 : 0,
                       robust ? (int)robust->scale_mode : 0, robust ? robust->scale : 0.0, robust ? robust->min_scale : 0.0);
}

extern "C" int gingr_order_statistic(gingr_ctx *ctx, int64_t n, const double *values, int64_t k, double *out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!values || !out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "order_statistic: null argument");
    if (n < 1 || n > rsp::kMaxKeys) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "order_statistic: n = %lld outside 1 .. 2^31 - 1", (long long)n);
    if (k < 0 || k >= n) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "order_statistic: k = %lld outside [0, %lld)", (long long)k, (long long)n);
    for (int64_t i = 0; i < n; ++i)
        if (!(values[i] >= 0.0))
            return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "order_statistic: value %lld is negative or NaN", (long long)i);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf vals, keys, counts, sel;
    HIP_TRY(ctx, vals.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, keys.alloc((size_t)n * sizeof(uint64_t)));
    HIP_TRY(ctx, counts.alloc((size_t)rsp::count_words(n) * sizeof(uint32_t)));
    HIP_TRY(ctx, sel.alloc((size_t)kRobustSelWords * sizeof(uint64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(vals.p, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(order_keys_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, vals.as<double>(), keys.as<uint64_t>());
    robust_select_enqueue(ctx, n, keys.as<uint64_t>(), 0, nullptr, n, k, counts.as<uint32_t>(), sel.as<uint64_t>(), nullptr);
    GINGR_TRY(check_launch(ctx));
    uint64_t key = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&key, sel.as<uint64_t>() + 2, sizeof key, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = rsp::value_of(key);
    return GINGR_OK;
}
