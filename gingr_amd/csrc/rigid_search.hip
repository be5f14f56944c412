// Global rigid pre-alignment: S start poses of one template advanced together through K iterations of trimmed ICP against a target
// cloud, and the best of them (C ABI in include/gingr_hip.h: gingr_rigid_search, gingr_rotation_samples; planning, the spiral of start
// rotations and the slabs: rigid_search_plan.h; the definition in numpy: tests/rigid_search_restatement.py).  The template is stored
// once, a pose is 12 doubles, and every pose of a slab advances in the same launches:
//   pose kernel     p = R_s x + t_s for every (pose, point): the query cloud of the slab, SoA, pose-major.  Always from the original
//                   points and the composed pose, so the pose that is returned reproduces the points exactly
//   search          the exact grid search over the whole query cloud (nn_grid.hip), then the masked tile scan for what it flagged
//                   (nn_scan.hip) -- many queries in the first iterations of a bad start, which is what the tile scan is for; from
//                   the second iteration on every query starts from its previous match
//   selection       overlap < 1 only: the exact radix selection of robust_select.hip (key, digits and passes of robust_select_plan.h)
//                   with the pose as the second grid dimension: kPasses launches for all poses, not one selection per pose.  The
//                   rank is known on the host (keep - 1), so there is no rank kernel, and the sums kernel derives the last bucket
//                   itself, so there is no finish kernel
//   sums kernel     per (pose, workgroup) the 17 sums over the kept pairs, centred on mean Y: block partials in a fixed order
//   step kernel     one pose per lane: the partials summed in workgroup order, dR = the Kabsch rotation (polar factor, else svd3 with
//                   the determinant fix: kabsch3_rotation of svd3.h), dt, the composed pose; on the scoring pass score and kept count
//   argmin kernel   one workgroup: the smallest score, the lowest pose on ties
// gingr_rigid_search_poses is the same run from start poses the caller gives (a non-finite one is failed from the beginning), with two
// additions behind the scoring pass: an inlier kernel (a workgroup per pose: the integer count of d2 <= distance^2 over ALL moving
// points, LDS integers) and, for select = 1, a selection kernel (most inliers, then the smaller score, then the lowest pose).  Both
// entries run run_search below; gingr_rigid_search only builds its start poses first.
// A kernel boundary is the only synchronisation; no float atomic, integer counts in LDS only; nothing is read back before the end.
// No sum reaches across poses and the grids of the segmented kernels depend on M alone, so a pose's bits do not depend on its slab.
#include "common.h"
#include "cloud_sums.h"
#include "rigid_search_plan.h"
#include "rigid_step.h"
#include "robust_select_plan.h"
#include "svd3.h"

#include <cmath>
#include <vector>

namespace rsp = robust_select_plan;
namespace rs = rigid_search_plan;

namespace {

constexpr int kSelWords = 2 * rsp::kPasses;  // per pose and pass p the record (digits chosen before p, rank among the keys that carry them)

// slab-local views: everything below is indexed by the pose's place in its slab
struct SlabSel {
    uint32_t *counts;  // [poses][kPasses][G][kBins]
    uint64_t *sel;     // [poses][kSelWords]
    int G;
    uint64_t k0;       // keep - 1
};

__global__ __launch_bounds__(256) void search_pose_kernel(Cloud x, const double *__restrict__ poses, const int32_t *__restrict__ failed,
                                                          double cx, double cy, double cz, int64_t Q, double *__restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (i >= x.n) return;
    const double *T = poses + rs::kPoseWords * s;
    const int64_t o = s * x.n + i;
    if (failed[s]) {  // takes no further part: its queries sit on mean Y, where the search is cheap and finite
        q[o] = cx, q[Q + o] = cy, q[2 * Q + o] = cz;
        return;
    }
    const double px = x.x[i], py = x.y[i], pz = x.z[i];
    q[o] = ((T[0] * px + T[1] * py) + T[2] * pz) + T[9];
    q[Q + o] = ((T[3] * px + T[4] * py) + T[5] * pz) + T[10];
    q[2 * Q + o] = ((T[6] * px + T[7] * py) + T[8] * pz) + T[11];
}

// The bucket pass q chose for the pose, in every thread of the workgroup (robust_select.hip: derive_bucket, with the pose's slices of
// the counts and records): (digits 0 .. q of the key of rank k, the rank left within that bucket).  sh [kBins], out [2]: LDS.
__device__ __forceinline__ void derive_pose_bucket(int q, const uint32_t *__restrict__ counts, int G, const uint64_t *__restrict__ sel, uint64_t k0,
                                                   uint32_t *sh, uint64_t *out, uint64_t &prefix, uint64_t &rank) {
    const int t = threadIdx.x;
    uint32_t total = 0;
    for (int g = 0; g < G; ++g) total += counts[((int64_t)q * G + g) * rsp::kBins + t];
    const uint64_t before = q == 0 ? 0 : sel[2 * q], k = q == 0 ? k0 : sel[2 * q + 1];
    sh[t] = total;
    if (t == 0) out[0] = (before << rsp::kDigitBits) | (uint64_t)(rsp::kBins - 1), out[1] = 0;  // (a rank past the keys: never, k < M)
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

// Pass p of every pose's selection over its d2 [M]; grid (G, poses).  The key of a distance: the bits of d2 + 0 (robust_select_plan.h).
__global__ __launch_bounds__(rsp::kThreads) void search_select_pass_kernel(int p, int64_t M, const double *__restrict__ d2, SlabSel ss) {
    __shared__ uint32_t hist[rsp::kBins], sh[rsp::kBins];
    __shared__ uint64_t out[2];
    const int t = threadIdx.x, G = ss.G;
    const int64_t s = blockIdx.y;
    uint32_t *counts = ss.counts + s * ((int64_t)rsp::kPasses * G * rsp::kBins);
    uint64_t *sel = ss.sel + s * kSelWords;
    uint64_t prefix = 0, rank = 0;
    if (p > 0) {
        derive_pose_bucket(p - 1, counts, G, sel, ss.k0, sh, out, prefix, rank);
        if (blockIdx.x == 0 && t == 0) sel[2 * p] = prefix, sel[2 * p + 1] = rank;  // read by pass p + 1, behind the kernel boundary
    }
    hist[t] = 0;
    __syncthreads();
    const double *d = d2 + s * M;
    for (int64_t i = (int64_t)blockIdx.x * rsp::kThreads + t; i < M; i += (int64_t)G * rsp::kThreads) {
        const uint64_t key = rsp::key_of(d[i] + 0.0);
        if (rsp::prefix_of(key, p) == prefix) atomicAdd(&hist[rsp::digit_of(key, p)], 1u);  // (LDS, integers)
    }
    __syncthreads();
    counts[((int64_t)p * G + blockIdx.x) * rsp::kBins + t] = hist[t];
}

// part [poses][B][kSums], B = gridDim.x: the sums over the kept pairs of the pose, centred on c.  idx: positions in the (Morton-
// ordered) target cloud t0.  trimmed: the kept pairs are those with key(d2) <= the key the selection's last pass leaves.
__global__ __launch_bounds__(rs::kSumThreads) void search_sums_kernel(int64_t M, int64_t Q, const double *__restrict__ q, Cloud t0,
                                                                      const int32_t *__restrict__ idx, const double *__restrict__ d2,
                                                                      int trimmed, SlabSel ss, double cx, double cy, double cz,
                                                                      double *__restrict__ part) {
    __shared__ double shd[rs::kSumThreads];
    __shared__ uint32_t sh[rsp::kBins];
    __shared__ uint64_t out[2];
    const int64_t s = blockIdx.y;
    uint64_t tau = ~(uint64_t)0, rank = 0;
    if (trimmed)
        derive_pose_bucket(rsp::kPasses - 1, ss.counts + s * ((int64_t)rsp::kPasses * ss.G * rsp::kBins), ss.G, ss.sel + s * kSelWords, ss.k0, sh,
                           out, tau, rank);
    double a[rs::kSums];
    for (int k = 0; k < rs::kSums; ++k) a[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * rs::kSumThreads + threadIdx.x; i < M; i += (int64_t)gridDim.x * rs::kSumThreads) {
        const int64_t o = s * M + i;
        const int64_t j = idx[o];
        if (j < 0 || j >= t0.n) {  // the scan leaves -1 for a query whose distances are all NaN: no read out of bounds; the NaN makes
            a[1] += __builtin_nan("");  // the pose non-finite, which the step kernel records
            continue;
        }
        const double d = d2[o];
        if (trimmed && rsp::key_of(d + 0.0) > tau) continue;
        const double p0 = q[o] - cx, p1 = q[Q + o] - cy, p2 = q[2 * Q + o] - cz;
        const double y0 = t0.x[j] - cx, y1 = t0.y[j] - cy, y2 = t0.z[j] - cz;
        a[0] += 1.0;
        a[1] += p0; a[2] += p1; a[3] += p2;
        a[4] += y0; a[5] += y1; a[6] += y2;
        a[7] += y0 * p0; a[8] += y0 * p1; a[9] += y0 * p2;
        a[10] += y1 * p0; a[11] += y1 * p1; a[12] += y1 * p2;
        a[13] += y2 * p0; a[14] += y2 * p1; a[15] += y2 * p2;
        a[16] += d;
    }
    block_sums<rs::kSums>(a, shd, part + (s * gridDim.x + blockIdx.x) * rs::kSums);
}

// One pose per lane.  last == 0: the pose composed with the step of its kept pairs; last != 0: score and kept count, the pose stays.
__global__ __launch_bounds__(rs::kStepThreads) void search_step_kernel(int64_t P, int B, const double *__restrict__ part, double cx, double cy,
                                                                       double cz, int last, double *__restrict__ poses,
                                                                       int32_t *__restrict__ failed, double *__restrict__ scores,
                                                                       int64_t *__restrict__ kept) {
    const int64_t s = (int64_t)blockIdx.x * rs::kStepThreads + threadIdx.x;
    if (s >= P) return;
    if (failed[s]) {
        if (last) scores[s] = __builtin_huge_val(), kept[s] = 0;
        return;
    }
    double S[rs::kSums];
    for (int k = 0; k < rs::kSums; ++k) S[k] = sum_partials(part + s * B * rs::kSums, B, rs::kSums, k);
    const double n = S[0];
    if (last) {
        const double score = sqrt(S[16] / n);
        const bool fin = finite_d(score) && finite_d(S[1]);  // (S[1] carries the NaN of a query without a match)
        scores[s] = fin ? score : __builtin_huge_val();
        kept[s] = fin ? (int64_t)n : 0;
        if (!fin) failed[s] = 1;
        return;
    }
    const double c[3] = {cx, cy, cz};
    double dR[9], dt[3];
    kabsch_step_from_sums(S, c, dR, dt);
    double *T = poses + rs::kPoseWords * s, Tn[rs::kPoseWords];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) Tn[a * 3 + b] = (dR[a * 3] * T[b] + dR[a * 3 + 1] * T[3 + b]) + dR[a * 3 + 2] * T[6 + b];
        Tn[9 + a] = ((dR[a * 3] * T[9] + dR[a * 3 + 1] * T[10]) + dR[a * 3 + 2] * T[11]) + dt[a];
    }
    bool fin = true;
    for (int k = 0; k < rs::kPoseWords; ++k) fin = fin && finite_d(Tn[k]);
    if (!fin) {  // the pose keeps its last finite value
        failed[s] = 1;
        return;
    }
    for (int k = 0; k < rs::kPoseWords; ++k) T[k] = Tn[k];
}

// *best = the pose of the smallest score that did not fail, the lowest index on ties; -1: every pose failed.  One workgroup.
__global__ __launch_bounds__(256) void search_argmin_kernel(int64_t S, const double *__restrict__ scores, const int32_t *__restrict__ failed,
                                                            int64_t *__restrict__ best) {
    __shared__ double shs[256];
    __shared__ int64_t shi[256];
    const int t = threadIdx.x;
    double bs = __builtin_huge_val();
    int64_t bi = -1;
    for (int64_t s = t; s < S; s += 256)  // ascending: a later pose replaces only on a strictly smaller score
        if (!failed[s] && (bi < 0 || scores[s] < bs)) bs = scores[s], bi = s;
    shs[t] = bs, shi[t] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            const double os = shs[t + off];
            const int64_t oi = shi[t + off];
            if (oi >= 0 && (shi[t] < 0 || os < shs[t] || (os == shs[t] && oi < shi[t]))) shs[t] = os, shi[t] = oi;
        }
        __syncthreads();
    }
    if (t == 0) *best = shi[0];
}

// inliers[s] = the moving points of pose s with d2 <= lim in the scoring pass (0 for a failed pose); a workgroup per pose
__global__ __launch_bounds__(256) void search_inliers_kernel(int64_t M, const double *__restrict__ d2, const int32_t *__restrict__ failed, double lim,
                                                             int64_t *__restrict__ inliers) {
    __shared__ uint32_t total;
    const int64_t s = blockIdx.x;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t n = 0;
    if (!failed[s])
        for (int64_t i = threadIdx.x; i < M; i += 256) n += d2[s * M + i] <= lim ? 1u : 0u;  // (a NaN is no inlier)
    if (n) atomicAdd(&total, n);  // (LDS, integers)
    __syncthreads();
    if (threadIdx.x == 0) inliers[s] = (int64_t)total;
}

// pose a before pose b: more inliers, then the smaller score, then the lower index
__device__ __forceinline__ bool better_pose(int64_t ia, double sa, int64_t a, int64_t ib, double sb, int64_t b) {
    return ia > ib || (ia == ib && (sa < sb || (sa == sb && a < b)));
}

// *best = the first pose by better_pose among those that did not fail; -1: every pose failed.  One workgroup.
__global__ __launch_bounds__(256) void search_select_inliers_kernel(int64_t S, const double *__restrict__ scores, const int64_t *__restrict__ inliers,
                                                                    const int32_t *__restrict__ failed, int64_t *__restrict__ best) {
    __shared__ int64_t shi[256];
    const int t = threadIdx.x;
    int64_t bi = -1;
    for (int64_t s = t; s < S; s += 256)
        if (!failed[s] && (bi < 0 || better_pose(inliers[s], scores[s], s, inliers[bi], scores[bi], bi))) bi = s;
    shi[t] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            const int64_t a = shi[t], o = shi[t + off];
            if (o >= 0 && (a < 0 || better_pose(inliers[o], scores[o], o, inliers[a], scores[a], a))) shi[t] = o;
        }
        __syncthreads();
    }
    if (t == 0) *best = shi[0];
}

bool all_finite(const double *v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

void mean3(const double *xyz, int64_t n, double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) out[d] += xyz[3 * i + d];
    for (int d = 0; d < 3; ++d) out[d] /= (double)n;
}

// the checks the two entries share; `who` names the entry in the message
int check_search(gingr_ctx *ctx, const char *who, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S, int32_t K,
                 double overlap) {
    if (M < 1 || M > INT32_MAX || N < 1 || N > INT32_MAX || S < 1 || S > INT32_MAX || K < 0)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld, N = %lld, S = %lld, K = %d: sizes >= 1 (below 2^31), K >= 0", who,
                               (long long)M, (long long)N, (long long)S, (int)K);
    if (!(overlap > 0.0 && overlap <= 1.0)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: overlap = %g outside (0, 1]", who, overlap);
    if (!all_finite(moving_xyz, 3 * M) || !all_finite(target_xyz, 3 * N))
        return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite coordinate", who);
    return GINGR_OK;
}

// what gingr_rigid_search_poses adds behind the scoring pass
struct SearchExtras {
    double inlier_lim;     // inlier_distance^2
    int select;            // 0: the smallest score; 1: the most inliers, then the smaller score, then the lowest pose
    int64_t *inliers_out;  // [S], nullable
};

// The run of both entries from the start poses `start` [S][12] (host; start_failed [S]: 1 = takes no part), sums centred on c = mean Y.
// extras == nullptr: gingr_rigid_search.
int run_search(gingr_ctx *ctx, const char *who, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S,
               const std::vector<double> &start, const std::vector<int32_t> &start_failed, const double c[3], int32_t K, double overlap,
               const SearchExtras *extras, int64_t *best_out, double *poses12_out, double *scores_out, int64_t *kept_out, int32_t *failed_out) {
    const int64_t slab = rs::slab_poses(M, N), Pmax = S < slab ? S : slab, Qmax = Pmax * M;
    const int64_t keep = rs::keep_count(M, overlap);
    const bool trimmed = keep < M;
    const int G = rsp::groups(M), B = rs::sum_blocks(M);
    int64_t ws_bytes = nn_ws_bytes(Qmax, N);
    if (S % slab != 0 && S > slab) {  // the last, shorter slab plans its own chunks
        const int64_t w = nn_ws_bytes((S % slab) * M, N);
        if (w > ws_bytes) ws_bytes = w;
    }
    DevBuf stage, tpl, tgt, torig, tboxes, ws, q, idx, d2, counts, sel, part, poses, failed, scores, kept, best, inliers;
    if (extras) HIP_TRY(ctx, inliers.alloc((size_t)S * sizeof(int64_t)));
    HIP_TRY(ctx, stage.alloc((size_t)3 * (M > N ? M : N) * sizeof(double)));
    HIP_TRY(ctx, tpl.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, tgt.alloc((size_t)3 * N * sizeof(double)));
    HIP_TRY(ctx, torig.alloc((size_t)N * sizeof(int32_t)));
    HIP_TRY(ctx, tboxes.alloc((size_t)30 * ceil_div(N, 256) * sizeof(double)));
    HIP_TRY(ctx, ws.alloc((size_t)ws_bytes));
    HIP_TRY(ctx, q.alloc((size_t)3 * Qmax * sizeof(double)));
    HIP_TRY(ctx, idx.alloc((size_t)Qmax * sizeof(int32_t)));
    HIP_TRY(ctx, d2.alloc((size_t)Qmax * sizeof(double)));
    if (trimmed) {
        HIP_TRY(ctx, counts.alloc((size_t)Pmax * rsp::kPasses * G * rsp::kBins * sizeof(uint32_t)));
        HIP_TRY(ctx, sel.alloc((size_t)Pmax * kSelWords * sizeof(uint64_t)));
    }
    HIP_TRY(ctx, part.alloc((size_t)Pmax * B * rs::kSums * sizeof(double)));
    HIP_TRY(ctx, poses.alloc((size_t)S * rs::kPoseWords * sizeof(double)));
    HIP_TRY(ctx, failed.alloc((size_t)S * sizeof(int32_t)));
    HIP_TRY(ctx, scores.alloc((size_t)S * sizeof(double)));
    HIP_TRY(ctx, kept.alloc((size_t)S * sizeof(int64_t)));
    HIP_TRY(ctx, best.alloc(sizeof(int64_t)));

    // the template as an SoA cloud; the target in k-d leaf order with its tile boxes and its grid, as gingr_rigid_icp_create lays it out
    GINGR_TRY(upload_cloud(ctx, stage.as<double>(), moving_xyz, M, tpl.as<double>()));
    std::vector<int32_t> order;
    kd_leaf_order(target_xyz, N, order);
    HIP_TRY(ctx, hipMemcpyAsync(torig.p, order.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GINGR_TRY(upload_cloud(ctx, stage.as<double>(), target_xyz, N, tgt.as<double>(), torig.as<int32_t>()));
    const double *x = tpl.as<double>(), *t = tgt.as<double>();
    const Cloud cx{x, x + M, x + 2 * M, M}, ct{t, t + N, t + 2 * N, N};
    launch_tile_bbox(ctx, ct, tboxes.as<double>());
    HIP_TRY(ctx, hipMemcpyAsync(poses.p, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(failed.p, start_failed.data(), (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GINGR_TRY(check_launch(ctx));
    struct GridOwner {
        NNGrid g;
        ~GridOwner() { nn_grid_free(&g); }
    } grid;
    if (nn_grid_build(ctx, target_xyz, N, order.data(), Qmax, &grid.g) != GINGR_OK) return GINGR_ERR_HIP;  // (message set; synchronises)
    const bool use_grid = ctx->nn_grid && grid.g.ready && ctx->cull;

    for (int64_t first = 0; first < S; first += slab) {
        const int64_t P = S - first < slab ? S - first : slab, Q = P * M;
        double *qs = q.as<double>(), *pose_s = poses.as<double>() + rs::kPoseWords * first;
        int32_t *failed_s = failed.as<int32_t>() + first;
        const Cloud cq{qs, qs + Q, qs + 2 * Q, Q};
        const SlabSel ss{counts.as<uint32_t>(), sel.as<uint64_t>(), G, (uint64_t)(keep - 1)};
        for (int32_t k = 0; k <= K; ++k) {  // K iterations, then the scoring pass
            const int last = k == K;
            {
                TimerScope ts(ctx, 26);
                hipLaunchKernelGGL(search_pose_kernel, dim3((unsigned)ceil_div(M, 256), (unsigned)P), dim3(256), 0, ctx->stream, cx, pose_s,
                                   failed_s, c[0], c[1], c[2], Q, qs);
            }
            const int32_t *warm = k > 0 ? idx.as<int32_t>() : nullptr;  // the previous iteration's matches of this slab
            if (use_grid) {
                if (!launch_nn_grid(ctx, cq, ct, torig.as<int32_t>(), grid.g, warm, idx.as<int32_t>(), d2.as<double>()))
                    launch_nn(ctx, cq, ct, torig.as<int32_t>(), tboxes.as<double>(), ws.p, idx.as<int32_t>(), d2.as<double>(), idx.as<int32_t>(),
                              grid.g.flag, grid.g.cur_nflag());
            } else {
                launch_nn(ctx, cq, ct, torig.as<int32_t>(), tboxes.as<double>(), ws.p, idx.as<int32_t>(), d2.as<double>(), warm);
            }
            if (trimmed) {
                TimerScope ts(ctx, 24);
                for (int p = 0; p < rsp::kPasses; ++p)
                    hipLaunchKernelGGL(search_select_pass_kernel, dim3((unsigned)G, (unsigned)P), dim3(rsp::kThreads), 0, ctx->stream, p, M,
                                       d2.as<double>(), ss);
            }
            {
                TimerScope ts(ctx, 25);
                hipLaunchKernelGGL(search_sums_kernel, dim3((unsigned)B, (unsigned)P), dim3(rs::kSumThreads), 0, ctx->stream, M, Q, qs, ct,
                                   idx.as<int32_t>(), d2.as<double>(), trimmed ? 1 : 0, ss, c[0], c[1], c[2], part.as<double>());
            }
            {
                TimerScope ts(ctx, 26);
                hipLaunchKernelGGL(search_step_kernel, dim3((unsigned)ceil_div(P, rs::kStepThreads)), dim3(rs::kStepThreads), 0, ctx->stream, P, B,
                                   part.as<double>(), c[0], c[1], c[2], last, pose_s, failed_s, scores.as<double>() + first,
                                   kept.as<int64_t>() + first);
                if (last && extras)  // (behind the step kernel: a pose it just failed counts nothing)
                    hipLaunchKernelGGL(search_inliers_kernel, dim3((unsigned)P), dim3(256), 0, ctx->stream, M, d2.as<double>(), failed_s,
                                       extras->inlier_lim, inliers.as<int64_t>() + first);
            }
        }
    }
    {
        TimerScope ts(ctx, 26);
        if (extras && extras->select == 1)
            hipLaunchKernelGGL(search_select_inliers_kernel, dim3(1), dim3(256), 0, ctx->stream, S, scores.as<double>(), inliers.as<int64_t>(),
                               failed.as<int32_t>(), best.as<int64_t>());
        else
            hipLaunchKernelGGL(search_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, S, scores.as<double>(), failed.as<int32_t>(),
                               best.as<int64_t>());
    }
    GINGR_TRY(check_launch(ctx));
    int64_t b = -1;
    HIP_TRY(ctx, hipMemcpyAsync(&b, best.p, sizeof b, hipMemcpyDeviceToHost, ctx->stream));
    if (poses12_out) HIP_TRY(ctx, hipMemcpyAsync(poses12_out, poses.p, (size_t)S * rs::kPoseWords * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (scores_out) HIP_TRY(ctx, hipMemcpyAsync(scores_out, scores.p, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (kept_out) HIP_TRY(ctx, hipMemcpyAsync(kept_out, kept.p, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (failed_out) HIP_TRY(ctx, hipMemcpyAsync(failed_out, failed.p, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (extras && extras->inliers_out)
        HIP_TRY(ctx, hipMemcpyAsync(extras->inliers_out, inliers.p, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (b < 0) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: every pose failed (non-finite transform)", who);
    *best_out = b;
    return GINGR_OK;
}

}  // namespace

extern "C" {

int gingr_rotation_samples(int64_t n, double *rotations9_out) {
    if (n < 1 || !rotations9_out) return GINGR_ERR_BAD_ARGUMENT;
    rs::rotation_samples(n, rotations9_out);
    return GINGR_OK;
}

int gingr_rigid_search(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S,
                       const double *rotations9, int32_t K, double overlap, int64_t *best_out, double *poses12_out, double *scores_out,
                       int64_t *kept_out, int32_t *failed_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!moving_xyz || !target_xyz || !rotations9 || !best_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_search: null argument");
    GINGR_TRY(check_search(ctx, "rigid_search", M, moving_xyz, N, target_xyz, S, K, overlap));
    if (!all_finite(rotations9, 9 * S)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "rigid_search: non-finite rotation");
    *best_out = -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // start poses: T_s(x) = R0_s (x - mean X) + mean Y
    double mx[3], c[3];
    mean3(moving_xyz, M, mx);
    mean3(target_xyz, N, c);
    std::vector<double> start((size_t)S * rs::kPoseWords);
    for (int64_t s = 0; s < S; ++s) {
        const double *R = rotations9 + 9 * s;
        double *T = start.data() + rs::kPoseWords * s;
        for (int k = 0; k < 9; ++k) T[k] = R[k];
        for (int a = 0; a < 3; ++a) T[9 + a] = c[a] - ((R[a * 3] * mx[0] + R[a * 3 + 1] * mx[1]) + R[a * 3 + 2] * mx[2]);
    }
    if (!all_finite(start.data(), (int64_t)start.size())) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "rigid_search: non-finite start pose");
    return run_search(ctx, "rigid_search", M, moving_xyz, N, target_xyz, S, start, std::vector<int32_t>((size_t)S, 0), c, K, overlap, nullptr,
                      best_out, poses12_out, scores_out, kept_out, failed_out);
}

int gingr_rigid_search_poses(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S,
                             const double *poses12_in, int32_t K, double overlap, double inlier_distance, int32_t select, int64_t *best_out,
                             double *poses12_out, double *scores_out, int64_t *kept_out, int32_t *failed_out, int64_t *inliers_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!moving_xyz || !target_xyz || !poses12_in || !best_out)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_search_poses: null argument");
    GINGR_TRY(check_search(ctx, "rigid_search_poses", M, moving_xyz, N, target_xyz, S, K, overlap));
    if (!(inlier_distance >= 0.0) || (select != 0 && select != 1))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_search_poses: inlier_distance = %g, select = %d: need a distance >= 0, select 0 or 1",
                               inlier_distance, (int)select);
    *best_out = -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double c[3];
    mean3(target_xyz, N, c);
    std::vector<double> start(poses12_in, poses12_in + (size_t)S * rs::kPoseWords);
    std::vector<int32_t> start_failed((size_t)S, 0);
    for (int64_t s = 0; s < S; ++s)  // a non-finite start pose (a degenerate triple's) takes no part
        start_failed[(size_t)s] = all_finite(poses12_in + rs::kPoseWords * s, rs::kPoseWords) ? 0 : 1;
    const SearchExtras extras{inlier_distance * inlier_distance, (int)select, inliers_out};
    return run_search(ctx, "rigid_search_poses", M, moving_xyz, N, target_xyz, S, start, start_failed, c, K, overlap, &extras, best_out,
                      poses12_out, scores_out, kept_out, failed_out);
}

}  // extern "C"
