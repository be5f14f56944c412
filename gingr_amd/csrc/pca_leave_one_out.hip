// Leave-one-out generalization of a PCA shape model on the device (C ABI in include/gingr_hip.h: gingr_pca_leave_one_out) -- what a
// scalismo user gets from Crossvalidation.leaveOneOutCrossvalidation with the generalization measure: for every shape i the PCA model
// of the other n - 1 shapes (gingr_model_from_shapes without alignment), shape i projected onto its k leading components
// (gingr_model_generalization), the mean and the largest vertex distance.  Nothing of mesh size is repeated per fold:
//   D      [3 M + 48][np]  the shapes centred on the mean of ALL n, as columns in the basis layout (rows in the caller's order)
//   G      = D^T D         the Gram pass of gp_gram.hip, once
//   fold i, a = 1 / (n - 1), J = the shapes but i:  the fold's mean is mean - a d_i, its centred shapes are d_j + a d_i, so
//            Gf[j][l] = (G[j][l] + a (G[j][i] + G[i][l]) + a^2 G[i][i]) / (n - 2)               (fold_gram_kernel)
//            Gf + shift I = V diag(lambda + shift) V^T, shift = trace Gf / (n - 1)               (sym_eig_strided: all folds side by side)
//            g[j] = (1 + a) (G[j][i] + a G[i][i]),  b = V^T g / sqrt(n - 2),  alpha_j = b_j / (lambda_j + 1e-5) for j < k' = min(k, fold rank)
//            c = V_k' alpha / sqrt(n - 2);  w_j = c_j (j != i),  w_i = a sum c - (1 + a)        (fold_factor_kernel)
//   error field of (rank, fold) = D w: project_measure_kernel (model_metrics.hip) with D as the basis and W = w + e_i as the factor --
//            that kernel subtracts column i of D in its epilogue -- on float64 MFMA, norm, sum and maximum per column, never stored.
// The shift is the mean eigenvalue of pca_model.hip: a centred Gram matrix is always singular.  A fold whose total variance lies within
// the rounding of its own Gram entries (the other shapes are all identical) has rank 0: c = 0, the projection is the fold's mean.
// Every sum is taken in a fixed order (per-thread ascending, trees of a fixed shape, no float atomics): two calls give the same bits.
#include "gp.h"
#include "model_metrics.h"
#include "pca_loo_plan.h"
#include "spectrum_plan.h"

#include <algorithm>
#include <cmath>

namespace lp = pca_loo_plan;

namespace {

constexpr int kFoldThreads = 512;  // one thread per row of a fold (n - 1 <= 511)
static_assert(lp::kMaxShapes <= kFoldThreads, "a fold's rows fit one workgroup");

struct LooRanks {
    int32_t n;
    int32_t k[lp::kMaxRanks];
};

// D[row][j] -= mean of the row over the n shapes, mean[row] = that mean.  Sixteen lanes per row (one 128-byte line per step), each
// ascending; the butterfly over the sixteen adds mirror images: the same bits in every lane.
__global__ __launch_bounds__(256) void center_rows_kernel(double *__restrict__ D, int64_t rows, int n, int np, double *__restrict__ mean) {
    const int c = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (row >= rows) return;  // (whole groups of sixteen lanes)
    double *d = D + row * np;
    double acc = 0.0;
    for (int j = c; j < n; j += 16) acc += d[j];
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 8);
    const double m = acc / (double)n;
    if (c == 0) mean[row] = m;
    for (int j = c; j < n; j += 16) d[j] -= m;
}

// the sum of the 512 entries of `red` in every thread: a tree of a fixed shape.  All kFoldThreads threads call it.
__device__ __forceinline__ double tree_sum(double *red, double v) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = kFoldThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

// out[0] = trace G, out[1] = |mean shape|^2; one workgroup
__global__ __launch_bounds__(kFoldThreads) void totals_kernel(const double *__restrict__ G, int np, int n, const double *__restrict__ mean, int64_t rows,
                                                              double *__restrict__ out) {
    __shared__ double red[kFoldThreads];
    const int t = threadIdx.x;
    double sq = 0.0;
    for (int64_t e = t; e < rows; e += kFoldThreads) sq = __builtin_fma(mean[e], mean[e], sq);
    const double trace = tree_sum(red, t < n ? G[(int64_t)t * np + t] : 0.0);
    const double mu_sq = tree_sum(red, sq);
    if (t == 0) out[0] = trace, out[1] = mu_sq;
}

// Workgroup f, fold i = fold0 + f: Gs [f][n - 1][n - 1] = Gf + shift I, g [f][n - 1], shift[f], rank0[f].  G is read at (min, max) of
// its indices: the fold matrix is symmetric to the bit.  A fold is of rank 0 when its trace is not above the rounding the sums that
// form it can carry -- cancel x the sum of the magnitudes of their terms -- plus noise_floor, the rounding of the mean shape
// (pca_model.hip); its matrix is written as the identity (nothing to decompose) and its right-hand side as zero.
__global__ __launch_bounds__(kFoldThreads) void fold_gram_kernel(const double *__restrict__ G, int np, int n, int fold0, double cancel, double noise_floor,
                                                                 double *__restrict__ Gs, double *__restrict__ g, double *__restrict__ shift,
                                                                 int32_t *__restrict__ rank0) {
    __shared__ double red[kFoldThreads];
    __shared__ double gi[kFoldThreads];  // G[j][i] by local row
    const int f = blockIdx.x, i = fold0 + f, t = threadIdx.x, nf = n - 1;
    const double a = 1.0 / (double)(n - 1), gii = G[(int64_t)i * np + i], div = (double)(n - 2);
    auto sym = [&](int j, int l) { return G[(int64_t)min(j, l) * np + max(j, l)]; };
    double diag = 0.0, mag = 0.0;
    if (t < nf) {
        const int j = lp::fold_shape(i, t);
        gi[t] = sym(j, i);
        const double gjj = sym(j, j);
        diag = (gjj + a * (gi[t] + gi[t]) + a * a * gii) / div;
        mag = (fabs(gjj) + a * (fabs(gi[t]) + fabs(gi[t])) + a * a * fabs(gii)) / div;
    }
    const double trace = tree_sum(red, diag);
    const double bound = tree_sum(red, mag);
    const bool none = !(trace > cancel * bound + noise_floor / div);
    const double sh = none ? 0.0 : trace / (double)nf;
    if (t == 0) shift[f] = sh, rank0[f] = none ? 1 : 0;
    if (t < nf) g[(int64_t)f * nf + t] = none ? 0.0 : (1.0 + a) * (gi[t] + a * gii);
    double *out = Gs + (int64_t)f * nf * nf;
    for (int e = t; e < nf * nf; e += kFoldThreads) {
        const int r = e / nf, c = e - r * nf;
        const double v = (sym(lp::fold_shape(i, r), lp::fold_shape(i, c)) + a * (gi[r] + gi[c]) + a * a * gii) / div;
        out[e] = none ? (r == c ? 1.0 : 0.0) : v + (r == c ? sh : 0.0);
    }
}

// Workgroup f, fold i = fold0 + f, thread = local row / component.  lambda_j = max(evals_j - shift, 0); fold rank = the leading
// components with lambda_j > relative_tolerance lambda_0 and > 0, at most n - 2 (both: spectrum_plan.h); b, alpha and, per rank q with k' = min(k(q), fold rank),
// c as one running sum over the components that is written out whenever it reaches the next k'.  W[shape][q np + i] = w + e_i (the
// measure pass subtracts column i of D): c_r at the shapes that stay, a sum c - a at shape i.  flag: set on a non-finite eigenvalue.
__global__ __launch_bounds__(kFoldThreads) void fold_factor_kernel(const double *__restrict__ evals, const double *__restrict__ V, const double *__restrict__ g,
                                                                   const double *__restrict__ shift, const int32_t *__restrict__ rank0, int n, int np,
                                                                   int fold0, double relative_tolerance, LooRanks ranks, double *__restrict__ W, int64_t ldw,
                                                                   int32_t *__restrict__ fold_rank, int32_t *__restrict__ flag) {
    __shared__ double red[kFoldThreads];
    __shared__ double lam[kFoldThreads], alpha[kFoldThreads], gs[kFoldThreads];
    __shared__ int rank_s;
    const int f = blockIdx.x, i = fold0 + f, t = threadIdx.x, nf = n - 1;
    const double a = 1.0 / (double)(n - 1), root = sqrt((double)(n - 2));
    const double *Vf = V + (int64_t)f * nf * nf;
    const bool none = rank0[f] != 0;
    if (t < nf) {
        const double ev = evals[(int64_t)f * nf + t];
        if (!(fabs(ev) <= kDblMax)) atomicOr(flag, 1);
        lam[t] = none ? 0.0 : spectrum_plan::unshift(ev, shift[f]);
        gs[t] = g[(int64_t)f * nf + t];
    }
    __syncthreads();
    if (t == 0) {
        const int k = spectrum_plan::leading_rank(lam, n - 2, relative_tolerance);
        rank_s = k;
        fold_rank[i] = k;
    }
    __syncthreads();
    const int rank = rank_s;
    if (t < rank) {
        double b = 0.0;
        for (int r = 0; r < nf; ++r) b = __builtin_fma(Vf[(int64_t)r * nf + t], gs[r], b);
        alpha[t] = (b / root) / (lam[t] + GINGR_COEFF_NOISE);
    }
    __syncthreads();
    double acc = 0.0;
    int j = 0;
    for (int q = 0; q < ranks.n; ++q) {
        const int k = min(ranks.k[q], rank);
        if (t < nf)
            for (; j < k; ++j) acc = __builtin_fma(Vf[(int64_t)t * nf + j], alpha[j], acc);
        const double c = t < nf ? acc / root : 0.0;
        const double sum = tree_sum(red, c);
        double *col = W + (int64_t)q * np + i;
        if (t < nf) col[lp::fold_shape(i, t) * ldw] = c;
        if (t == 0) col[i * ldw] = a * sum - a;
    }
}

}  // namespace

extern "C" {

int gingr_pca_leave_one_out(gingr_ctx *ctx, int64_t M, int32_t n_shapes, const double *shapes_xyz, double relative_tolerance, int32_t n_ranks,
                            const int32_t *ranks, double *avg, double *max_out, int32_t *fold_rank) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "pca_leave_one_out";
    if (!shapes_xyz || !avg || !max_out || !fold_rank || (n_ranks > 0 && !ranks))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (n_shapes < lp::kMinShapes || n_shapes > lp::kMaxShapes)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d shapes, need %d <= n_shapes <= %d", who, (int)n_shapes, (int)lp::kMinShapes,
                               (int)lp::kMaxShapes);
    if (M < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld < 1", who, (long long)M);
    if (M > (int64_t)0x7fffffff / 3) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld too large", who, (long long)M);
    if (!(relative_tolerance >= 0.0 && relative_tolerance < 1.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: relative_tolerance %g outside [0, 1)", who, relative_tolerance);
    const int n = n_shapes, nf = n - 1;
    LooRanks rl{};
    {
        int at = 0;
        switch (lp::check_ranks(n, n_ranks, ranks, &at)) {
            case 0: break;
            case 1: return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d ranks, need 1 <= n_ranks <= %d", who, (int)n_ranks, (int)lp::kMaxRanks);
            case 2:
                return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: ranks[%d] = %d outside 1..%d (n_shapes - 2)", who, at, (int)ranks[at], n - 2);
            default:
                return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: ranks must be strictly increasing (ranks[%d] = %d after %d)", who, at,
                                       (int)ranks[at], (int)ranks[at - 1]);
        }
        rl.n = n_ranks;
        for (int q = 0; q < n_ranks; ++q) rl.k[q] = ranks[q];
    }
    GINGR_TRY(check_finite(ctx, shapes_xyz, 3 * M, n, who, "shape"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int np = (int)lp::padded_shapes(n), ldt = (int)lp::weight_columns(n, n_ranks);
    const int64_t rows = 3 * M;

    // ---- 1. D and G = D^T D
    DevBuf D, mean, gws, G, totals;
    GINGR_TRY(pack_shape_columns(ctx, M, nullptr, nullptr, nullptr, n, shapes_xyz, false, D, np));
    HIP_TRY(ctx, mean.alloc((size_t)rows * sizeof(double)));
    HIP_TRY(ctx, gws.alloc((size_t)gram_ws_doubles(M, np) * sizeof(double)));
    HIP_TRY(ctx, G.alloc((size_t)np * np * sizeof(double)));
    HIP_TRY(ctx, totals.alloc(2 * sizeof(double)));
    hipLaunchKernelGGL(center_rows_kernel, dim3((unsigned)ceil_div(rows, 16)), dim3(256), 0, ctx->stream, D.as<double>(), rows, n, np, mean.as<double>());
    launch_gram(ctx, D.as<double>(), M, np, nullptr, gws.as<double>(), G.as<double>());
    hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(kFoldThreads), 0, ctx->stream, G.as<double>(), np, n, mean.as<double>(), rows, totals.as<double>());
    GINGR_TRY(check_launch(ctx));
    double h[2] = {0.0, 0.0};
    HIP_TRY(ctx, hipMemcpyAsync(h, totals.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    gws.release();
    mean.release();
    if (!std::isfinite(h[0])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Gram matrix of the centred shapes", who);
    // identical shapes leave the rounding of the mean behind (pca_model.hip): a total variance within that bound is no variance
    const double eps = 2.220446049250313e-16;
    const double noise_floor = (64.0 + (double)n * n) * eps * eps * h[1];
    if (!(h[0] > noise_floor)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: all shapes are identical", who);
    // an entry of G is a sum of 3 M products, an entry of a fold's matrix a sum of four such terms
    const double cancel = (3.0 * (double)M + 64.0) * eps;

    // ---- 2. the folds, a batch at a time: fold matrices, their decompositions, the weight columns
    DevBuf Gs, V, evals, g, shift, rank0, W, franks, flag;
    const lp::FoldBatches batches = lp::fold_batches(n, nf <= kSymEigColsMaxN ? sym_eig_cols_work_doubles(nf) : 0);
    const size_t per = (size_t)batches.per_batch;
    HIP_TRY(ctx, Gs.alloc(per * nf * nf * sizeof(double)));
    HIP_TRY(ctx, V.alloc(per * nf * nf * sizeof(double)));
    HIP_TRY(ctx, evals.alloc(per * nf * sizeof(double)));
    HIP_TRY(ctx, g.alloc(per * nf * sizeof(double)));
    HIP_TRY(ctx, shift.alloc(per * sizeof(double)));
    HIP_TRY(ctx, rank0.alloc(per * sizeof(int32_t)));
    HIP_TRY(ctx, W.alloc((size_t)np * ldt * sizeof(double)));
    HIP_TRY(ctx, franks.alloc((size_t)n * sizeof(int32_t)));
    HIP_TRY(ctx, flag.alloc(sizeof(int32_t)));
    HIP_TRY(ctx, hipMemsetAsync(W.p, 0, (size_t)np * ldt * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(flag.p, 0, sizeof(int32_t), ctx->stream));
    for (int64_t b = 0; b < batches.count; ++b) {
        const int fold0 = (int)batches.begin(b), cnt = (int)batches.length(b);
        hipLaunchKernelGGL(fold_gram_kernel, dim3((unsigned)cnt), dim3(kFoldThreads), 0, ctx->stream, G.as<double>(), np, n, fold0, cancel, noise_floor,
                           Gs.as<double>(), g.as<double>(), shift.as<double>(), rank0.as<int32_t>());
        GINGR_TRY(check_launch(ctx));
        GINGR_TRY(sym_eig_strided(ctx, cnt, Gs.as<double>(), nf, evals.as<double>(), V.as<double>()));
        hipLaunchKernelGGL(fold_factor_kernel, dim3((unsigned)cnt), dim3(kFoldThreads), 0, ctx->stream, evals.as<double>(), V.as<double>(), g.as<double>(),
                           shift.as<double>(), rank0.as<int32_t>(), n, np, fold0, relative_tolerance, rl, W.as<double>(), (int64_t)ldt,
                           franks.as<int32_t>(), flag.as<int32_t>());
        GINGR_TRY(check_launch(ctx));
    }
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite eigenvalue", who);
    Gs.release();
    V.release();

    // ---- 3. D W measured: one column per (rank, fold)
    DevBuf partial, res;
    HIP_TRY(ctx, res.alloc((size_t)2 * n_ranks * n * sizeof(double)));
    GINGR_TRY(launch_project_measure(ctx, D.as<double>(), M, np, W.as<double>(), ldt, D.as<double>(), np, n, (int)n_ranks, partial, res.as<double>()));
    HIP_TRY(ctx, hipMemcpyAsync(avg, res.p, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(max_out, res.as<double>() + (size_t)n_ranks * n, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fold_rank, franks.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

}  // extern "C"
