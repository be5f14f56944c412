// Classic Coherent Point Drift (the reference's `other/` family, Myronenko & Song 2010) on the device: a second consumer of the
// streaming affinity statistics (cpd_pairs.hip) and of the Gaussian kernel block.
//
//   CPDFactory(templatePoints, lambda, beta, w)         G/other/algorithms/cpd/CPDFactory.scala:28-80   (G = exp(-|a-b|^2 / 2 beta^2))
//   RigidCPD.Expectation / Maximization / Registration  G/other/algorithms/cpd/RigidCPD.scala:59-139
//   AffineCPD.Maximization                              G/other/algorithms/cpd/AffineCPD.scala:35-61
//   NonRigidCPD.Maximization                            G/other/algorithms/cpd/NonRigidCPD.scala:45-88
//
// Expectation never forms the M x N matrix P: the Maximizations only need P1 = P 1, Pt1 = P^T 1, P X and Np, which the two
// streaming passes of the GiNGR path already produce.  Rigid / affine: two O(M + N) reductions (weighted means, then the centred
// 3x3 moments) and one thread of 3x3 algebra.  Non-rigid: the M x M system (G + lambda sigma2 diag(1/P1)) W = diag(1/P1) P X - Y is
// symmetric positive definite (the reference solves it with LU, `A \ B`); it is factored here by a blocked right-looking Cholesky
// with 64-wide panels (dense_spd.hip: diagonal block in LDS, panel and trailing update as 64 x 64 MFMA tiles, v_mfma_f64_16x16x4,
// over the whole chip) with the three right-hand sides riding along as extra rows of the matrix (the forward
// substitution is a by-product), a blocked backward substitution, and TY = Y + G W as one pass over G.  Past dense sizes the non-rigid
// Maximization runs over a low-rank factor of G (classic_cpd_lowrank.hip).  The reductions and the row products are cloud_sums.h's.
#include "common.h"
#include "cloud_sums.h"
#include "classic_cpd_lowrank.h"
#include "dense_spd.h"
#include "kernel_warp.h"
#include "svd3.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int kNBc = DenseSpdWork::kBlock;  // Cholesky panel width
constexpr int kRedBlocks = 64;  // workgroups of the O(M + N) reductions

Cloud cloud_at(const double *soa, int64_t n) { return Cloud{soa, soa + n, soa + 2 * n, n}; }

// partial[b][0..2] = sum_j Pt1_j x_j, [3..5] = sum_i P1_i y_i
__global__ __launch_bounds__(256) void means_kernel(Cloud X, const double *__restrict__ Pt1, Cloud Y, const double *__restrict__ P1,
                                                    double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < X.n; j += (int64_t)kRedBlocks * 256) {
        const double p = Pt1[j];
        a[0] += p * X.x[j];
        a[1] += p * X.y[j];
        a[2] += p * X.z[j];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < Y.n; i += (int64_t)kRedBlocks * 256) {
        const double p = P1[i];
        a[3] += p * Y.x[i];
        a[4] += p * Y.y[i];
        a[5] += p * Y.z[i];
    }
    block_sums<6>(a, sh, partial + blockIdx.x * 6);
}

// mu[0..2] = muX, mu[3..5] = muY   (RigidCPD.scala:117-118)
__global__ void means_finish_kernel(const double *__restrict__ partial, const double *__restrict__ scalars, double *__restrict__ mu) {
    if (threadIdx.x >= 6) return;
    mu[threadIdx.x] = sum_partials(partial, kRedBlocks, 6, threadIdx.x) / scalars[0];
}

// partial[b][0..8] = A = Xhat^T P^T Yhat (row-major; from P X: sum_i (PX_i - P1_i muX)(y_i - muY)^T), [9..17] = Yhat^T diag(P1) Yhat,
// [18] = trace(Xhat^T diag(Pt1) Xhat)
__global__ __launch_bounds__(256) void moments_kernel(Cloud X, const double *__restrict__ Pt1, Cloud Y, const double *__restrict__ P1,
                                                      const double *__restrict__ PX, const double *__restrict__ mu,
                                                      double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[19];
    for (int q = 0; q < 19; ++q) a[q] = 0.0;
    const double mx[3] = {mu[0], mu[1], mu[2]}, my[3] = {mu[3], mu[4], mu[5]};
    const int64_t M = Y.n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)kRedBlocks * 256) {
        const double p = P1[i];
        const double u[3] = {PX[i] - p * mx[0], PX[M + i] - p * mx[1], PX[2 * M + i] - p * mx[2]};
        const double yh[3] = {Y.x[i] - my[0], Y.y[i] - my[1], Y.z[i] - my[2]};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                a[r * 3 + c] += u[r] * yh[c];
                a[9 + r * 3 + c] += p * yh[r] * yh[c];
            }
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < X.n; j += (int64_t)kRedBlocks * 256) {
        const double dx = X.x[j] - mx[0], dy = X.y[j] - mx[1], dz = X.z[j] - mx[2];
        a[18] += Pt1[j] * ((dx * dx + dy * dy) + dz * dz);
    }
    block_sums<19>(a, sh, partial + blockIdx.x * 19);
}

// params[0] = s (affine: 1), [1..9] = R or B (row-major), [10..12] = t; scalars[8] = the new sigma2
__global__ void transform_finish_kernel(const double *__restrict__ partial, const double *__restrict__ mu, double *__restrict__ scalars,
                                        int affine, double *__restrict__ params, int32_t *__restrict__ flag) {
    if (threadIdx.x != 0) return;
    double m[19];
    for (int q = 0; q < 19; ++q) m[q] = sum_partials(partial, kRedBlocks, 19, q);
    const double *A = m, *YPY = m + 9, s1 = m[18], Np = scalars[0];
    double L[9], sc = 1.0, s2;
    if (!affine) {
        // svd(A) = U S V^T; C = diag(1, 1, det(U V^T)); R = U C V^T; s = tr(A^T R) / tr(Yhat^T P1 Yhat)     (RigidCPD.scala:124-131)
        double U[9], S[3], V[9], UVt[9];
        svd3(A, U, S, V);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) UVt[r * 3 + c] = U[r * 3] * V[c * 3] + U[r * 3 + 1] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2];
        const double d = det3(UVt);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) L[r * 3 + c] = U[r * 3] * V[c * 3] + U[r * 3 + 1] * V[c * 3 + 1] + d * U[r * 3 + 2] * V[c * 3 + 2];
        double trAR = 0.0;
        for (int q = 0; q < 9; ++q) trAR += A[q] * L[q];
        sc = trAR / (YPY[0] + YPY[4] + YPY[8]);
        s2 = sc * trAR;
    } else {
        // B = Xhat^T P^T Yhat (Yhat^T P1 Yhat)^-1; s2 = tr(Xhat^T P^T Yhat B^T)                              (AffineCPD.scala:51-56)
        double inv[9];
        spd3_inverse(YPY, inv);  // Yhat^T diag(P1) Yhat is symmetric positive definite unless the template is planar: NaNs then, flagged below
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) L[r * 3 + c] = A[r * 3] * inv[c] + A[r * 3 + 1] * inv[3 + c] + A[r * 3 + 2] * inv[6 + c];
        s2 = 0.0;
        for (int q = 0; q < 9; ++q) s2 += A[q] * L[q];
    }
    params[0] = sc;
    bool fin = true;
    for (int q = 0; q < 9; ++q) {
        params[1 + q] = L[q];
        fin = fin && finite_d(L[q]);
    }
    for (int r = 0; r < 3; ++r) params[10 + r] = mu[r] - sc * (L[r * 3] * mu[3] + L[r * 3 + 1] * mu[4] + L[r * 3 + 2] * mu[5]);
    const double ns = (s1 - s2) / (Np * 3.0);
    scalars[8] = ns;
    if (!fin || !finite_d(ns)) *flag = GINGR_ERR_NONFINITE;
}

// TY = s Y R^T + 1 t^T  (in place)
__global__ void apply_transform_kernel(int64_t M, double *__restrict__ ty, const double *__restrict__ params) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double p[3];
    similarity_apply(params, ty[i], ty[M + i], ty[2 * M + i], p);
    for (int d = 0; d < 3; ++d) ty[d * M + i] = p[d];
}

// ------------------------------------------------------------------------------------------------ non-rigid: the M x M system
// Aw: (Mp + 64) x Mp row-major (ld = Mp, Mp = M rounded up to 64).  Rows < M: lower triangle of G + lambda sigma2 diag(1/P1); rows
// M..Mp-1: identity (padding); rows Mp + d, d < 3: B[:, d]^T with B = diag(1/P1) P X - Y; the other border rows are zero.
__global__ void build_system_kernel(int64_t M, int64_t Mp, const double *__restrict__ G, const double *__restrict__ P1,
                                    const double *__restrict__ PX, const double *__restrict__ Y, const double *__restrict__ scalars,
                                    double lambda, double *__restrict__ Aw) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (c >= Mp) return;
    double v = 0.0;
    if (r < M) {
        if (c <= r) v = G[r * M + c];
        if (c == r) v += lambda * scalars[8] * (1.0 / P1[r]);
    } else if (r < Mp) {
        v = c == r ? 1.0 : 0.0;
    } else if (r < Mp + 3 && c < M) {
        const int64_t d = r - Mp;
        v = PX[d * M + c] * (1.0 / P1[c]) - Y[d * M + c];
    }
    Aw[r * Mp + c] = v;
}

// TY = Y + G W: 16 lanes per row of G
__global__ __launch_bounds__(256) void deform_kernel(int64_t M, int64_t Mp, const double *__restrict__ G, const double *__restrict__ W,
                                                     double *__restrict__ ty) {
    const int lane16 = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    double a[3];
    row_dot3(G + i * M, 0, i < M ? M : 0, lane16, W, Mp, nullptr, a);
    if (i < M && lane16 == 0) {
        ty[i] += a[0];
        ty[M + i] += a[1];
        ty[2 * M + i] += a[2];
    }
}

// partial[b][0] = sum_i P1_i |TY_i|^2, [1] = sum_i TY_i . PX_i      (NonRigidCPD.scala:74-77)
__global__ __launch_bounds__(256) void nonrigid_sums_kernel(int64_t M, const double *__restrict__ ty, const double *__restrict__ P1,
                                                            const double *__restrict__ PX, double *__restrict__ partial) {
    __shared__ double sh[256];
    double a[2] = {0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)kRedBlocks * 256) {
        const double x = ty[i], y = ty[M + i], z = ty[2 * M + i];
        a[0] += P1[i] * ((x * x + y * y) + z * z);
        a[1] += (x * PX[i] + y * PX[M + i]) + z * PX[2 * M + i];
    }
    block_sums<2>(a, sh, partial + blockIdx.x * 2);
}

__global__ void nonrigid_finish_kernel(const double *__restrict__ partial, double *__restrict__ scalars, int32_t *__restrict__ flag) {
    if (threadIdx.x != 0) return;
    const double ypy = sum_partials(partial, kRedBlocks, 2, 0), tr = sum_partials(partial, kRedBlocks, 2, 1);
    const double ns = (scalars[1] - 2 * tr + ypy) / (scalars[0] * 3.0);
    scalars[8] = ns;
    if (!finite_d(ns)) *flag = GINGR_ERR_NONFINITE;
}

}  // namespace

struct gingr_classic_cpd {
    gingr_ctx *ctx = nullptr;
    int32_t kind = 0;
    int64_t M = 0, N = 0, Mp = 0;
    double lambda = 2.0, beta = 2.0, w = 0.0;
    DevBuf X, TY, den, inv_den, Pt1, P1, PX, ws, part, sc, aux, red, mu, params, flag, G, Aw, Linv, W, stage;
    std::unique_ptr<LowRankCpd> lowrank;  // gingr_classic_cpd_create_lowrank: G, Aw and Linv stay empty
    // the kernel warp (gingr_classic_cpd_transform_points): the map belongs to the last successful iteration; Y0 (non-rigid kind): the
    // template as it was given, the centres of the Gaussian -- TY moves
    bool map_valid = false;
    DevBuf Y0;
    KernelWarpWork warp;
};

static_assert(GINGR_CLASSIC_CPD_MAX_COLUMNS == lowrank_plan::kMaxColumns, "the header's ceiling is the plan's");

// what gingr_classic_cpd_create_lowrank adds to the arguments of gingr_classic_cpd_create
struct LowRankRequest {
    double relative_tolerance;
    int32_t max_columns;
    gingr_classic_cpd_lowrank_info *info;
};

extern "C" {

void gingr_classic_cpd_destroy(gingr_classic_cpd *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    delete h;
}

static int classic_cpd_create_impl(gingr_ctx *ctx, int32_t kind, int64_t M, const double *template_xyz, int64_t N,
                                   const double *target_xyz, double lambda, double beta, double w, const LowRankRequest *lowrank,
                                   gingr_classic_cpd **out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!out || !template_xyz || !target_xyz || M < 1 || N < 1 || kind < 0 || kind > 2)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_create: bad argument");
    // CPDFactory's requirements (CPDFactory.scala:43-45); w = 1 divides by zero in the outlier constant
    if (!(w >= 0.0 && w < 1.0) || !(beta > 0.0) || !(lambda > 0.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_create: need 0 <= w < 1, beta > 0, lambda > 0");
    if (kind == 2 && !lowrank && M > 46000) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_create: non-rigid template too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gingr_classic_cpd *h = new gingr_classic_cpd;
    h->ctx = ctx;
    h->kind = kind;
    h->M = M;
    h->N = N;
    h->Mp = round_up(M, kNBc);
    h->lambda = lambda;
    h->beta = beta;
    h->w = w;
    auto fail = [&](int rc) {
        gingr_classic_cpd_destroy(h);
        return rc;
    };
    const int64_t big = M > N ? M : N;
    HANDLE_TRY(ctx, fail, h->X.alloc((size_t)3 * N * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->TY.alloc((size_t)3 * M * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->stage.alloc((size_t)3 * big * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->den.alloc((size_t)N * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->inv_den.alloc((size_t)N * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->Pt1.alloc((size_t)N * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->P1.alloc((size_t)M * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->PX.alloc((size_t)3 * M * sizeof(double)));
    const int64_t ws1 = cpd_colsum_ws_doubles(M, N), ws2 = cpd_rowstats_ws_doubles(M, N);
    HANDLE_TRY(ctx, fail, h->ws.alloc((size_t)std::max(std::max(ws1, ws2), sumsq_pairs_ws_doubles(M)) * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->part.alloc(GINGR_SCALAR_PART * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->sc.alloc(16 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->aux.alloc(GINGR_AUX * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->red.alloc((size_t)kRedBlocks * 19 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->mu.alloc(6 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->params.alloc(16 * sizeof(double)));
    HANDLE_TRY(ctx, fail, h->flag.alloc(sizeof(int32_t)));
    HANDLE_TRY(ctx, fail, hipMemsetAsync(h->sc.p, 0, 16 * sizeof(double), ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemsetAsync(h->params.p, 0, 16 * sizeof(double), ctx->stream));
    HANDLE_TRY(ctx, fail, hipMemsetAsync(h->flag.p, 0, sizeof(int32_t), ctx->stream));
    if (int rc = upload_cloud(ctx, h->stage.as<double>(), target_xyz, N, h->X.as<double>())) return fail(rc);
    if (int rc = upload_cloud(ctx, h->stage.as<double>(), template_xyz, M, h->TY.as<double>())) return fail(rc);
    if (kind == 2) {
        HANDLE_TRY(ctx, fail, h->Y0.alloc((size_t)3 * M * sizeof(double)));
        HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->Y0.p, h->TY.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    const Cloud X = cloud_at(h->X.as<double>(), N), Y = cloud_at(h->TY.as<double>(), M);
    double *aux = h->aux.as<double>();
    launch_cloud_centroid(ctx, X, aux + 2);
    launch_cloud_absmax(ctx, X, aux + 2, aux);
    // sigma2_0 = sum |y_m - x_n|^2 / (dim N M)                                    (RigidCPD.initializeGaussianKernel, :46-57)
    double s0 = 0.0;
    if (int rc = first_variance(ctx, Y, X, 1.0, h->ws.as<double>(), h->sc.as<double>() + 9, &s0)) return fail(rc);
    HANDLE_TRY(ctx, fail, hipMemcpyAsync(h->sc.as<double>() + 8, &s0, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (lowrank) {
        h->lowrank.reset(new LowRankCpd);
        HANDLE_TRY(ctx, fail, h->W.alloc((size_t)3 * h->Mp * sizeof(double)));
        HANDLE_TRY(ctx, fail, hipMemsetAsync(h->W.p, 0, (size_t)3 * h->Mp * sizeof(double), ctx->stream));
        const int rc = lowrank_cpd_build(ctx, Y, beta, lowrank->relative_tolerance, lowrank->max_columns, *h->lowrank);
        if (rc != GINGR_OK) {
            (void)hipGetLastError();  // (a refused allocation must not surface again in the next call's launch check)
            return fail(rc);
        }
        if (lowrank->info) {
            const LowRankCpd &lr = *h->lowrank;
            *lowrank->info = gingr_classic_cpd_lowrank_info{lr.plan.k, lr.tolerance_reached, lr.residual_fraction, (int64_t)lr.L.bytes};
        }
    } else if (kind == 2) {
        const int64_t Mp = h->Mp;
        const DenseSpdWork sys(Mp, DenseSpdWork::kRhsRows);
        HANDLE_TRY(ctx, fail, h->G.alloc((size_t)M * M * sizeof(double)));
        HANDLE_TRY(ctx, fail, h->Aw.alloc((size_t)sys.aw_doubles() * sizeof(double)));
        HANDLE_TRY(ctx, fail, h->Linv.alloc((size_t)sys.linv_doubles() * sizeof(double)));
        HANDLE_TRY(ctx, fail, h->W.alloc((size_t)sys.w_doubles() * sizeof(double)));
        // G = exp(-|y_i - y_j|^2 / (2 beta^2)) over the TEMPLATE points                    (CPDFactory.initializeKernelMatrixG, :54-66)
        launch_gauss_block(ctx, Y, Y, sqrt(2.0) * beta, 1.0, h->G.as<double>());
    }
    HANDLE_TRY(ctx, fail, hipGetLastError());
    HANDLE_TRY(ctx, fail, hipStreamSynchronize(ctx->stream));
    *out = h;
    return GINGR_OK;
}

int gingr_classic_cpd_create(gingr_ctx *ctx, int32_t kind, int64_t M, const double *template_xyz, int64_t N, const double *target_xyz,
                             double lambda, double beta, double w, gingr_classic_cpd **out) {
    return classic_cpd_create_impl(ctx, kind, M, template_xyz, N, target_xyz, lambda, beta, w, nullptr, out);
}

int gingr_classic_cpd_create_lowrank(gingr_ctx *ctx, int64_t M, const double *template_xyz, int64_t N, const double *target_xyz,
                                     double lambda, double beta, double w, double relative_tolerance, int32_t max_columns,
                                     gingr_classic_cpd_lowrank_info *info, gingr_classic_cpd **out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (info) memset(info, 0, sizeof(*info));
    if (!(relative_tolerance >= 0.0) || !(relative_tolerance < 1.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_create_lowrank: relative tolerance must be in [0, 1)");
    if (max_columns > GINGR_CLASSIC_CPD_MAX_COLUMNS)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_create_lowrank: max_columns = %d is above the ceiling of %d factor columns",
                               (int)max_columns, GINGR_CLASSIC_CPD_MAX_COLUMNS);
    const LowRankRequest req{relative_tolerance, max_columns, info};
    return classic_cpd_create_impl(ctx, 2, M, template_xyz, N, target_xyz, lambda, beta, w, &req, out);
}

int gingr_classic_cpd_get_factor(gingr_classic_cpd *h, int32_t *columns, double *L_rowmajor_M_by_k) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (!h->lowrank) return gingr_set_error(ctx, GINGR_ERR_STATE, "classic_cpd_get_factor: the handle holds the dense kernel matrix, not a factor");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (columns) *columns = h->lowrank->plan.k;
    if (L_rowmajor_M_by_k) return lowrank_cpd_get_factor(ctx, *h->lowrank, L_rowmajor_M_by_k);
    return GINGR_OK;
}

int gingr_classic_cpd_iterate(gingr_classic_cpd *h, int32_t n_iterations) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (n_iterations < 0) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_iterate: negative count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = h->M, N = h->N, Mp = h->Mp;
    const Cloud X = cloud_at(h->X.as<double>(), N), Y = cloud_at(h->TY.as<double>(), M);
    double *sc = h->sc.as<double>(), *s2 = sc + 8, *aux = h->aux.as<double>(), *ty = h->TY.as<double>();
    int32_t *flag = h->flag.as<int32_t>();
    if (n_iterations > 0) h->map_valid = false;
    for (int32_t it = 0; it < n_iterations; ++it) {
        // Expectation (RigidCPD.scala:90-105) as streaming statistics: P1, Pt1, P X, Np, xPx
        launch_cloud_absmax(ctx, Y, aux + 2, aux + 1);
        launch_cpd_colsum(ctx, Y, X, s2, aux, nullptr, h->ws.as<double>(), h->den.as<double>());
        launch_cpd_den_finalize(ctx, X, s2, h->w, M, h->den.as<double>(), h->inv_den.as<double>(), h->Pt1.as<double>(), nullptr,
                                h->part.as<double>(), sc);
        launch_cpd_rowstats(ctx, Y, X, s2, aux, h->inv_den.as<double>(), nullptr, nullptr, h->ws.as<double>(), h->P1.as<double>(),
                            h->PX.as<double>(), h->part.as<double>(), sc);
        if (h->lowrank) {
            lowrank_cpd_mstep(ctx, *h->lowrank, h->P1.as<double>(), h->PX.as<double>(), ty, sc, h->lambda, h->W.as<double>(), Mp, flag);
        } else if (h->kind != 2) {
            hipLaunchKernelGGL(means_kernel, dim3(kRedBlocks), dim3(256), 0, ctx->stream, X, h->Pt1.as<double>(), Y, h->P1.as<double>(),
                               h->red.as<double>());
            hipLaunchKernelGGL(means_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, h->red.as<double>(), sc, h->mu.as<double>());
            hipLaunchKernelGGL(moments_kernel, dim3(kRedBlocks), dim3(256), 0, ctx->stream, X, h->Pt1.as<double>(), Y, h->P1.as<double>(),
                               h->PX.as<double>(), h->mu.as<double>(), h->red.as<double>());
            hipLaunchKernelGGL(transform_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, h->red.as<double>(), h->mu.as<double>(), sc,
                               h->kind == 1 ? 1 : 0, h->params.as<double>(), flag);
            hipLaunchKernelGGL(apply_transform_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, ty,
                               h->params.as<double>());
        } else {
            double *Aw = h->Aw.as<double>(), *Linv = h->Linv.as<double>();
            hipLaunchKernelGGL(build_system_kernel, dim3((unsigned)ceil_div(Mp, 256), (unsigned)(Mp + kNBc)), dim3(256), 0, ctx->stream, M, Mp,
                               h->G.as<double>(), h->P1.as<double>(), h->PX.as<double>(), ty, sc, h->lambda, Aw);
            dense_spd_solve3(ctx, Aw, Mp, Linv, h->W.as<double>(), flag);
            hipLaunchKernelGGL(deform_kernel, dim3((unsigned)ceil_div(M, 16)), dim3(256), 0, ctx->stream, M, Mp, h->G.as<double>(),
                               h->W.as<double>(), ty);
            hipLaunchKernelGGL(nonrigid_sums_kernel, dim3(kRedBlocks), dim3(256), 0, ctx->stream, M, ty, h->P1.as<double>(),
                               h->PX.as<double>(), h->red.as<double>());
            hipLaunchKernelGGL(nonrigid_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, h->red.as<double>(), sc, flag);
        }
    }
    const int rc = finish_iterate(ctx, flag, 1, 0, "classic_cpd_iterate");
    if (rc == GINGR_OK && n_iterations > 0) h->map_valid = true;
    return rc;
}

int gingr_classic_cpd_transform_points(gingr_classic_cpd *h, int64_t P, const double *points_xyz, double *out_xyz) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    if (P < 0 || (P > 0 && (!points_xyz || !out_xyz)))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "classic_cpd_transform_points: bad argument");
    if (P == 0) return GINGR_OK;  // (whatever the state: nothing is asked for)
    if (!h->map_valid)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "classic_cpd_transform_points: no successful iteration since the state was created or set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (h->kind != 2)  // T(z) = s B z + t
        return kernel_warp_points(ctx, h->warp, Cloud{nullptr, nullptr, nullptr, 0}, nullptr, 0, h->beta, h->params.as<double>(), true, P,
                                  points_xyz, out_xyz);
    // T(z) = z + sum_m g(z, y_m) W_m
    return kernel_warp_points(ctx, h->warp, cloud_at(h->Y0.as<double>(), h->M), h->W.as<double>(), h->Mp, h->beta, nullptr, false, P, points_xyz,
                              out_xyz);
}

int gingr_classic_cpd_get(gingr_classic_cpd *h, double *ty_xyz, double *sigma2, double *transform13, double *w_xyz) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = h->M, Mp = h->Mp;
    if (ty_xyz) GINGR_TRY(download_cloud(ctx, h->stage.as<double>(), h->TY.as<double>(), M, ty_xyz));
    if (sigma2) HIP_TRY(ctx, hipMemcpyAsync(sigma2, h->sc.as<double>() + 8, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (transform13) HIP_TRY(ctx, hipMemcpyAsync(transform13, h->params.p, 13 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (w_xyz) {
        if (h->kind != 2) return gingr_set_error(ctx, GINGR_ERR_STATE, "classic_cpd_get: W exists for the non-rigid kind only");
        std::vector<double> hw((size_t)3 * Mp);
        HIP_TRY(ctx, hipMemcpyAsync(hw.data(), h->W.p, hw.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < M; ++i)
            for (int d = 0; d < 3; ++d) w_xyz[3 * i + d] = hw[(size_t)d * Mp + i];
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_classic_cpd_set(gingr_classic_cpd *h, const double *ty_xyz, double sigma2) {
    if (!h) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = h->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    h->map_valid = false;
    if (ty_xyz) GINGR_TRY(upload_cloud(ctx, h->stage.as<double>(), ty_xyz, h->M, h->TY.as<double>()));
    HIP_TRY(ctx, hipMemcpyAsync(h->sc.as<double>() + 8, &sigma2, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}


}  // extern "C"
