// The posterior of a low-rank model as a model of its own (C ABI in include/gingr_hip.h): model.transform(rigid).posterior(obs) of
// scalismo (DiscreteLowRankGaussianProcess.regression; G/api/GingrAlgorithm.scala:281-302) with the basis staying on the device.
//   W = L^-T, L L^T = I + G        (launch_posterior_factor; G, rhs: Gram matrix and right-hand side of the observations)
//   H = W^T diag(lambda) W = V diag(lambda_p) V^T        (r x r; the eigenvalues of scalismo's D Minv D, which is (D W)(D W)^T)
//   T = W V,   Q0_new = R (Q0 T) = U_p sqrt(lambda_p)    (one pass over the basis: basis_rotate_kernel)
//   a = W W^T rhs,   mean_new = R (mean + Q0 a),   ref_new = R (ref - c) + c + t
// No division by a prior variance anywhere: a model with lambda_k = 0 gives lambda_p = 0 for that direction.
// Also the home of the r x r tail every derived-model builder ends in (gp.h): eig_descending_to_host, launch_factor_rows, moment_trace
// and launch_basis_rotate; the cut of the spectrum is spectrum_plan.h.
#include "basis_rotate.h"
#include "spectrum_plan.h"

#include <algorithm>
#include <cmath>

namespace {

// The column chunk [n0, n0 + 16 NT) of R (Q0_rows T) for the wave's 16 vertices, stored (tile and store layout: basis_rotate.h)
template <int NT>
__device__ __forceinline__ void rotate_chunk(const double *__restrict__ qrow, int rs, int rp, const double *__restrict__ T, int n0, int kq, int cl,
                                             const Rot3 &rot, double *__restrict__ out, int64_t vleft) {
    v4f64 acc[3][NT];
    rotate_clear<NT>(acc);
    rotate_accumulate<NT>(acc, qrow, rs, rp, T, n0, kq, cl);
    rotate_store<NT>(acc, rp, n0, kq, cl, rot, out, vleft);
}

// Qn[3 s + d][:] = sum_e R[d][e] (Qs[3 src(s) + e][:] T) for the device rows s < M of the new model, src(s) = iperm_src[perm_new[s]]: the
// source row of the vertex the new model keeps at row s (both models order their rows by the Morton code of their own ref + mean).
// Workgroup b takes the 16 kRotWaves vertices b / nchunks and the column chunk b % nchunks: the workgroups that share basis rows are
// neighbours in dispatch order.  Qs has kBasisRowSlack zero rows behind row 3 M: the lanes of vertices past the last one read those.
// T: [rs][rp] (rs: padded width of the source basis -- the posterior keeps it, rs == rp; a PCA model has fewer columns than the data
// it comes from, pca_model.hip), zero beyond the ranks, so the columns r .. rp - 1 of Qn come out as sums of zeros.  Rows 3 M and
// beyond are not written.
__global__ __launch_bounds__(64 * kRotWaves) void basis_rotate_kernel(const double *__restrict__ Qs, int64_t M, int rs, int rp, const double *__restrict__ T,
                                                                      Rot3 rot, const int32_t *__restrict__ perm_new,
                                                                      const int32_t *__restrict__ iperm_src, int nchunks, double *__restrict__ Qn) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t vb = blockIdx.x / nchunks;
    const int chunk = (int)(blockIdx.x - vb * nchunks);
    const int64_t v0 = (vb * kRotWaves + wave) * kRotVerts;
    if (v0 >= M) return;
    const int64_t v = v0 + cl;
    const int64_t srow = v < M ? (int64_t)iperm_src[perm_new[v]] : M;
    const double *qrow = Qs + 3 * srow * (int64_t)rs;
    double *out = Qn + 3 * v0 * (int64_t)rp;
    const int nt = rp / 16, t0 = chunk * kRotChunkTiles;
    switch (min(nt - t0, kRotChunkTiles)) {
        case 1: rotate_chunk<1>(qrow, rs, rp, T, 16 * t0, kq, cl, rot, out, M - v0); break;
        case 2: rotate_chunk<2>(qrow, rs, rp, T, 16 * t0, kq, cl, rot, out, M - v0); break;
        case 3: rotate_chunk<3>(qrow, rs, rp, T, 16 * t0, kq, cl, rot, out, M - v0); break;
        case 4: rotate_chunk<4>(qrow, rs, rp, T, 16 * t0, kq, cl, rot, out, M - v0); break;
        default: break;
    }
}

// ---- the r x r step.  W is upper triangular (row stride ldw): only k <= min(i, j) contributes to H, only k >= i to a row of W V.
// H[i][j] = sum_k W[k][i] lambda_k W[k][j], row stride ldh; the product of the two factor entries first: H[i][j] and H[j][i] are the
// same float
__global__ __launch_bounds__(256) void factor_gram_kernel(int r, const double *__restrict__ W, int64_t ldw, const double *__restrict__ lam,
                                                          double *__restrict__ H, int ldh) {
    const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= r || j >= r) return;
    double acc = 0.0;
    for (int k = 0; k <= min(i, j); ++k) acc = __builtin_fma(W[k * ldw + i] * W[k * ldw + j], lam[k], acc);
    H[(int64_t)i * ldh + j] = acc;
}

// T [rp][rp] = W V (V[k * r + j]: component k of eigenvector j), zero beyond the rank
__global__ __launch_bounds__(256) void factor_vectors_kernel(int r, int rp, const double *__restrict__ W, int64_t ldw, const double *__restrict__ V,
                                                             double *__restrict__ T) {
    const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= rp || j >= rp) return;
    double acc = 0.0;
    if (i < r && j < r)
        for (int k = i; k < r; ++k) acc = __builtin_fma(W[i * ldw + k], V[(int64_t)k * r + j], acc);
    T[(int64_t)i * rp + j] = acc;
}

// T [rsp][kp]: rows row0 .. row0 + rs of V[:, :k] (V [n][n]), zero padded (launch_factor_rows, gp.h)
__global__ __launch_bounds__(256) void factor_rows_kernel(const double *__restrict__ V, int n, int row0, int rs, int rsp, int k, int kp,
                                                          double *__restrict__ T) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)rsp * kp) return;
    const int i = (int)(e / kp), j = (int)(e - (int64_t)i * kp);
    T[e] = (i < rs && j < k) ? V[(int64_t)(row0 + i) * n + j] : 0.0;
}

// a [rp] = W (W^T rhs) = (I + G)^-1 rhs, zero beyond the rank; one workgroup
__global__ __launch_bounds__(512) void posterior_coeff_kernel(int r, int rp, const double *__restrict__ W, int64_t ldw, const double *__restrict__ rhs,
                                                              double *__restrict__ a) {
    __shared__ double y[512];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < r) {  // y[k] = sum_{i <= k} W[i][k] rhs[i]: consecutive threads, consecutive columns
        double acc = 0.0;
        for (int i = 0; i <= tid; ++i) acc = __builtin_fma(W[i * ldw + tid], rhs[i], acc);
        y[tid] = acc;
    }
    __syncthreads();
    for (int i = tid >> 6; i < rp; i += 8) {  // a[i] = sum_{k >= i} W[i][k] y[k]: a wave per row
        double acc = 0.0;
        if (i < r)
            for (int k = i + lane; k < r; k += 64) acc = __builtin_fma(W[i * ldw + k], y[k], acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) a[i] = acc;
    }
}

}  // namespace

void launch_basis_rotate(gingr_ctx *ctx, const gingr_model *src, const double *T, const Rot3 &rot, gingr_model *dst) {
    const int nchunks = (int)ceil_div(dst->rp / 16, kRotChunkTiles);
    const int64_t blocks = ceil_div(dst->M, (int64_t)kRotWaves * kRotVerts) * nchunks;
    TimerScope ts(ctx, 10);
    hipLaunchKernelGGL(basis_rotate_kernel, dim3((unsigned)blocks), dim3(64 * kRotWaves), 0, ctx->stream, src->Q0, dst->M, (int)src->rp, (int)dst->rp, T,
                       rot, dst->perm, src->iperm, nchunks, dst->Q0);
}

// ---- the r x r tail the derived-model builders share (declared in gp.h)
int eig_descending_to_host(gingr_ctx *ctx, const double *Gs, int32_t ld, int32_t n, double shift, const char *who, const char *what, double *evals,
                           double *V, std::vector<double> &lam) {
    GINGR_TRY(launch_jacobi_eig(ctx, Gs, ld, n, evals, V, true));
    lam.resize((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(lam.data(), evals, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (double &v : lam) {
        if (!std::isfinite(v)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite %s", who, what);
        v = spectrum_plan::unshift(v, shift);
    }
    return GINGR_OK;
}

void launch_factor_rows(gingr_ctx *ctx, const double *V, int n, int row0, int rs, int rsp, int k, int kp, double *T) {
    hipLaunchKernelGGL(factor_rows_kernel, dim3((unsigned)ceil_div((int64_t)rsp * kp, 256)), dim3(256), 0, ctx->stream, V, n, row0, rs, rsp, k, kp, T);
}

int moment_trace(gingr_ctx *ctx, const double *S, int32_t r, int32_t rp, double *trace) {
    std::vector<double> diag((size_t)r);
    HIP_TRY(ctx, hipMemcpy2D(diag.data(), sizeof(double), S, (size_t)(rp + 1) * sizeof(double), sizeof(double), (size_t)r, hipMemcpyDeviceToHost));
    double t = 0.0;
    for (int32_t j = 0; j < r; ++j) t += diag[(size_t)j];
    *trace = t;
    return GINGR_OK;
}

// the new model from G and rhs of the observations; f: a fitter on the source model whose state holds the rigid transform
static int posterior_model_build(gingr_fitter *f, const double *G, const double *rhs, const char *who, gingr_model **out) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    const int32_t r = m->r, rp = m->rp;
    const dim3 tiles((unsigned)(rp / 16), (unsigned)(rp / 16));
    HIP_TRY(ctx, ensure(f->cov_work, (size_t)posterior_factor_work_doubles(rp) * sizeof(double)));
    DevBuf small, H, V, T, shape, aos;  // small: lambda [rp], a [rp], lambda_p [rp]
    HIP_TRY(ctx, small.alloc((size_t)3 * rp * sizeof(double)));
    HIP_TRY(ctx, H.alloc((size_t)rp * rp * sizeof(double)));
    HIP_TRY(ctx, V.alloc((size_t)r * r * sizeof(double)));
    HIP_TRY(ctx, T.alloc((size_t)rp * rp * sizeof(double)));
    HIP_TRY(ctx, shape.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, aos.alloc((size_t)3 * M * sizeof(double)));
    double *lam = small.as<double>(), *a = lam + rp, *lam_p = a + rp;
    int64_t ldw = 0;
    int32_t *flag = nullptr;
    const double *W = launch_posterior_factor(ctx, r, rp, G, f->cov_work.as<double>(), &ldw, &flag);
    // the posterior mean mesh R (ref + mean + Q0 a - c) + c + t in the caller's point order, with the state's rigid transform
    hipLaunchKernelGGL(posterior_coeff_kernel, dim3(1), dim3(512), 0, ctx->stream, (int)r, (int)rp, W, ldw, rhs, a);
    SweepArgs sa = base_args(f);
    sa.coef0 = a;
    sa.shape_out = shape.as<double>();
    launch_sweep(ctx, SWEEP_POSED, sa);
    launch_soa_to_aos(ctx, shape.as<double>(), M, aos.as<double>(), m->perm);
    GINGR_TRY(check_launch(ctx));
    std::vector<double> mesh((size_t)3 * M), href((size_t)3 * M), hmean((size_t)3 * M), lam_h;
    DevState hst;
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&hst, f->st, sizeof(hst), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(mesh.data(), aos.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "%s: I + G of the observations is not positive definite", who);
    for (int64_t i = 0; i < 3 * M; ++i)
        if (!std::isfinite(mesh[(size_t)i])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite posterior mean", who);
    // H = W^T diag(lambda) W = V diag(lambda_p) V^T (descending), T = W V
    HIP_TRY(ctx, hipMemcpyAsync(lam, m->variance.data(), (size_t)r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(factor_gram_kernel, tiles, dim3(256), 0, ctx->stream, (int)r, W, ldw, lam, H.as<double>(), (int)rp);
    GINGR_TRY(check_launch(ctx));
    // (no shift: H is as definite as the prior; a direction the prior does not have is rounding around zero and clamps to 0)
    GINGR_TRY(eig_descending_to_host(ctx, H.as<double>(), rp, r, 0.0, who, "posterior variance", lam_p, V.as<double>(), lam_h));
    hipLaunchKernelGGL(factor_vectors_kernel, tiles, dim3(256), 0, ctx->stream, (int)r, (int)rp, W, ldw, V.as<double>(), T.as<double>());
    GINGR_TRY(check_launch(ctx));
    // reference and mean displacement of the new model (host: they fix its row order)
    GINGR_TRY(gingr_model_download(ctx, m, href.data(), nullptr, nullptr, nullptr));
    for (int64_t i = 0; i < M; ++i) {
        const double p[3] = {href[(size_t)3 * i] - hst.center[0], href[(size_t)3 * i + 1] - hst.center[1], href[(size_t)3 * i + 2] - hst.center[2]};
        for (int d = 0; d < 3; ++d) {
            const double x = (hst.R[3 * d] * p[0] + hst.R[3 * d + 1] * p[1]) + hst.R[3 * d + 2] * p[2] + hst.center[d] + hst.t[d];
            href[(size_t)3 * i + d] = x;
            hmean[(size_t)3 * i + d] = mesh[(size_t)3 * i + d] - x;
        }
    }
    Rot3 rot;
    for (int q = 0; q < 9; ++q) rot.R[q] = hst.R[q];
    auto fill = [&](gingr_model *nm) -> int {
        launch_basis_rotate(ctx, m, T.as<double>(), rot, nm);
        return check_launch(ctx);
    };
    return model_create_impl(ctx, M, r, href.data(), hmean.data(), lam_h.data(), 0, M, fill, out);
}

// posterior model of the fitter's current state: built like posterior_covariance (posterior_cov.hip) -- phases 0 and 1 of the state
// (they do not touch it; landmarks are in G already), then the common part
static int fitter_posterior_model(gingr_fitter *f, const Correspondence &c, gingr_model **out) {
    if (!out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    GINGR_TRY(check_correspondence(f, c));
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (m->M != m->M_total || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "posterior_model: single shard only");
    GINGR_TRY(fitter_posterior_inputs(f, c));
    const double *G = f->seg1_live();
    return posterior_model_build(f, G, G + (int64_t)m->rp * m->rp, "posterior_model", out);
}

extern "C" {

int gingr_model_posterior(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3], const double translation[3],
                          const double *obs_xyz, const double *weight, int32_t n_lm, const int32_t *lm_pid, const double *lm_xyz,
                          const double *lm_cov, gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!model || !euler || !center || !translation || !obs_xyz || !weight)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_posterior: null argument");
    if (model->M != model->M_total) return gingr_set_error(ctx, GINGR_ERR_STATE, "model_posterior: single shard only");
    gingr_fitter *f = nullptr;
    DevBuf sys;
    GINGR_TRY(model_observation_system(ctx, model, euler, center, translation, obs_xyz, weight, n_lm, lm_pid, lm_xyz, lm_cov, &f, sys));
    const double *G = sys.as<double>();
    const int rc = posterior_model_build(f, G, G + (int64_t)model->rp * model->rp, "model_posterior", out);
    gingr_fitter_destroy(f);
    return rc;
}

int gingr_fitter_posterior_model_cpd(gingr_fitter *f, const gingr_cpd_params *p, gingr_model **out) {
    return fitter_posterior_model(f, abi_correspondence(0, p, nullptr), out);
}
int gingr_fitter_posterior_model_icp(gingr_fitter *f, const gingr_icp_params *p, gingr_model **out) {
    return fitter_posterior_model(f, abi_correspondence(1, nullptr, p), out);
}
int gingr_fitter_posterior_model_icp_surface(gingr_fitter *f, const gingr_icp_params *p, gingr_model **out) {
    return fitter_posterior_model(f, abi_correspondence(2, nullptr, p), out);
}
int gingr_fitter_posterior_model_pairs(gingr_fitter *f, gingr_model **out) {
    return fitter_posterior_model(f, abi_correspondence(3, nullptr, nullptr), out);
}

}  // extern "C"
