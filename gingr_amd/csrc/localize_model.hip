// A resident model localized (C ABI in include/gingr_hip.h: gingr_model_localize): the model whose covariance is the source's, tapered
// element-wise by a Gaussian of the distance between the reference points (Luethi et al., Gaussian Process Morphable Models:
// localized statistical shape models),
//   K[(i,a),(j,b)] = g(x_i, x_j) sum_k Q[3i+a, k] Q[3j+b, k],   g(x, y) = exp(-|x - y|^2 / sigma^2),   Q = U sqrt(lambda) of the source.
// K is a full 3 x 3 block kernel read from the basis in HBM.  It is factored by the generic pivoted Cholesky over the 3M (point,
// coordinate) entries (gpmm.hip: pc_step_kernel<Tapered> under gpmm_factor::Factor's driver -- the GPMM builder's pivot, tie and stop
// rules) and re-diagonalised by the tail of the generic GPMM build (gpmm_factor::generic_tail).  The factor works in the caller's entry
// order with lanes along the entries, so the basis is gathered and transposed once per call: Qt[q][3i+d] = Q0[3 iperm[i] + d][q].
// Only reference and mean pass through the host (download_ref_mean, model.hip).  The kept components are the cut of spectrum_plan.h, the
// complete-model check is model.hip's (gp.h).  Every sum has a fixed order: two calls give the same bits.
#include "gp.h"

#include "gpmm_factor.h"
#include "gpmm_plan.h"
#include "spectrum_plan.h"

#include <algorithm>
#include <cmath>

namespace {

// Qt[q][e] = Q0[(3 iperm[e / 3] + e % 3) rp + q]: a 32 x 32 tile through LDS, reads along the columns of a row, writes along the entries
__global__ __launch_bounds__(256) void localize_gather_kernel(const double *__restrict__ Q0, int32_t r, int32_t rp, const int32_t *__restrict__ iperm,
                                                              int64_t n, double *__restrict__ Qt) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t e0 = (int64_t)blockIdx.x * 32;
    const int q0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const int64_t e = e0 + j;
        const int q = q0 + tx;
        double v = 0.0;
        if (e < n && q < r) {
            const int64_t i = e / 3;
            v = Q0[(3 * (int64_t)iperm[i] + (e - 3 * i)) * rp + q];
        }
        tile[j][tx] = v;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int64_t e = e0 + tx;
        const int q = q0 + j;
        if (e < n && q < r) Qt[(int64_t)q * n + e] = tile[tx][j];
    }
}

}  // namespace

extern "C" {

int gingr_model_localize(gingr_ctx *ctx, const gingr_model *model, double sigma, double relative_tolerance, int32_t max_rank, gingr_model **out,
                         gingr_localize_info *info) {
    if (out) *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_localize";
    if (!model) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (const char *fault = complete_model_fault(ctx, model))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the model %s (need a complete, finalized model of this context)", who, fault);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: sigma must be positive and finite", who);
    if (!(relative_tolerance >= 0.0) || !(relative_tolerance < 1.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: relative_tolerance must be in [0, 1)", who);
    if (max_rank < 0) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: max_rank must not be negative", who);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = model->M, n = 3 * M;
    const int32_t r = model->r;

    // ---- 1. reference and mean pass through the host once (model_create_impl takes them there); the reference goes back as the planes
    // of the caller's order that the factor's taper reads
    std::vector<double> href, hmean;
    GINGR_TRY(download_ref_mean(ctx, model, href, hmean));
    DevBuf aos, soa, qt;
    HIP_TRY(ctx, aos.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, soa.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(aos.p, href.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos.as<double>(), M, soa.as<double>());
    const double *s = soa.as<double>();
    const Cloud pts{s, s + M, s + 2 * M, M};

    // ---- 2. the basis, gathered into the caller's entry order and transposed
    HIP_TRY(ctx, qt.alloc((size_t)r * n * sizeof(double)));
    hipLaunchKernelGGL(localize_gather_kernel, dim3((unsigned)ceil_div(n, 32), (unsigned)ceil_div(r, 32)), dim3(256), 0, ctx->stream, model->Q0, r,
                       model->rp, model->iperm, n, qt.as<double>());
    GINGR_TRY(check_launch(ctx));

    // ---- 3. K ~ L L^T: the generic factor's ceiling of 512 columns (its swap log lives in LDS)
    gpmm_factor::Factor fg;
    const int32_t cap = (int32_t)std::min<int64_t>(n, 512);
    GINGR_TRY(fg.init_tapered(ctx, gpmm_factor::gaussian_specs(sigma, 1.0), pts, gpmm_factor::TaperBasis{qt.as<double>(), r}, cap, 21));
    GINGR_TRY(fg.run_to_tolerance(relative_tolerance));
    const int32_t cols = fg.ks;
    const double trace = fg.htrace[0];
    if (!std::isfinite(trace)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite trace of the covariance", who);
    if (cols < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the covariance has no positive entry (rank 0)", who);
    const double residual = fg.htrace[(size_t)cols];
    if (!std::isfinite(residual)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite residual trace", who);
    // reached: below the tolerance, or nothing left to pivot (every entry taken, or no positive residual) before the ceiling
    const bool reached = gpmm_plan::below_tolerance(residual, trace, relative_tolerance) || cols < cap || (int64_t)cols == n;

    // ---- 4. L^T L = V diag(lambda') V^T, Q' = L V; the leading components above the noise floor of the Gram route
    // (spectrum_plan.h: no shift, the noise floor of the Gram route as the tolerance)
    double kept = 0.0;
    std::vector<double> lam;
    auto choose = [&](std::vector<double> &ev, int32_t *keep) -> int {
        const spectrum_plan::Cut cut = spectrum_plan::cut(ev.data(), (int)ev.size(), 0.0, cols, max_rank, 1e-12);
        if (cut.first_nonfinite >= 0) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite eigenvalue", who);
        if (cut.k < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: no eigenvalue of the tapered covariance passes the cutoff (rank 0)", who);
        kept = cut.kept;
        *keep = cut.k;
        return GINGR_OK;
    };
    GINGR_TRY(gpmm_factor::generic_tail(ctx, fg, M, href.data(), hmean.data(), 0, M, lam, choose, out));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        info->columns = cols;
        info->rank = (*out)->r;
        info->tolerance_reached = reached ? 1 : 0;
        info->residual_fraction = residual / trace;
        info->total_variance = trace;
        info->kept_variance = kept;
    }
    return GINGR_OK;
}

}  // extern "C"
