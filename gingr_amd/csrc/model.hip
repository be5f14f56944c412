// Model upload, finalize, download, truncation and re-sampling on a new reference, and the stateless model operators (instance,
// coefficients, posterior mean), which borrow a short-lived fitter (C ABI in include/gingr_hip.h).  Behind model_create_impl: the checks
// and transfers the derived-model builders share (complete_model_fault, check_finite, for_each_shape_stage, download_ref_mean; gp.h).
#include "fitter.h"
#include "model_extend.h"

#include <algorithm>
#include <cmath>
#include <functional>

namespace {

// stage[k*3M + 3*perm[s] + d] = Q0[(3s+d)*rp + k] / sqrt(variance[k])   (inverse of pack_basis_kernel)
__global__ __launch_bounds__(256) void unpack_basis_kernel(const double *__restrict__ Q0, const double *__restrict__ variance,
                                                           int64_t M, int32_t r, int32_t rp,
                                                           const int32_t *__restrict__ perm, double *__restrict__ stage) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * M * r) return;
    const int64_t row = idx / r;
    const int32_t k = (int32_t)(idx - row * r);
    const int64_t s = row / 3, d = row - 3 * s;
    const double sd = sqrt(variance[k]);
    stage[(int64_t)k * 3 * M + 3 * (int64_t)(perm ? perm[s] : s) + d] = sd > 0.0 ? Q0[row * rp + k] / sd : 0.0;
}

// Q[(row) * rpn + q] = q < k ? Qs[row * rps + q] : 0 for the 3M basis rows (the slack rows behind them are cleared by model_create_impl)
__global__ __launch_bounds__(256) void truncate_basis_kernel(const double *__restrict__ Qs, int32_t rps, int64_t rows, int32_t k, int32_t rpn,
                                                             double *__restrict__ Q) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * rpn) return;
    const int64_t row = idx / rpn;
    const int32_t q = (int32_t)(idx - row * rpn);
    Q[idx] = q < k ? Qs[row * rps + q] : 0.0;
}

// ---- coordinate-separable bases (gp.h: gingr_model::separable) ----------------------------------------------------------------------
// partial[b][d * rp + k] = 1 when any entry of column k in the rows 3i + d of workgroup b's share is not +-0.0 (a NaN counts), else 0.
// Every thread owns the columns k = tid, tid + 256, ... and walks its workgroup's rows: whole 2 KB runs per load instruction, no atomics.
constexpr int kSepBlocks = 256;
__global__ __launch_bounds__(256) void sep_flags_kernel(const double *__restrict__ Q0, int64_t rows, int32_t rp, int32_t *__restrict__ partial) {
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    for (int k = threadIdx.x; k < rp; k += 256) {
        int32_t fl[3] = {0, 0, 0};
        for (int64_t row = r0; row < r1; ++row)
            if (Q0[row * rp + k] != 0.0) fl[row % 3] = 1;
        for (int d = 0; d < 3; ++d) partial[(int64_t)blockIdx.x * 3 * rp + d * rp + k] = fl[d];
    }
}
// flags[q] = OR over the workgroups' partials, q < 3 rp
__global__ __launch_bounds__(256) void sep_flags_reduce_kernel(const int32_t *__restrict__ partial, int nblocks, int32_t n, int32_t *__restrict__ flags) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    int32_t f = 0;
    for (int b = 0; b < nblocks; ++b) f |= partial[(int64_t)b * n + q];
    flags[q] = f;
}
// Qc[d][p][k] = Q0[3p + d][col(d, k)], zero behind the class's last column (the slack rows are cleared by the caller)
__global__ __launch_bounds__(256) void compact_basis_kernel(const double *__restrict__ Q0, int64_t M, int32_t rp, const int32_t *__restrict__ sep_map,
                                                            double *__restrict__ Qc) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * M * kCompactCols) return;
    const int k = (int)(idx % kCompactCols);
    const int64_t pd = idx / kCompactCols;
    const int64_t p = pd % M;
    const int d = (int)(pd / M);
    const int col = sep_map[SepMap{rp}.col(d, k)];
    Qc[d * compact_plane_doubles(M) + p * kCompactCols + k] = col >= 0 ? Q0[(3 * p + d) * rp + col] : 0.0;
}

// Decides gingr_model::separable from the local Q0 and, where the compact passes can use it, builds Qc and sep_map.
int model_detect_separable(gingr_ctx *ctx, gingr_model *m) {
    const int32_t r = m->r, rp = m->rp;
    const int64_t rows = 3 * m->M;
    dev_free(m->Qc), dev_free(m->sep_map);
    m->Qc = nullptr, m->sep_map = nullptr;
    m->separable = false;
    const int nb = (int)std::min<int64_t>(kSepBlocks, (rows + 63) / 64);
    DevBuf part, flags;
    HIP_TRY(ctx, part.alloc((size_t)nb * 3 * rp * sizeof(int32_t)));
    HIP_TRY(ctx, flags.alloc((size_t)3 * rp * sizeof(int32_t)));
    hipLaunchKernelGGL(sep_flags_kernel, dim3(nb), dim3(256), 0, ctx->stream, m->Q0, rows, rp, part.as<int32_t>());
    hipLaunchKernelGGL(sep_flags_reduce_kernel, dim3((unsigned)ceil_div(3 * rp, 256)), dim3(256), 0, ctx->stream, part.as<int32_t>(), nb, 3 * rp,
                       flags.as<int32_t>());
    GINGR_TRY(check_launch(ctx));
    std::vector<int32_t> hf((size_t)3 * rp);
    HIP_TRY(ctx, hipMemcpyAsync(hf.data(), flags.p, hf.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    m->col_class.assign((size_t)r, 0);
    for (int d = 0; d < 3; ++d) m->class_cols[d].clear();
    bool sep = true;
    for (int32_t k = 0; k < r; ++k) {
        const int n = hf[(size_t)k] + hf[(size_t)rp + k] + hf[(size_t)2 * rp + k];
        if (n > 1) sep = false;
        const int cls = hf[(size_t)k] ? 0 : hf[(size_t)rp + k] ? 1 : hf[(size_t)2 * rp + k] ? 2 : 0;  // an all-zero column joins class x
        m->col_class[(size_t)k] = cls;
        m->class_cols[cls].push_back(k);
    }
    for (int d = 0; d < 3; ++d) m->rc[d] = (int32_t)m->class_cols[d].size();
    if (!sep) {
        m->col_class.clear();
        for (int d = 0; d < 3; ++d) m->class_cols[d].clear(), m->rc[d] = 0;
        return GINGR_OK;
    }
    m->separable = true;
    // the compact passes: one shard, the ranks of the triangle kernel, and every class inside a plane's width
    if (m->M != m->M_total || rp > 112 || std::max(m->rc[0], std::max(m->rc[1], m->rc[2])) > kCompactCols) return GINGR_OK;
    const SepMap sm{rp};
    std::vector<int32_t> map((size_t)sm.total(), -1);
    for (int d = 0; d < 3; ++d)
        for (int32_t p = 0; p < m->rc[d]; ++p) {
            const int32_t k = m->class_cols[d][(size_t)p];
            map[(size_t)sm.cls(k)] = d;
            map[(size_t)sm.pos(k)] = p;
            map[(size_t)sm.col(d, p)] = k;
        }
    GINGR_TRY(dev_alloc(ctx, &m->sep_map, map.size()));
    GINGR_TRY(dev_alloc(ctx, &m->Qc, (size_t)3 * compact_plane_doubles(m->M)));
    HIP_TRY(ctx, hipMemcpyAsync(m->sep_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    for (int d = 0; d < 3; ++d)
        HIP_TRY(ctx, hipMemsetAsync(m->Qc + d * compact_plane_doubles(m->M) + m->M * kCompactCols, 0,
                                    (size_t)kCompactRowSlack * kCompactCols * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(compact_basis_kernel, dim3((unsigned)ceil_div(3 * m->M * kCompactCols, 256)), dim3(256), 0, ctx->stream, m->Q0, m->M, rp,
                       m->sep_map, m->Qc);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // map leaves scope
    return GINGR_OK;
}

int model_finalize_impl(gingr_ctx *ctx, gingr_model *m) {
    GINGR_TRY(model_detect_separable(ctx, m));
    DevBuf work, flag;
    HIP_TRY(ctx, work.alloc((size_t)binv_work_doubles(m->rp) * sizeof(double)));
    HIP_TRY(ctx, flag.alloc(sizeof(int32_t)));
    launch_binv(ctx, m->r, m->rp, m->mom, work.as<double>(), m->Binv, flag.as<int32_t>());
    GINGR_TRY(check_launch(ctx));
    int32_t err = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&err, flag.p, sizeof(err), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (err) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "model finalize: Q^T Q / 1e-5 + I is not positive definite");
    // constant products of the moment form (gp.h: cmat, PostVec): C = Binv S_tot / eps, Binv S[d][e], Binv S[d][e] C (work = S[d][e] C)
    const MomentLayout ml{m->rp};
    const int64_t rr = (int64_t)m->rp * m->rp;
    launch_small_gemm(ctx, m->r, m->rp, m->Binv, m->mom + ml.stot(), 1.0 / GINGR_COEFF_NOISE, m->cmat);
    for (int d = 0; d < 3; ++d)
        for (int e = 0; e < 3; ++e) {
            launch_small_gemm(ctx, m->r, m->rp, m->Binv, m->mom + ml.S(d, e), 1.0, m->cmat + (1 + d * 3 + e) * rr);
            launch_small_gemm(ctx, m->r, m->rp, m->mom + ml.S(d, e), m->cmat, 1.0, work.as<double>());
            launch_small_gemm(ctx, m->r, m->rp, m->Binv, work.as<double>(), 1.0, m->cmat + (10 + d * 3 + e) * rr);
        }
    // the moment vectors V[d][e], W[d] (contiguous in mom from V(0, 0) on) and Binv times them; then the scalars of the full model
    const PostVec pvl{m->rp};
    launch_postvec(ctx, m->r, m->rp, m->Binv, m->mom + ml.V(0, 0), m->pvec);
    {
        double cst[16];
        for (int q = 0; q < 9; ++q) cst[q] = m->Pp[q];
        for (int q = 0; q < 3; ++q) {
            cst[9 + q] = m->Ps[q];
            cst[12 + q] = m->c0[q];
        }
        cst[15] = (double)m->M_total;
        HIP_TRY(ctx, hipMemcpyAsync(m->pvec + pvl.consts(), cst, sizeof(cst), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // cst leaves scope
    }
    GINGR_TRY(check_launch(ctx));
    // The eigen-decomposition S_tot = V diag(lam) V^T for the uniform-weight posterior (point-cloud ICP without landmarks: the
    // posterior (I + S_tot / sigma2)^-1 rhs is two mat-vecs then).  Decided HERE, once, outside every asynchronous update: S_tot is
    // the all-reduced moment, bit-identical on every shard, and the decomposition is deterministic, so all shards of a sharded model
    // take the same path.  Up to the 192 columns of the register kernel (eig.hip: 0.24 ms at rank 100, 3.5 ms at 192); above that the
    // two-sided kernel would take tens of ms of every model's set-up, more than the Cholesky path costs an ICP run (0.1 ms an iteration).
    m->eig_ready = false;
    if (m->r <= kSymEigColsMaxN) {
        if (launch_jacobi_eig(ctx, m->mom + ml.stot(), m->rp, m->r, m->eigL, m->eigV) == GINGR_OK)
            m->eig_ready = true;
        else
            (void)hipGetLastError();
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    m->finalized = true;
    return GINGR_OK;
}

}  // namespace

// ===================================================================================================== model

// Shared by gingr_model_upload (basis from the host) and the on-device GPMM builder (gpmm.hip): everything of a model
// except how Q0 = U sqrt(lambda) gets filled.  fill_basis runs after the row permutation exists and must write all of
// m->Q0 ([3M][rp], device row order, zero padded) on ctx->stream.
int model_create_impl(gingr_ctx *ctx, int64_t M_total, int32_t rank, const double *ref, const double *mean,
                      const double *variance, int64_t row_begin, int64_t row_end,
                      const std::function<int(gingr_model *)> &fill_basis, gingr_model **out, bool finalize) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (M_total < 1 || rank < 1 || rank > 512 || !ref || !mean || !variance)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_upload: need M >= 1 and 1 <= rank <= 512");
    if (row_begin < 0 || row_end > M_total || row_begin >= row_end)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_upload: bad row shard [%lld,%lld)", (long long)row_begin,
                               (long long)row_end);
    for (int32_t k = 0; k < rank; ++k)
        if (!(variance[k] >= 0.0)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_upload: variance[%d] < 0", k);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gingr_model *m = new gingr_model();
    m->ctx = ctx;
    m->M_total = M_total;
    m->row_begin = row_begin;
    m->row_end = row_end;
    m->M = row_end - row_begin;
    m->r = rank;
    m->rp = (int32_t)round_up(rank, 16);
    m->variance.assign(variance, variance + rank);
    const int64_t M = m->M;
    // centroid of the full reference (identical on every shard)
    double c[3] = {0, 0, 0};
    for (int64_t i = 0; i < M_total; ++i) {
        c[0] += ref[3 * i];
        c[1] += ref[3 * i + 1];
        c[2] += ref[3 * i + 2];
    }
    for (int d = 0; d < 3; ++d) m->c0[d] = c[d] / (double)M_total;

    int rc = GINGR_OK;
    DevBuf aos;
    auto fail = [&](int code) {
        gingr_model_destroy(m);
        return code;
    };
    if ((rc = dev_alloc(ctx, &m->Q0, (size_t)(3 * M + kBasisRowSlack) * m->rp)) || (rc = dev_alloc(ctx, &m->ref, (size_t)3 * M)) ||
        (rc = dev_alloc(ctx, &m->mean, (size_t)3 * M)) || (rc = dev_alloc(ctx, &m->mom, (size_t)MomentLayout{m->rp}.total())) ||
        (rc = dev_alloc(ctx, &m->Binv, (size_t)m->rp * m->rp)) || (rc = dev_alloc(ctx, &m->eigV, (size_t)m->r * m->r)) ||
        (rc = dev_alloc(ctx, &m->eigL, (size_t)m->r)) ||
        (rc = dev_alloc(ctx, &m->cmat, (size_t)19 * m->rp * m->rp)) ||
        (rc = dev_alloc(ctx, &m->pvec, (size_t)PostVec{m->rp}.total())))
        return fail(rc);
    if (aos.alloc((size_t)3 * M * sizeof(double)) != hipSuccess)
        return fail(gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: out of device memory"));
    // device row order = Morton order of the local mean shape
    {
        std::vector<double> pts((size_t)3 * M);
        for (int64_t i = 0; i < 3 * M; ++i) pts[(size_t)i] = ref[3 * row_begin + i] + mean[3 * row_begin + i];
        kd_leaf_order(pts.data(), M, m->hperm);
        m->hiperm.resize((size_t)M);
        for (int64_t sidx = 0; sidx < M; ++sidx) m->hiperm[(size_t)m->hperm[(size_t)sidx]] = (int32_t)sidx;
        if ((rc = dev_alloc(ctx, &m->perm, (size_t)M)) || (rc = dev_alloc(ctx, &m->iperm, (size_t)M))) return fail(rc);
        if (hipMemcpy(m->perm, m->hperm.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(m->iperm, m->hiperm.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
            return fail(gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: permutation copy failed"));
    }
    (void)hipMemsetAsync(m->Q0 + (size_t)3 * M * m->rp, 0, (size_t)kBasisRowSlack * m->rp * sizeof(double), ctx->stream);
    if ((rc = fill_basis(m))) return fail(rc);
    (void)hipMemcpyAsync(aos.p, ref + 3 * row_begin, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    launch_aos_to_soa(ctx, aos.as<double>(), M, m->ref, m->perm);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipMemcpyAsync(aos.p, mean + 3 * row_begin, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    launch_aos_to_soa(ctx, aos.as<double>(), M, m->mean, m->perm);
    // one-off moments of the local rows (MomentLayout): S_tot, S[d][e], V[d][e], W[d]
    {
        const MomentLayout ml{m->rp};
        DevBuf gws, sws, ptil, ev;
        if (gws.alloc((size_t)std::max(gram_ws_doubles(M, m->rp), moment_grams_ws_doubles(M, m->rp)) * sizeof(double)) != hipSuccess ||
            sws.alloc((size_t)sweep_ws_doubles(M, m->rp) * sizeof(double)) != hipSuccess ||
            ptil.alloc((size_t)3 * M * sizeof(double)) != hipSuccess || ev.alloc((size_t)3 * M * sizeof(double)) != hipSuccess)
            return fail(gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: out of device memory"));
        launch_gram(ctx, m->Q0, M, m->rp, nullptr, gws.as<double>(), m->mom + ml.stot());
        launch_moment_grams(ctx, m->Q0, M, m->rp, gws.as<double>(), m->mom);
        launch_centered_mean(ctx, m, ptil.as<double>());
        std::vector<double> ones((size_t)M, 1.0);
        DevBuf dones;
        if (dones.alloc((size_t)M * sizeof(double)) != hipSuccess)
            return fail(gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: out of device memory"));
        (void)hipMemcpyAsync(dones.p, ones.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        SweepArgs a;
        memset(&a, 0, sizeof(a));
        a.Q0 = m->Q0;
        a.ref = m->ref;
        a.mean = m->mean;
        a.M = M;
        a.rp = m->rp;
        a.evec = ev.as<double>();
        a.partial = sws.as<double>();
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e <= 3; ++e) {  // e == 3: the all-ones plane gives W[d]
                (void)hipMemsetAsync(ev.p, 0, (size_t)3 * M * sizeof(double), ctx->stream);
                const double *src = e < 3 ? ptil.as<double>() + (size_t)e * M : dones.as<double>();
                (void)hipMemcpyAsync(ev.as<double>() + (size_t)d * M, src, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice,
                                     ctx->stream);
                a.out = m->mom + (e < 3 ? ml.V(d, e) : ml.W(d));
                launch_sweep(ctx, SWEEP_RHS, a);
            }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return fail(gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: kernel launch failed"));
    }
    // host moments of p~ over the FULL model (identical on every shard)
    for (int q = 0; q < 9; ++q) m->Pp[q] = 0.0;
    for (int q = 0; q < 3; ++q) m->Ps[q] = 0.0;
    if (M != M_total) {  // a shard keeps the mean shape of the whole model on the host (gingr_fitter_set_meshes: triangle order)
        m->h_full_pts.resize((size_t)3 * M_total);
        for (int64_t i = 0; i < 3 * M_total; ++i) m->h_full_pts[(size_t)i] = ref[i] + mean[i];
    }
    for (int64_t i = 0; i < M_total; ++i) {
        double pt[3];
        for (int d = 0; d < 3; ++d) pt[d] = ref[3 * i + d] + mean[3 * i + d] - m->c0[d];
        for (int d = 0; d < 3; ++d) {
            m->Ps[d] += pt[d];
            for (int e = 0; e < 3; ++e) m->Pp[d * 3 + e] += pt[d] * pt[e];
        }
    }
    if (row_begin == 0 && row_end == M_total && finalize) {
        rc = model_finalize_impl(ctx, m);
        if (rc) return fail(rc);
    }
    *out = m;
    return GINGR_OK;
}

// ---- what the builders of a model from models or shapes share in front of model_create_impl (declared in gp.h)
const char *complete_model_fault(const gingr_ctx *ctx, const gingr_model *m) {
    if (m->ctx != ctx) return "belongs to another context";
    if (m->row_begin != 0 || m->row_end != m->M_total || m->M != m->M_total) return "is a row shard";
    if (!m->finalized) return "is not finalized";
    return nullptr;
}

int check_finite(gingr_ctx *ctx, const double *x, int64_t per, int64_t n, const char *who, const char *what) {
    for (int64_t e = 0; e < per * n; ++e)
        if (!std::isfinite(x[e])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite value in %s %lld", who, what, (long long)(e / per));
    return GINGR_OK;
}

int for_each_shape_stage(gingr_ctx *ctx, int64_t M, int n, const double *shapes, DevBuf &stage, const std::function<int(int, int)> &fn) {
    const int per_stage = (int)std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)8 << 20) / (3 * M)));  // <= 64 MB of staging
    HIP_TRY(ctx, stage.alloc((size_t)per_stage * 3 * M * sizeof(double)));
    for (int i0 = 0; i0 < n; i0 += per_stage) {
        const int cnt = std::min(per_stage, n - i0);
        HIP_TRY(ctx, hipMemcpyAsync(stage.p, shapes + (size_t)i0 * 3 * M, (size_t)cnt * 3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        GINGR_TRY(fn(cnt, i0));
        GINGR_TRY(check_launch(ctx));
    }
    return GINGR_OK;
}

int download_ref_mean(gingr_ctx *ctx, const gingr_model *m, std::vector<double> &href, std::vector<double> &hmean) {
    href.resize((size_t)3 * m->M);
    hmean.resize((size_t)3 * m->M);
    return gingr_model_download(ctx, m, href.data(), hmean.data(), nullptr, nullptr);
}

extern "C" {

int gingr_model_upload(gingr_ctx *ctx, int64_t M_total, int32_t rank, const double *ref, const double *mean,
                       const double *basis_colmajor, const double *variance, int64_t row_begin, int64_t row_end,
                       gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!basis_colmajor) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_upload: basis is null");
    DevBuf stage, var;
    auto fill = [&](gingr_model *m) -> int {
        const int64_t M = m->M;
        if (stage.alloc((size_t)3 * M * rank * sizeof(double)) != hipSuccess || var.alloc(rank * sizeof(double)) != hipSuccess)
            return gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: out of device memory");
        // basis: column k of the shard = rows [3*row_begin, 3*row_end) of host column k
        if (hipMemcpy2DAsync(stage.p, (size_t)3 * M * sizeof(double), basis_colmajor + 3 * row_begin,
                             (size_t)3 * M_total * sizeof(double), (size_t)3 * M * sizeof(double), (size_t)rank,
                             hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            return gingr_set_error(ctx, GINGR_ERR_HIP, "model_upload: basis copy failed");
        (void)hipMemcpyAsync(var.p, variance, rank * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        launch_pack_basis(ctx, stage.as<double>(), var.as<double>(), M, rank, m->rp, m->perm, m->Q0);
        return GINGR_OK;
    };
    return model_create_impl(ctx, M_total, rank, ref, mean, variance, row_begin, row_end, fill, out);
}

void gingr_model_destroy(gingr_model *m) {
    if (!m) return;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    void *ptrs[] = {m->Q0, m->ref, m->mean, m->mom, m->Binv, m->eigV, m->eigL, m->cmat, m->pvec, m->perm, m->iperm, m->Qc, m->sep_map};
    for (void *p : ptrs) dev_free(p);
    delete m;
}

int gingr_model_separable(const gingr_model *m, int32_t *separable, int32_t class_counts[3], int32_t *compact) {
    if (!m || !separable) return GINGR_ERR_BAD_ARGUMENT;
    *separable = m->separable ? 1 : 0;
    if (class_counts)
        for (int d = 0; d < 3; ++d) class_counts[d] = m->rc[d];
    if (compact) *compact = m->Qc ? 1 : 0;
    return GINGR_OK;
}

int64_t gingr_model_num_points(const gingr_model *m) { return m ? m->M : 0; }
int32_t gingr_model_rank(const gingr_model *m) { return m ? m->r : 0; }

int gingr_model_gram_exchange(gingr_model *m, void **dev_ptr, int64_t *count) {
    if (!m || !dev_ptr || !count) return GINGR_ERR_BAD_ARGUMENT;
    *dev_ptr = m->mom;
    *count = MomentLayout{m->rp}.total();
    return GINGR_OK;
}

int gingr_model_finalize(gingr_ctx *ctx, gingr_model *m) {
    if (!ctx || !m) return GINGR_ERR_BAD_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return model_finalize_impl(ctx, m);
}

// ===================================================================================== stateless model operators
static void fill_scalars(gingr_state_scalars *s, const double euler[3], const double center[3], const double translation[3],
                         double scale) {
    memset(s, 0, sizeof(*s));
    for (int q = 0; q < 3; ++q) {
        s->euler[q] = euler[q];
        s->center[q] = center[q];
        s->translation[q] = translation[q];
    }
    s->scale = scale;
    s->sigma2 = 1.0;
}

}  // extern "C"

// The posterior system of stateless observations (gingr_model_posterior_mean, gingr_model_posterior): a short-lived fitter whose state
// is the rigid transform with zero shape coefficients, and G [rp*rp] followed by rhs [rp] of the observations in `sys` (landmarks
// included).  Synchronises (the staging buffers are its own); on failure no fitter is left behind.
int model_observation_system(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                             const double translation[3], const double *obs_xyz, const double *weight, int32_t n_lm, const int32_t *lm_pid,
                             const double *lm_xyz, const double *lm_cov, gingr_fitter **f_out, DevBuf &sys) {
    gingr_fitter *f = nullptr;
    GINGR_TRY(gingr_fitter_create(ctx, model, &f));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    int rc = GINGR_OK;
    std::vector<double> zero((size_t)r, 0.0);
    gingr_state_scalars s;
    fill_scalars(&s, euler, center, translation, 1.0);
    rc = gingr_fitter_set_state(f, zero.data(), &s);
    if (!rc) rc = gingr_fitter_set_landmarks(f, n_lm, lm_pid, lm_xyz, lm_cov);
    DevBuf aos, obs, win, gws;
    if (!rc && (aos.alloc((size_t)3 * M * sizeof(double)) != hipSuccess || obs.alloc((size_t)3 * M * sizeof(double)) != hipSuccess ||
                win.alloc((size_t)M * sizeof(double)) != hipSuccess ||
                sys.alloc(((size_t)rp * rp + rp) * sizeof(double)) != hipSuccess ||
                gws.alloc((size_t)gram_ws_doubles(M, rp) * sizeof(double)) != hipSuccess))
        rc = gingr_set_error(ctx, GINGR_ERR_HIP, "out of memory");
    if (!rc) {
        std::vector<double> wo((size_t)M), wh((size_t)M);
        for (int64_t i = 0; i < M; ++i) wo[(size_t)i] = weight[i];
        for (int32_t l = 0; l < n_lm; ++l) wo[(size_t)lm_pid[l]] = 0.0;  // landmark pids carry weight 0
        for (int64_t sidx = 0; sidx < M; ++sidx) wh[(size_t)sidx] = wo[(size_t)model->hperm[(size_t)sidx]];  // device order
        (void)hipMemcpyAsync(aos.p, obs_xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        launch_aos_to_soa(ctx, aos.as<double>(), M, obs.as<double>(), model->perm);
        (void)hipMemcpyAsync(win.p, wh.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        launch_obs_points(ctx, model, f->st, obs.as<double>(), win.as<double>(), f->weight, f->evec);
        double *Gd = sys.as<double>(), *rhs = Gd + (int64_t)rp * rp;
        launch_gram(ctx, model->Q0, M, rp, f->weight, gws.as<double>(), Gd);
        SweepArgs a = base_args(f);
        a.evec = f->evec;
        a.out = rhs;
        launch_sweep(ctx, SWEEP_RHS, a);
        launch_landmarks(ctx, model, f->st, f->n_lm, f->lm_pid, f->lm_xyz, f->lm_cov, Gd, rhs);
        rc = check_launch(ctx);
        // the staging buffers and the host weights go out of scope
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = gingr_set_error(ctx, GINGR_ERR_HIP, "synchronize failed");
    }
    if (rc) {
        gingr_fitter_destroy(f);
        return rc;
    }
    *f_out = f;
    return GINGR_OK;
}

extern "C" {

int gingr_model_instance(gingr_ctx *ctx, const gingr_model *model, const double *alpha, const double euler[3],
                         const double center[3], const double translation[3], double scale, double *out_xyz) {
    if (!ctx || !model || !alpha || !euler || !center || !translation || !out_xyz) return GINGR_ERR_BAD_ARGUMENT;
    gingr_fitter *f = nullptr;
    // a non-finalized shard can still be instantiated: bypass the finalize check through a local flag
    gingr_model *mm = const_cast<gingr_model *>(model);
    const bool was = mm->finalized;
    mm->finalized = true;
    int rc = gingr_fitter_create(ctx, model, &f);
    mm->finalized = was;
    if (rc) return rc;
    gingr_state_scalars s;
    fill_scalars(&s, euler, center, translation, scale);
    rc = gingr_fitter_set_state(f, alpha, &s);
    if (!rc) rc = gingr_fitter_get_state(f, nullptr, nullptr, out_xyz);
    gingr_fitter_destroy(f);
    return rc;
}

int gingr_model_coefficients(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                             const double translation[3], const double *mesh_xyz, double *alpha) {
    if (!ctx || !model || !euler || !center || !translation || !mesh_xyz || !alpha) return GINGR_ERR_BAD_ARGUMENT;
    if (model->M != model->M_total)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "model_coefficients: single-shard models only");
    gingr_fitter *f = nullptr;
    GINGR_TRY(gingr_fitter_create(ctx, model, &f));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    int rc = GINGR_OK;
    std::vector<double> zero((size_t)r, 0.0);
    gingr_state_scalars s;
    fill_scalars(&s, euler, center, translation, 1.0);
    rc = gingr_fitter_set_state(f, zero.data(), &s);
    DevBuf aos, pose_h;
    if (!rc && aos.alloc((size_t)3 * M * sizeof(double)) != hipSuccess) rc = gingr_set_error(ctx, GINGR_ERR_HIP, "out of memory");
    if (!rc) {
        (void)hipMemcpyAsync(aos.p, mesh_xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        launch_aos_to_soa(ctx, aos.as<double>(), M, f->newshape, model->perm);
        // pose := the state's rigid transform
        DevState hst;
        (void)hipMemcpyAsync(&hst, f->st, sizeof(hst), hipMemcpyDeviceToHost, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        DevPose hp;
        memcpy(hp.R, hst.R, sizeof(hp.R));
        memcpy(hp.euler, hst.euler, sizeof(hp.euler));
        memcpy(hp.t, hst.t, sizeof(hp.t));
        memcpy(hp.center, hst.center, sizeof(hp.center));
        hp.scale = 1.0;
        (void)hipMemcpyAsync(f->pose, &hp, sizeof(hp), hipMemcpyHostToDevice, ctx->stream);
        SweepArgs a = base_args(f);
        a.shape_in = f->newshape;
        a.out = f->acoef;
        launch_sweep(ctx, SWEEP_PROJ2, a);
        launch_coeff_solve(ctx, r, rp, model->Binv, f->acoef, f->alpha_c);
        rc = check_launch(ctx);
        if (!rc && hipMemcpyAsync(alpha, f->alpha_c, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = gingr_set_error(ctx, GINGR_ERR_HIP, "copy failed");
        (void)hipStreamSynchronize(ctx->stream);
        if (!rc)
            for (int32_t k = 0; k < r; ++k)
                if (!std::isfinite(alpha[k])) {
                    rc = gingr_set_error(ctx, GINGR_ERR_NONFINITE, "model_coefficients: non-finite coefficient");
                    break;
                }
    }
    gingr_fitter_destroy(f);
    return rc;
}

int gingr_model_posterior_mean(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                               const double translation[3], const double *obs_xyz, const double *weight, int32_t n_lm,
                               const int32_t *lm_pid, const double *lm_xyz, const double *lm_cov, double *mean_xyz,
                               double *coeffs) {
    if (!ctx || !model || !euler || !center || !translation || !obs_xyz || !weight) return GINGR_ERR_BAD_ARGUMENT;
    if (model->M != model->M_total)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "model_posterior_mean: single-shard models only");
    gingr_fitter *f = nullptr;
    DevBuf G, aos;
    GINGR_TRY(model_observation_system(ctx, model, euler, center, translation, obs_xyz, weight, n_lm, lm_pid, lm_xyz, lm_cov, &f, G));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    int rc = GINGR_OK;
    if (aos.alloc((size_t)3 * M * sizeof(double)) != hipSuccess) rc = gingr_set_error(ctx, GINGR_ERR_HIP, "out of memory");
    if (!rc) {
        double *Gd = G.as<double>(), *rhs = Gd + (int64_t)rp * rp;
        launch_posterior_solve(ctx, r, rp, Gd, rhs, nullptr, f->work, f->acoef, f->st);
        SweepArgs b = base_args(f);
        b.coef0 = f->acoef;
        b.shape_out = f->newshape;
        launch_sweep(ctx, SWEEP_POSED, b);
        launch_soa_to_aos(ctx, f->newshape, M, aos.as<double>(), model->perm);
        rc = check_launch(ctx);
        DevState hst;
        (void)hipMemcpyAsync(&hst, f->st, sizeof(hst), hipMemcpyDeviceToHost, ctx->stream);
        if (mean_xyz) (void)hipMemcpyAsync(mean_xyz, aos.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (coeffs) (void)hipMemcpyAsync(coeffs, f->acoef, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = gingr_set_error(ctx, GINGR_ERR_HIP, "synchronize failed");
        if (!rc && hst.err) rc = gingr_set_error(ctx, hst.err, "model_posterior_mean: posterior solve failed (%s)",
                                                  hst.err == GINGR_ERR_NOT_SPD ? "not SPD" : "non-finite");
    }
    gingr_fitter_destroy(f);
    return rc;
}

int gingr_model_new_reference(gingr_ctx *ctx, const gingr_model *src, int64_t M_new, const double *new_ref,
                              const int32_t *vertex_ids, const double *weights, int64_t row_begin, int64_t row_end,
                              gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!src || !new_ref || !vertex_ids || !weights || M_new < 1)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_new_reference: bad argument");
    if (src->ctx != ctx || src->row_begin != 0 || src->row_end != src->M_total)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_new_reference: the source must be a complete model of this context");
    const int64_t Ms = src->M;
    for (int64_t k = 0; k < 3 * M_new; ++k)
        if (vertex_ids[k] < 0 || vertex_ids[k] >= Ms)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_new_reference: source vertex id out of range");
    if (row_end <= 0) row_end = M_new;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // mean displacement of the new points (host: 3 M_new values)
    std::vector<double> smean((size_t)3 * Ms), nmean((size_t)3 * M_new);
    GINGR_TRY(gingr_model_download(ctx, src, nullptr, smean.data(), nullptr, nullptr));
    for (int64_t i = 0; i < M_new; ++i)
        for (int d = 0; d < 3; ++d) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += weights[3 * i + k] * smean[(size_t)3 * vertex_ids[3 * i + k] + d];
            nmean[(size_t)3 * i + d] = acc;
        }
    DevBuf dids, dw, dinv;
    HIP_TRY(ctx, dids.alloc((size_t)3 * M_new * sizeof(int32_t)));
    HIP_TRY(ctx, dw.alloc((size_t)3 * M_new * sizeof(double)));
    HIP_TRY(ctx, dinv.alloc((size_t)Ms * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(dids.p, vertex_ids, (size_t)3 * M_new * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dw.p, weights, (size_t)3 * M_new * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dinv.p, src->hiperm.data(), (size_t)Ms * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    auto fill = [&](gingr_model *m) -> int {
        launch_interp_pack(ctx, src->Q0, src->rp, dinv.as<int32_t>(), dids.as<int32_t>(), dw.as<double>(), m->perm, m->row_begin, m->M,
                           m->Q0);
        return check_launch(ctx);
    };
    return model_create_impl(ctx, M_new, src->r, new_ref, nmean.data(), src->variance.data(), row_begin, row_end, fill, out);
}

int gingr_model_download(gingr_ctx *ctx, const gingr_model *m, double *ref, double *mean, double *basis_colmajor,
                         double *variance) {
    if (!ctx || !m) return GINGR_ERR_BAD_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = m->M;
    DevBuf aos, var, stage;
    HIP_TRY(ctx, aos.alloc((size_t)3 * M * sizeof(double)));
    if (ref) {
        launch_soa_to_aos(ctx, m->ref, M, aos.as<double>(), m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(ref, aos.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (mean) {
        launch_soa_to_aos(ctx, m->mean, M, aos.as<double>(), m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(mean, aos.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (variance) memcpy(variance, m->variance.data(), (size_t)m->r * sizeof(double));
    if (basis_colmajor) {
        HIP_TRY(ctx, var.alloc((size_t)m->r * sizeof(double)));
        HIP_TRY(ctx, stage.alloc((size_t)3 * M * m->r * sizeof(double)));
        HIP_TRY(ctx, hipMemcpyAsync(var.p, m->variance.data(), (size_t)m->r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        const int64_t total = 3 * M * m->r;
        hipLaunchKernelGGL(unpack_basis_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, m->Q0,
                           var.as<double>(), M, m->r, m->rp, m->perm, stage.as<double>());
        GINGR_TRY(check_launch(ctx));
        HIP_TRY(ctx, hipMemcpyAsync(basis_colmajor, stage.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GINGR_OK;
}

int gingr_model_truncate(gingr_ctx *ctx, const gingr_model *src, int32_t k, gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!src) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_truncate: no model");
    if (const char *fault = complete_model_fault(ctx, src))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT,
                               "model_truncate: the source %s; truncate a complete, finalized model of this context (or build the shard with keep_rank)", fault);
    if (k < 1 || k > src->r)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_truncate: k = %d outside 1..%d (the model's rank)", (int)k, (int)src->r);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = src->M;
    std::vector<double> href, hmean;
    GINGR_TRY(download_ref_mean(ctx, src, href, hmean));
    auto fill = [&](gingr_model *m) -> int {
        // the same points and mean give the same row order (Morton order of ref + mean): rows are copied in place
        if (m->M != M || m->hperm != src->hperm) return gingr_set_error(ctx, GINGR_ERR_STATE, "model_truncate: row order differs from the source's");
        const int64_t total = 3 * M * m->rp;
        hipLaunchKernelGGL(truncate_basis_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, src->Q0, src->rp, 3 * M, k, m->rp,
                           m->Q0);
        return check_launch(ctx);
    };
    // a kernel-built model stays one: the columns of its extension's coefficients are cut with the basis
    std::shared_ptr<KernelExtension> ext;
    GINGR_TRY(kernel_extension_truncate(ctx, src, k, &ext));
    GINGR_TRY(model_create_impl(ctx, src->M_total, k, href.data(), hmean.data(), src->variance.data(), 0, src->M_total, fill, out));
    (*out)->ext = ext;
    (*out)->ext_missing = src->ext_missing;
    return GINGR_OK;
}

}  // extern "C"
