// Per-vertex covariance maps of a low-rank model (C ABI in include/gingr_hip.h): for a right factor W [rp x rp]
//   C_i = (Q0_i W)(Q0_i W)^T,  Q0_i = the three basis rows of vertex i,
// rotated to R C_i R^T.  W = I is the prior marginal U_i diag(lambda) U_i^T; W = L^-T with L L^T = I + G is the posterior of a
// registration state (posterior.gp.cov(pid, pid) of scalismo; G/api/GingrAlgorithm.scala:297-301).  The factored form keeps every
// block positive semi-definite by construction and never forms (I + G)^-1, whose error relative to a small posterior block grows
// with cond(I + G).
#include "dense_spd.h"
#include "fitter.h"

#include <algorithm>
#include <cmath>

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));

// Rot3 (fitter.h): row-major; the kernels here read the rotation from `state` instead when that is given

constexpr int kCovWaves = 8;      // waves per workgroup, each with 16 vertices of its own (no LDS, no barrier); two per SIMD keep the
                                  // 96 accumulator registers in VGPRs (four waves: the compiler moves them through AGPRs every step)
constexpr int kCovVerts = 16;     // vertices per wave = rows of one MFMA tile
constexpr int kCovChunkTiles = 4; // column tiles of Y a wave holds at a time (3 x 4 accumulator tiles = 96 registers)

// One column chunk [n0, n0 + 16 NT) of Y = Q0_rows W for the wave's 16 vertices, reduced into the six running sums at once.
//   D(16x16) += A(16x4) B(4x16): lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D: lane holds column
//   j = l & 15 of the rows i = (l >> 4) + 4 reg (the layouts of gram_kernel, gp_gram.hip).
// Row tile d holds coordinate d of the 16 vertices (A row i = basis row 3 (v0 + i) + d), so the three coordinates of a vertex sit in
// the same lane and register of the three tiles and Y_d Y_e needs no exchange.  The 16 k of a step are dealt to the four MFMAs as
// k0 + 4 (l >> 4) + t: a lane's four A values are 32 contiguous bytes (one load), and B follows the same permutation of k.
// k_end: columns of W at and past n0 + 16 NT only (upper triangular W: the rows past the chunk's last column are zero).
template <int NT>
__device__ __forceinline__ void cov_chunk(const double *__restrict__ qrow, int rp, const double *__restrict__ W, int64_t ldw, int n0, int k_end,
                                          int kq, int cl, double (&s)[4][6]) {
    v4f64 acc[3][NT];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[d][j] = v4f64{0, 0, 0, 0};
    const double *wcol = W + (int64_t)(4 * kq) * ldw + n0 + cl;
    for (int k0 = 0; k0 < k_end; k0 += 16) {
        d4 a[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = *reinterpret_cast<const d4 *>(qrow + (int64_t)d * rp + k0 + 4 * kq);
        double b[4][NT];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < NT; ++j) b[t][j] = wcol[(int64_t)(k0 + t) * ldw + 16 * j];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[d][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[d][t], b[t][j], acc[d][j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double x = acc[0][j][g], y = acc[1][j][g], z = acc[2][j][g];
            s[g][0] = __builtin_fma(x, x, s[g][0]);
            s[g][1] = __builtin_fma(x, y, s[g][1]);
            s[g][2] = __builtin_fma(x, z, s[g][2]);
            s[g][3] = __builtin_fma(y, y, s[g][3]);
            s[g][4] = __builtin_fma(y, z, s[g][4]);
            s[g][5] = __builtin_fma(z, z, s[g][5]);
        }
}

// cov6[perm[s]] = the six unique entries {xx, xy, xz, yy, yz, zz} of R (Q0_s W)(Q0_s W)^T R^T for the device rows s < M.
// Q0 has kBasisRowSlack zero rows behind row 3 M: a wave whose first vertex exists reads at most 47 of them.
__global__ __launch_bounds__(64 * kCovWaves) void marginal_cov_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ W,
                                                                      int64_t ldw, int upper, Rot3 rot, const DevState *__restrict__ state,
                                                                      const int32_t *__restrict__ perm, double *__restrict__ cov6) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t v0 = ((int64_t)blockIdx.x * kCovWaves + wave) * kCovVerts;
    if (v0 >= M) return;
    const double *qrow = Q0 + 3 * (v0 + cl) * (int64_t)rp;
    double s[4][6];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < 6; ++q) s[g][q] = 0.0;
    const int nt = rp / 16;
    int t0 = 0;
    for (; t0 + kCovChunkTiles <= nt; t0 += kCovChunkTiles)
        cov_chunk<kCovChunkTiles>(qrow, rp, W, ldw, 16 * t0, upper ? 16 * (t0 + kCovChunkTiles) : rp, kq, cl, s);
    const int k_end = upper ? 16 * nt : rp;
    switch (nt - t0) {
        case 1: cov_chunk<1>(qrow, rp, W, ldw, 16 * t0, k_end, kq, cl, s); break;
        case 2: cov_chunk<2>(qrow, rp, W, ldw, 16 * t0, k_end, kq, cl, s); break;
        case 3: cov_chunk<3>(qrow, rp, W, ldw, 16 * t0, k_end, kq, cl, s); break;
        default: break;
    }
    // the sums over the 16 columns a row of lanes holds (same order in every lane: all of them end with the total)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double v = s[g][q];
            v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 1);
            s[g][q] = v;
        }
    // lane cl < 4 of row kq writes vertex kq + 4 cl (register cl)
    if (cl >= 4) return;
    double c[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) c[q] = cl == 0 ? s[0][q] : (cl == 1 ? s[1][q] : (cl == 2 ? s[2][q] : s[3][q]));
    const int64_t v = v0 + kq + 4 * cl;
    if (v >= M) return;
    const double *R = state ? state->R : rot.R;
    const double C[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    double T[3][3];  // R C
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i][j] = (R[3 * i] * C[0][j] + R[3 * i + 1] * C[1][j]) + R[3 * i + 2] * C[2][j];
    double *out = cov6 + 6 * (int64_t)perm[v];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) out[q++] = (T[i][0] * R[3 * j] + T[i][1] * R[3 * j + 1]) + T[i][2] * R[3 * j + 2];
}

// ---- cross-covariance with one point p: cov9[i] = R (Q0_i W)(Q0_p W)^T R^T = R Q0_i Z R^T with Z = W (Q0_p W)^T [rp x 3]
// Z first (one workgroup: y = Q0_p W, then z = W y^T), then one pass with 16 lanes per vertex: GEMV-shaped, no MFMA.
__global__ __launch_bounds__(256) void cross_vector_kernel(const double *__restrict__ Qp, int rp, const double *__restrict__ W, int64_t ldw,
                                                           double *__restrict__ Z) {
    __shared__ double y[3][512];
    const int tid = threadIdx.x;
    for (int j = tid; j < rp; j += 256) {  // y[d][j] = sum_k Q0[3p + d][k] W[k][j]: consecutive threads, consecutive columns
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < rp; ++k) {
            const double w = W[(int64_t)k * ldw + j];
            a0 = __builtin_fma(Qp[k], w, a0);
            a1 = __builtin_fma(Qp[rp + k], w, a1);
            a2 = __builtin_fma(Qp[2 * rp + k], w, a2);
        }
        y[0][j] = a0, y[1][j] = a1, y[2][j] = a2;
    }
    __syncthreads();
    const int l16 = tid & 15;
    for (int k = tid >> 4; k < rp; k += 16) {  // z[k][e] = sum_j W[k][j] y[e][j]: 16 lanes per row of W
        double a[3] = {0.0, 0.0, 0.0};
        for (int j = l16; j < rp; j += 16) {
            const double w = W[(int64_t)k * ldw + j];
            a[0] = __builtin_fma(w, y[0][j], a[0]);
            a[1] = __builtin_fma(w, y[1][j], a[1]);
            a[2] = __builtin_fma(w, y[2][j], a[2]);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            a[e] += __shfl_xor(a[e], 8);
            a[e] += __shfl_xor(a[e], 4);
            a[e] += __shfl_xor(a[e], 2);
            a[e] += __shfl_xor(a[e], 1);
        }
        if (l16 == 0) Z[3 * k] = a[0], Z[3 * k + 1] = a[1], Z[3 * k + 2] = a[2];
    }
}

__global__ __launch_bounds__(256) void cross_cov_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ Z, Rot3 rot,
                                                        const int32_t *__restrict__ perm, double *__restrict__ cov9) {
    const int l16 = threadIdx.x & 15;
    const int64_t v = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (v >= M) return;  // (whole groups of 16 lanes leave together: the shuffles below stay inside a group)
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double *q = Q0 + 3 * v * (int64_t)rp;
    for (int k = l16; k < rp; k += 16) {
        const double z0 = Z[3 * k], z1 = Z[3 * k + 1], z2 = Z[3 * k + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = q[(int64_t)d * rp + k];
            c[3 * d] = __builtin_fma(a, z0, c[3 * d]);
            c[3 * d + 1] = __builtin_fma(a, z1, c[3 * d + 1]);
            c[3 * d + 2] = __builtin_fma(a, z2, c[3 * d + 2]);
        }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        c[e] += __shfl_xor(c[e], 8);
        c[e] += __shfl_xor(c[e], 4);
        c[e] += __shfl_xor(c[e], 2);
        c[e] += __shfl_xor(c[e], 1);
    }
    if (l16 != 0) return;
    const double *R = rot.R;
    double T[9];  // R C
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[3 * i + j] = (R[3 * i] * c[j] + R[3 * i + 1] * c[3 + j]) + R[3 * i + 2] * c[6 + j];
    double *out = cov9 + 9 * (int64_t)perm[v];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (T[3 * i] * R[3 * j] + T[3 * i + 1] * R[3 * j + 1]) + T[3 * i + 2] * R[3 * j + 2];
}

// W [rp x rp] of a model operator: the caller's r x r factor zero padded, or the identity
__global__ __launch_bounds__(256) void pad_factor_kernel(int r, int rp, const double *__restrict__ factor, double *__restrict__ W) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rp * rp) return;
    const int row = idx / rp, c = idx - row * rp;
    double v = 0.0;
    if (row < r && c < r) v = factor ? factor[(int64_t)row * r + c] : (row == c ? 1.0 : 0.0);
    W[idx] = v;
}

struct FactorBufs {  // device copy of a model operator's factor
    DevBuf host_factor, W;
};

// W of a model operator on the device: [rp x rp], row stride rp
int upload_factor(gingr_ctx *ctx, const gingr_model *m, const double *factor, FactorBufs &b) {
    const int32_t r = m->r, rp = m->rp;
    if (b.W.alloc((size_t)rp * rp * sizeof(double)) != hipSuccess) return gingr_set_error(ctx, GINGR_ERR_HIP, "covariance: out of device memory");
    if (factor) {
        if (b.host_factor.alloc((size_t)r * r * sizeof(double)) != hipSuccess)
            return gingr_set_error(ctx, GINGR_ERR_HIP, "covariance: out of device memory");
        HIP_TRY(ctx, hipMemcpyAsync(b.host_factor.p, factor, (size_t)r * r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(pad_factor_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp, 256)), dim3(256), 0, ctx->stream, (int)r, (int)rp,
                       factor ? b.host_factor.as<double>() : nullptr, b.W.as<double>());
    return GINGR_OK;
}

Rot3 rot_of_euler(const double euler[3]) {
    Rot3 rot;
    euler_to_rot(euler, rot.R);
    return rot;
}

}  // namespace

void launch_marginal_covariance(gingr_ctx *ctx, const gingr_model *m, const double *W, int64_t ldw, bool upper, const double R[9],
                                const DevState *state, double *cov6) {
    Rot3 rot;
    for (int q = 0; q < 9; ++q) rot.R[q] = R ? R[q] : (q % 4 == 0 ? 1.0 : 0.0);
    const int64_t blocks = ceil_div(m->M, (int64_t)kCovWaves * kCovVerts);
    TimerScope ts(ctx, 9);
    hipLaunchKernelGGL(marginal_cov_kernel, dim3((unsigned)blocks), dim3(64 * kCovWaves), 0, ctx->stream, m->Q0, m->M, (int)m->rp, W, ldw,
                       upper ? 1 : 0, rot, state, m->perm, cov6);
}

void launch_cross_covariance(gingr_ctx *ctx, const gingr_model *m, const double *W, int64_t ldw, const double R[9], int64_t device_row,
                             double *Z, double *cov9) {
    Rot3 rot;
    for (int q = 0; q < 9; ++q) rot.R[q] = R ? R[q] : (q % 4 == 0 ? 1.0 : 0.0);
    hipLaunchKernelGGL(cross_vector_kernel, dim3(1), dim3(256), 0, ctx->stream, m->Q0 + 3 * device_row * (int64_t)m->rp, (int)m->rp, W, ldw, Z);
    hipLaunchKernelGGL(cross_cov_kernel, dim3((unsigned)ceil_div(m->M, 16)), dim3(256), 0, ctx->stream, m->Q0, m->M, (int)m->rp, Z, rot, m->perm,
                       cov9);
}

int64_t posterior_factor_work_doubles(int32_t rp) {
    return DenseSpdWork::doubles(rp, DenseSpdWork::kIdentity);  // the system over the identity, the inverses of the diagonal blocks, the flag
}

const double *launch_posterior_factor(gingr_ctx *ctx, int32_t r, int32_t rp, const double *G, double *work, int64_t *ldw, int32_t **flag) {
    // Aw: the lower triangle of I + G (identity on the padding) on top of the identity the blocked Cholesky turns into L^-T
    const DenseSpdWork ws(rp, DenseSpdWork::kIdentity);
    double *Aw = work + ws.aw(), *Linv = work + ws.linv();
    *flag = reinterpret_cast<int32_t *>(work + ws.flag());
    *ldw = ws.Mp;
    launch_spd_system(ctx->stream, (int)r, ws, SpdIdentityPlus{G, (int)rp}, SpdIdentityBorder{}, Aw, *flag);
    dense_spd_inverse(ctx, Aw, ws.Mp, Linv, nullptr, *flag);
    return work + ws.lt();
}

extern "C" {

int gingr_model_marginal_covariance(gingr_ctx *ctx, const gingr_model *model, const double *factor, const double euler[3], double *cov6_out) {
    if (!ctx || !model || !euler || !cov6_out) return GINGR_ERR_BAD_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = model->M;
    FactorBufs fb;
    DevBuf out;
    GINGR_TRY(upload_factor(ctx, model, factor, fb));
    if (out.alloc((size_t)6 * M * sizeof(double)) != hipSuccess) return gingr_set_error(ctx, GINGR_ERR_HIP, "marginal_covariance: out of device memory");
    const Rot3 rot = rot_of_euler(euler);
    launch_marginal_covariance(ctx, model, fb.W.as<double>(), model->rp, factor == nullptr, rot.R, nullptr, out.as<double>());
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(cov6_out, out.p, (size_t)6 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_model_cross_covariance(gingr_ctx *ctx, const gingr_model *model, const double *factor, const double euler[3], int64_t pid,
                                 double *cov9_out) {
    if (!ctx || !model || !euler || !cov9_out) return GINGR_ERR_BAD_ARGUMENT;
    if (pid < 0 || pid >= model->M_total) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cross_covariance: pid outside the model");
    if (pid < model->row_begin || pid >= model->row_end)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "cross_covariance: this row shard does not own point %lld", (long long)pid);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = model->M;
    FactorBufs fb;
    DevBuf out, Z;
    GINGR_TRY(upload_factor(ctx, model, factor, fb));
    if (out.alloc((size_t)9 * M * sizeof(double)) != hipSuccess || Z.alloc((size_t)3 * model->rp * sizeof(double)) != hipSuccess)
        return gingr_set_error(ctx, GINGR_ERR_HIP, "cross_covariance: out of device memory");
    const Rot3 rot = rot_of_euler(euler);
    const int64_t device_row = model->hiperm[(size_t)(pid - model->row_begin)];
    launch_cross_covariance(ctx, model, fb.W.as<double>(), model->rp, rot.R, device_row, Z.as<double>(), out.as<double>());
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(cov9_out, out.p, (size_t)9 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

// posterior(of the current state).gp.cov(pid, pid) for every vertex: built like posterior_logpdf (fitter_mh.hip) -- phases 0 and 1
// of the state (they do not touch it; landmarks are in G already), the factor of I + G, one pass over the basis with the state's
// rotation.  The posterior is that of model.transform(rigid) (GingrAlgorithm.scala:297-301): no scale.
static int posterior_covariance(gingr_fitter *f, const Correspondence &c, double *cov6_out) {
    GINGR_TRY(check_correspondence(f, c));
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (!cov6_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "posterior_covariance: null argument");
    if (m->M != m->M_total || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "posterior_covariance: single shard only");
    const int64_t M = m->M;
    GINGR_TRY(fitter_posterior_inputs(f, c));
    HIP_TRY(ctx, ensure(f->cov_work, (size_t)posterior_factor_work_doubles(m->rp) * sizeof(double)));
    HIP_TRY(ctx, ensure(f->cov_out, (size_t)6 * M * sizeof(double)));
    int64_t ldw = 0;
    int32_t *flag = nullptr;
    const double *W = launch_posterior_factor(ctx, m->r, m->rp, f->seg1_live(), f->cov_work.as<double>(), &ldw, &flag);
    launch_marginal_covariance(ctx, m, W, ldw, true, nullptr, f->st, f->cov_out.as<double>());
    GINGR_TRY(check_launch(ctx));
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cov6_out, f->cov_out.p, (size_t)6 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "posterior_covariance: posterior of the current state failed");
    for (int64_t i = 0; i < 6 * M; ++i)
        if (!std::isfinite(cov6_out[i])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "posterior_covariance: non-finite result");
    return GINGR_OK;
}

int gingr_fitter_posterior_covariance_cpd(gingr_fitter *f, const gingr_cpd_params *p, double *cov6_out) {
    return posterior_covariance(f, abi_correspondence(0, p, nullptr), cov6_out);
}
int gingr_fitter_posterior_covariance_icp(gingr_fitter *f, const gingr_icp_params *p, double *cov6_out) {
    return posterior_covariance(f, abi_correspondence(1, nullptr, p), cov6_out);
}
int gingr_fitter_posterior_covariance_icp_surface(gingr_fitter *f, const gingr_icp_params *p, double *cov6_out) {
    return posterior_covariance(f, abi_correspondence(2, nullptr, p), cov6_out);
}
int gingr_fitter_posterior_covariance_pairs(gingr_fitter *f, double *cov6_out) {
    return posterior_covariance(f, abi_correspondence(3, nullptr, nullptr), cov6_out);
}

}  // extern "C"
