// Observations of the GiNGR update (CPD, ICP, given points) and landmarks, one thread per model point (gfx950, MI355X).
#include "gp.h"
#include "svd3.h"

namespace {

__global__ void centered_mean_kernel(const double *__restrict__ ref, const double *__restrict__ mean, int64_t M, double c0x,
                                     double c0y, double c0z, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    out[i] = ref[i] + mean[i] - c0x;
    out[M + i] = ref[M + i] + mean[M + i] - c0y;
    out[2 * M + i] = ref[2 * M + i] + mean[2 * M + i] - c0z;
}

// ------------------------------------------------------------------------------------------------- observations
__global__ void obs_cpd_kernel(const double *__restrict__ ref, const double *__restrict__ mean, int64_t M,
                               const DevState *__restrict__ st, Cloud fit, const double *__restrict__ P1,
                               const double *__restrict__ PX, double lambda, const int32_t *__restrict__ lm_mask,
                               double *__restrict__ weight, double *__restrict__ evec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (lm_mask && lm_mask[i]) {  // point overridden by a landmark observation (GingrAlgorithm.scala:289-292)
        weight[i] = 0.0;
        evec[i] = evec[M + i] = evec[2 * M + i] = 0.0;
        return;
    }
    const double p1inv = 1.0 / P1[i];                         // CPD.scala:37
    const double yx = fit.x[i], yy = fit.y[i], yz = fit.z[i];
    // td = y + (sum_j P1inv*P_ij*x_j - y)                     CPD.scala:44-46
    const double ox = yx + (PX[i] * p1inv - yx), oy = yy + (PX[M + i] * p1inv - yy), oz = yz + (PX[2 * M + i] * p1inv - yz);
    const double var = st->sigma2 * lambda * p1inv;           // CPD.scala:126
    const double w = 1.0 / var;
    const double *R = st->R;
    const double dx = ox - st->center[0] - st->t[0], dy = oy - st->center[1] - st->t[1], dz = oz - st->center[2] - st->t[2];
    const double ex = R[0] * dx + R[3] * dy + R[6] * dz - (ref[i] - st->center[0]) - mean[i];
    const double ey = R[1] * dx + R[4] * dy + R[7] * dz - (ref[M + i] - st->center[1]) - mean[M + i];
    const double ez = R[2] * dx + R[5] * dy + R[8] * dz - (ref[2 * M + i] - st->center[2]) - mean[2 * M + i];
    weight[i] = w;
    evec[i] = w * ex;
    evec[M + i] = w * ey;
    evec[2 * M + i] = w * ez;
}

// obs point given explicitly (planes ox/oy/oz), weight given or derived from sigma2 (ICP)
__global__ void obs_points_kernel(const double *__restrict__ ref, const double *__restrict__ mean, int64_t M,
                                  const DevState *__restrict__ st, const double *__restrict__ obs, Cloud target,
                                  const int32_t *__restrict__ idx, const double *__restrict__ weight_in,
                                  const int32_t *__restrict__ lm_mask, double *__restrict__ weight,
                                  double *__restrict__ evec, int32_t *__restrict__ zero_counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (zero_counts) {  // the zero-weight vertices of this block (ZeroGate::counts); the same test as below
        const bool zero = i < M && ((lm_mask && lm_mask[i]) || (idx ? 1.0 / st->sigma2 : weight_in[i]) == 0.0);
        const int cnt = __syncthreads_count(zero);
        if (threadIdx.x == 0) zero_counts[blockIdx.x] = cnt;
    }
    if (i >= M) return;
    double w;
    double ox, oy, oz;
    if (idx) {  // ICP: closest target point, cov = I3 * sigma2 (ICP.scala:90-92)
        const int32_t j = idx[i];
        if (j >= 0 && (int64_t)j < target.n) {
            ox = target.x[j];
            oy = target.y[j];
            oz = target.z[j];
        } else {  // the searches leave -1 when no distance is finite: a NaN observation fails the posterior through the status path
            ox = oy = oz = __builtin_nan("");
        }
        w = 1.0 / st->sigma2;
    } else {
        ox = obs[i];
        oy = obs[M + i];
        oz = obs[2 * M + i];
        w = weight_in[i];
    }
    if ((lm_mask && lm_mask[i]) || w == 0.0) {
        weight[i] = 0.0;
        evec[i] = evec[M + i] = evec[2 * M + i] = 0.0;
        return;
    }
    const double *R = st->R;
    const double dx = ox - st->center[0] - st->t[0], dy = oy - st->center[1] - st->t[1], dz = oz - st->center[2] - st->t[2];
    const double ex = R[0] * dx + R[3] * dy + R[6] * dz - (ref[i] - st->center[0]) - mean[i];
    const double ey = R[1] * dx + R[4] * dy + R[7] * dz - (ref[M + i] - st->center[1]) - mean[M + i];
    const double ez = R[2] * dx + R[5] * dy + R[8] * dz - (ref[2 * M + i] - st->center[2]) - mean[2 * M + i];
    weight[i] = w;
    evec[i] = w * ex;
    evec[M + i] = w * ey;
    evec[2 * M + i] = w * ez;
}

// Landmark observations with a full 3x3 covariance: QtL block = Q_p^T Sigma^-1 in the posed frame, i.e.
// W = R^T Sigma^-1 R in the model frame.  Workgroup a < rp owns row a of G, workgroup rp owns rhs; every entry sums
// its landmarks in registers in landmark order and touches G once (the per-landmark read-modify-write of one
// workgroup cost 16 us a landmark).  The 3x3 algebra of a landmark is repeated by one lane of every workgroup.
constexpr int kLmChunk = 256;
__global__ __launch_bounds__(kLmChunk) void landmarks_kernel(const double *__restrict__ Q0, const double *__restrict__ ref,
                                                             const double *__restrict__ mean, int64_t M, int rp,
                                                             const DevState *__restrict__ st, int n_lm,
                                                             const int32_t *__restrict__ pid,
                                                             const double *__restrict__ xyz,
                                                             const double *__restrict__ cov, double *__restrict__ G,
                                                             double *__restrict__ rhs) {
    __shared__ double u[kLmChunk][3];  // row a: sum_d q[d][a] W[d][.]   |   rhs workgroup: W v
    __shared__ int32_t row[kLmChunk];
    const int a = blockIdx.x;
    const bool is_rhs = a == rp;
    constexpr int kCols = 2;  // columns per lane and pass (ranks up to 512 in one pass)
    for (int b0 = 0; b0 < rp; b0 += kCols * kLmChunk) {
        double s[kCols];
        for (int c = 0; c < kCols; ++c) s[c] = 0.0;
        for (int l0 = 0; l0 < n_lm; l0 += kLmChunk) {
            __syncthreads();
            const int l = l0 + (int)threadIdx.x;
            int32_t p = l < n_lm ? pid[l] : -1;
            if (p < 0 || p >= M) p = -1;  // owned by another shard
            double o0 = 0.0, o1 = 0.0, o2 = 0.0;
            if (p >= 0) {
                const double *C = cov + 9 * (int64_t)l;
                double Ci[9];
                spd3_inverse(C, Ci);  // NaNs for a matrix that is no covariance: the solve then fails by the status path
                const double *R = st->R;
                double T[9], W[9];  // T = Ci * R
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j)
                        T[i * 3 + j] = Ci[i * 3] * R[j] + Ci[i * 3 + 1] * R[3 + j] + Ci[i * 3 + 2] * R[6 + j];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) W[i * 3 + j] = R[i] * T[j] + R[3 + i] * T[3 + j] + R[6 + i] * T[6 + j];
                if (is_rhs) {
                    const double dx = xyz[3 * l] - st->center[0] - st->t[0], dy = xyz[3 * l + 1] - st->center[1] - st->t[1],
                                 dz = xyz[3 * l + 2] - st->center[2] - st->t[2];
                    double v[3];
                    v[0] = R[0] * dx + R[3] * dy + R[6] * dz - (ref[p] - st->center[0]) - mean[p];
                    v[1] = R[1] * dx + R[4] * dy + R[7] * dz - (ref[M + p] - st->center[1]) - mean[M + p];
                    v[2] = R[2] * dx + R[5] * dy + R[8] * dz - (ref[2 * M + p] - st->center[2]) - mean[2 * M + p];
                    o0 = W[0] * v[0] + W[1] * v[1] + W[2] * v[2];
                    o1 = W[3] * v[0] + W[4] * v[1] + W[5] * v[2];
                    o2 = W[6] * v[0] + W[7] * v[1] + W[8] * v[2];
                } else {
                    const double *q = Q0 + (int64_t)3 * p * rp + a;
                    const double q0 = q[0], q1 = q[rp], q2 = q[2 * rp];
                    o0 = q0 * W[0] + q1 * W[3] + q2 * W[6];
                    o1 = q0 * W[1] + q1 * W[4] + q2 * W[7];
                    o2 = q0 * W[2] + q1 * W[5] + q2 * W[8];
                }
            }
            u[threadIdx.x][0] = o0;
            u[threadIdx.x][1] = o1;
            u[threadIdx.x][2] = o2;
            row[threadIdx.x] = p;
            __syncthreads();
            const int nl = min(kLmChunk, n_lm - l0);
            for (int k = 0; k < nl; ++k) {
                const int32_t pk = row[k];
                if (pk < 0) continue;
                const double *q = Q0 + (int64_t)3 * pk * rp;
                const double u0 = u[k][0], u1 = u[k][1], u2 = u[k][2];
#pragma unroll
                for (int c = 0; c < kCols; ++c) {
                    const int b = b0 + c * kLmChunk + (int)threadIdx.x;
                    if (b < rp) s[c] += u0 * q[b] + u1 * q[rp + b] + u2 * q[2 * rp + b];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int b = b0 + c * kLmChunk + (int)threadIdx.x;
            if (b < rp) {
                if (is_rhs)
                    rhs[b] += s[c];
                else
                    G[(int64_t)a * rp + b] += s[c];
            }
        }
    }
}

}  // namespace

void launch_centered_mean(gingr_ctx *ctx, const gingr_model *m, double *ptil) {
    hipLaunchKernelGGL(centered_mean_kernel, dim3((unsigned)ceil_div(m->M, 256)), dim3(256), 0, ctx->stream, m->ref, m->mean,
                       m->M, m->c0[0], m->c0[1], m->c0[2], ptil);
}

void launch_obs_cpd(gingr_ctx *ctx, const gingr_model *m, const DevState *st, Cloud fit, const double *P1,
                    const double *PX, double lambda, const int32_t *lm_mask, double *weight, double *evec) {
    hipLaunchKernelGGL(obs_cpd_kernel, dim3((unsigned)ceil_div(m->M, 256)), dim3(256), 0, ctx->stream, m->ref, m->mean, m->M,
                       st, fit, P1, PX, lambda, lm_mask, weight, evec);
}

void launch_obs_icp(gingr_ctx *ctx, const gingr_model *m, const DevState *st, Cloud target, const int32_t *idx,
                    const int32_t *lm_mask, double *weight, double *evec) {
    hipLaunchKernelGGL(obs_points_kernel, dim3((unsigned)ceil_div(m->M, 256)), dim3(256), 0, ctx->stream, m->ref, m->mean,
                       m->M, st, (const double *)nullptr, target, idx, (const double *)nullptr, lm_mask, weight, evec, (int32_t *)nullptr);
}

void launch_obs_points(gingr_ctx *ctx, const gingr_model *m, const DevState *st, const double *obs_soa,
                       const double *weight_in, double *weight, double *evec, const int32_t *lm_mask, int32_t *zero_counts) {
    Cloud none{nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(obs_points_kernel, dim3((unsigned)ceil_div(m->M, 256)), dim3(256), 0, ctx->stream, m->ref, m->mean,
                       m->M, st, obs_soa, none, (const int32_t *)nullptr, weight_in, lm_mask, weight, evec, zero_counts);
}

void launch_landmarks(gingr_ctx *ctx, const gingr_model *m, const DevState *st, int32_t n_lm, const int32_t *lm_pid_local,
                      const double *lm_xyz, const double *lm_cov, double *G, double *rhs) {
    if (n_lm <= 0) return;
    hipLaunchKernelGGL(landmarks_kernel, dim3((unsigned)m->rp + 1), dim3(kLmChunk), 0, ctx->stream, m->Q0, m->ref, m->mean, m->M, (int)m->rp, st,
                       (int)n_lm, lm_pid_local, lm_xyz, lm_cov, G, rhs);
}
