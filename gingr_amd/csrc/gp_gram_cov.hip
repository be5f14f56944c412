// The 3 x 3-weighted Gram pass of the GiNGR update (gfx950, MI355X): one observation with a full covariance per vertex,
//     G   += sum_i Q_i^T W_i Q_i,      W_i = R^T Lambda_i R                 (Q_i: the 3 x rp block of vertex i in Q0)
//     rhs += sum_i Q_i^T W_i v_i,      v_i = R^T (xbar_i - c - t) - m_i
// with Lambda_i / xbar_i the consolidated precision and point of the vertex (fitter_pairs.hip: gingr_fitter_set_pairs_cov_dense).
//
//   cov_obs_kernel          per vertex: W_i, its upper Cholesky factor C_i (W_i = C_i^T C_i) and W_i v_i; zero rows for a vertex
//                           without pairs or one a landmark overrides -- the sibling of obs_points_kernel (gp_obs.hip)
//   gram_cov_kernel         G = sum_i (C_i Q_i)^T (C_i Q_i) is a symmetric product: float64 MFMA (v_mfma_f64_16x16x4_f64) over row
//                           slabs, 64 x 64 patches of the upper triangle; one transformed fragment serves both operands
//   gram_cov_reduce_kernel  slab partials added up in a fixed order and ADDED to G and rhs (the isotropic pass and the phase-1
//                           finalize kernel in front have written them; the landmark pass behind adds its own)
// No atomics; every sum has a fixed order, so two runs give the same bits.  The decisions are in gram_cov_plan.h.
#include "gp.h"
#include "gp_device.h"
#include "gram_cov_plan.h"

namespace {

// fac: planes [9][M] = {c00, c01, c02, c11, c12, c22, g0, g1, g2}, C upper triangular with W = C^T C, g = W v.
// A precision that is not finite or not positive definite (the consolidation passes on what spd3_inverse made of a matrix that is no
// covariance) gives NaN rows: the posterior then fails by the status path, as the landmark pass's does.
__global__ __launch_bounds__(256) void cov_obs_kernel(const double *__restrict__ ref, const double *__restrict__ mean, int64_t M,
                                                      const DevState *__restrict__ st, const double *__restrict__ obs,
                                                      const double *__restrict__ prec6, const int32_t *__restrict__ lm_mask,
                                                      double *__restrict__ fac) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double lxx = prec6[i], lxy = prec6[M + i], lxz = prec6[2 * M + i], lyy = prec6[3 * M + i], lyz = prec6[4 * M + i],
                 lzz = prec6[5 * M + i];
    const bool none = lxx == 0.0 && lxy == 0.0 && lxz == 0.0 && lyy == 0.0 && lyz == 0.0 && lzz == 0.0;
    if ((lm_mask && lm_mask[i]) || none) {
#pragma unroll
        for (int k = 0; k < 9; ++k) fac[k * M + i] = 0.0;
        return;
    }
    const double *R = st->R;
    const double L[9] = {lxx, lxy, lxz, lxy, lyy, lyz, lxz, lyz, lzz};
    double T[9];  // T = Lambda R
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) T[a * 3 + b] = L[a * 3] * R[b] + L[a * 3 + 1] * R[3 + b] + L[a * 3 + 2] * R[6 + b];
    double W[9];  // upper triangle of R^T T, mirrored: exactly symmetric
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) W[a * 3 + b] = W[b * 3 + a] = R[a] * T[b] + R[3 + a] * T[3 + b] + R[6 + a] * T[6 + b];
    const double dx = obs[i] - st->center[0] - st->t[0], dy = obs[M + i] - st->center[1] - st->t[1],
                 dz = obs[2 * M + i] - st->center[2] - st->t[2];
    const double v0 = R[0] * dx + R[3] * dy + R[6] * dz - (ref[i] - st->center[0]) - mean[i];
    const double v1 = R[1] * dx + R[4] * dy + R[7] * dz - (ref[M + i] - st->center[1]) - mean[M + i];
    const double v2 = R[2] * dx + R[5] * dy + R[8] * dz - (ref[2 * M + i] - st->center[2]) - mean[2 * M + i];
    const double kMax = 1.79769313486231570815e308;
    bool ok = W[0] > 0.0 && W[0] <= kMax;
    const double c00 = sqrt(W[0]);
    const double c01 = W[1] / c00, c02 = W[2] / c00;
    const double p1 = W[4] - c01 * c01;
    ok = ok && p1 > 0.0 && p1 <= kMax;
    const double c11 = sqrt(p1);
    const double c12 = (W[5] - c01 * c02) / c11;
    const double p2 = (W[8] - c02 * c02) - c12 * c12;
    ok = ok && p2 > 0.0 && p2 <= kMax;
    const double c22 = sqrt(p2);
    const double nan = __builtin_nan("");
    fac[i] = ok ? c00 : nan;
    fac[M + i] = ok ? c01 : nan;
    fac[2 * M + i] = ok ? c02 : nan;
    fac[3 * M + i] = ok ? c11 : nan;
    fac[4 * M + i] = ok ? c12 : nan;
    fac[5 * M + i] = ok ? c22 : nan;
    fac[6 * M + i] = ok ? W[0] * v0 + W[1] * v1 + W[2] * v2 : nan;
    fac[7 * M + i] = ok ? W[3] * v0 + W[4] * v1 + W[5] * v2 : nan;
    fac[8 * M + i] = ok ? W[6] * v0 + W[7] * v1 + W[8] * v2 : nan;
}

// A workgroup of 4 waves computes one 64 x 64 patch (4 x 4 MFMA tiles) of G over one slab of vertices, as gram_kernel (gp_gram.hip)
// does over a slab of rows -- same fragment layout, same column interleave, same output layout.  A K-step is four vertices: lane
// group kq = l >> 4 owns vertex v + kq and loads its three basis rows at the columns {p*64 + 4*(l & 15) + t}, t < 4 (three 128-byte
// row segments per sixteen lanes and side), forms the three rows of C Q in registers -- six multiply-adds per column,
//     y0 = c00 q0 + c01 q1 + c02 q2,   y1 = c11 q1 + c12 q2,   y2 = c22 q2
// -- and feeds row d to the d-th of three MFMA steps at k index kq:
//     D(16x16) += A(16x4) B(4x16),  A[i][k] = y_d(vertex k)[a0 + i],  B[k][j] = y_d(vertex k)[b0 + j]
// No cross-lane traffic: the vertex's six factor entries are the same address for the sixteen lanes of a group.  On a diagonal patch
// one transformed fragment serves both operands.  The right-hand side sum_i Q_i^T g_i rides along in the workgroups of patch row 0
// (they cover every column block once) from the untransformed B-side rows.  The waves interleave the K-steps of the slab and are
// summed through LDS in wave order; the next step's rows are requested before the current step's 48 MFMAs are issued.
__global__ __launch_bounds__(256) void gram_cov_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ fac,
                                                       int64_t verts_per_slab, int nbp, int64_t partial_stride,
                                                       double *__restrict__ partial) {
    __shared__ double red[16 * 4 * 64];
    __shared__ double rsh[4][64];
    int pa = 0, pb = 0;
    {  // triangular patch index -> (pa <= pb)
        int t = blockIdx.y;
        for (pa = 0; pa < nbp; ++pa) {
            const int cnt = nbp - pa;
            if (t < cnt) {
                pb = pa + t;
                break;
            }
            t -= cnt;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t v0 = (int64_t)blockIdx.x * verts_per_slab;
    const int64_t v1 = min(M, v0 + verts_per_slab);
    typedef double d4 __attribute__((ext_vector_type(4)));
    const bool vla = pa * 64 + 4 * cl < rp, vlb = pb * 64 + 4 * cl < rp;  // rp is a multiple of 16: all-or-nothing per lane
    const bool diag = pa == pb, with_rhs = pa == 0;                        // (workgroup-uniform)
    v4f64 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0, 0, 0, 0};
    double racc[4] = {0, 0, 0, 0};
    struct Rows {
        d4 a[3], b[3];
        double c[6], g[3];
    };
    // rows past the slab: zeros on both sides and a zero factor (nothing is read there)
    auto load = [&](int64_t base, Rows &r) {
        const int64_t v = base + kq;
        const bool valid = v < v1;
        const int64_t vc = valid ? v : v0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            r.a[d] = r.b[d] = d4{0, 0, 0, 0};
            if (vlb && valid) r.b[d] = *reinterpret_cast<const d4 *>(Q0 + (3 * vc + d) * rp + pb * 64 + 4 * cl);
            if (!diag && vla && valid) r.a[d] = *reinterpret_cast<const d4 *>(Q0 + (3 * vc + d) * rp + pa * 64 + 4 * cl);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) r.c[k] = valid ? fac[k * M + vc] : 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) r.g[d] = (valid && with_rhs) ? fac[(6 + d) * M + vc] : 0.0;
    };
    auto transform = [&](const d4 q[3], const double c[6], double y[3][4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            y[0][t] = __builtin_fma(c[2], q[2][t], __builtin_fma(c[1], q[1][t], c[0] * q[0][t]));
            y[1][t] = __builtin_fma(c[4], q[2][t], c[3] * q[1][t]);
            y[2][t] = c[5] * q[2][t];
        }
    };
    Rows cur, nxt;
    int64_t base = v0 + 4 * wave;
    load(base, cur);
    for (; base < v1; base += 16) {
        load(base + 16, nxt);  // (past the slab: zeros, no request)
        double ya[3][4], yb[3][4];
        transform(cur.b, cur.c, yb);
        if (!diag) transform(cur.a, cur.c, ya);
        if (with_rhs) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int t = 0; t < 4; ++t) racc[t] = __builtin_fma(cur.b[d][t], cur.g[d], racc[t]);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(diag ? yb[d][i] : ya[d][i], yb[d][j], acc[i][j], 0, 0, 0);
        cur = nxt;
    }
    // right-hand side: the four vertices of a step (lane groups) first, then the waves 0..3 in order
    if (with_rhs) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            racc[t] += __shfl_xor(racc[t], 16);
            racc[t] += __shfl_xor(racc[t], 32);
        }
        if (kq == 0)
#pragma unroll
            for (int t = 0; t < 4; ++t) rsh[wave][4 * cl + t] = racc[t];
    }
    // waves 1..3 are added into wave 0 in order
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) red[((i * 4 + j) * 4 + reg) * 64 + lane] = acc[i][j][reg];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[i][j][reg] += red[((i * 4 + j) * 4 + reg) * 64 + lane];
        }
    }
    if (wave != 0) return;
    double *out = partial + (int64_t)blockIdx.x * partial_stride;
    if (with_rhs && kq == 0 && vlb) {  // (rsh was written before the first barrier above)
        double *rhs_out = out + (int64_t)rp * rp;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 4 * cl + t;
            rhs_out[pb * 64 + c] = ((rsh[0][c] + rsh[1][c]) + rsh[2][c]) + rsh[3][c];
        }
    }
    // D[i_row][j_col]: i_row = kq + 4*reg is the A-side lane index, j_col = cl the B-side lane index
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = pa * 64 + 4 * (kq + 4 * reg) + i;
                const int gj = pb * 64 + 4 * cl + j;
                if (gi < rp && gj < rp) out[(int64_t)gi * rp + gj] = acc[i][j][reg];
            }
        }
}

// G[i][j] += sum over slabs, i <= j mirrored; rhs[k] += sum over slabs.  The grouping and order of gram_reduce_kernel (gp_gram.hip):
// 32 consecutive entries x 8 slab groups per workgroup, group g adds the slabs g, g + 8, ... in ascending order, the groups are
// combined as ((0+1)+(2+3))+((4+5)+(6+7)).  Entry idx >= rp * rp is the right-hand side behind the patch entries of a slab.
__global__ __launch_bounds__(256) void gram_cov_reduce_kernel(const double *__restrict__ partial, int nslabs, int rp, int64_t partial_stride,
                                                              double *__restrict__ G, double *__restrict__ rhs) {
    __shared__ double sh[8][33];
    const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int idx = blockIdx.x * 32 + el;
    const int rr = rp * rp;
    const int i = idx / rp, j = idx - i * rp;
    const bool is_rhs = idx >= rr;
    const bool need = idx < rr + rp && (is_rhs || i <= j);
    double s = 0.0;
    if (need) {
        const double *p = partial + idx;
#pragma unroll 8
        for (int b = g; b < nslabs; b += 8) s += p[(int64_t)b * partial_stride];
    }
    sh[g][el] = s;
    __syncthreads();
    if (g == 0 && need) {
        const double t = ((sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el])) + ((sh[4][el] + sh[5][el]) + (sh[6][el] + sh[7][el]));
        if (is_rhs) {
            rhs[idx - rr] += t;
        } else {
            G[i * rp + j] += t;
            if (i != j) G[j * rp + i] += t;
        }
    }
}

}  // namespace

int64_t gram_cov_ws_doubles(int64_t M, int32_t rp) { return gram_cov_plan::make_plan(M, (int)rp).workspace_doubles(); }

void launch_gram_cov(gingr_ctx *ctx, const gingr_model *m, const DevState *st, const double *obs_soa, const double *prec6,
                     const int32_t *lm_mask, double *ws, double *G, double *rhs) {
    const int64_t M = m->M;
    const int rp = (int)m->rp;
    const gram_cov_plan::Plan p = gram_cov_plan::make_plan(M, rp);
    double *partial = ws, *fac = ws + p.partial_doubles();
    hipLaunchKernelGGL(cov_obs_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, m->ref, m->mean, M, st, obs_soa, prec6, lm_mask,
                       fac);
    hipLaunchKernelGGL(gram_cov_kernel, dim3((unsigned)p.nslabs, (unsigned)p.npatch), dim3(256), 0, ctx->stream, m->Q0, M, rp, (const double *)fac,
                       p.verts_per_slab, p.nbp, p.partial_stride(), partial);
    hipLaunchKernelGGL(gram_cov_reduce_kernel, dim3((unsigned)ceil_div((int64_t)rp * rp + rp, 32)), dim3(256), 0, ctx->stream,
                       (const double *)partial, p.nslabs, rp, p.partial_stride(), G, rhs);
}
