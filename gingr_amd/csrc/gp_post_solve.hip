// The post-solve kernel of the GiNGR update with its mat-vec helpers for gfx950 (MI355X).
//
//   post_solve_kernel LandmarkRegistration.rigid3D/similarity3DLandmarkRegistration (3x3 SVD + Euler round trip) from the moments,
//                     second projection, the state hand-over of update (G/api/GingrAlgorithm.scala:239-246) incl. the Try-failure
//                     paths and the retry counter of the probabilistic proposal (:194-210,248,251)
// rotation conventions (euler_to_rot / rot_to_euler): svd3.h
#include "gp.h"
#include "gp_device.h"
#include "svd3.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------------------------------------- fused post-solve
// one-off r x r products at finalisation
// out = scale * A B on the r x r block, zero on the padding (A, B, out: [rp][rp], rp a multiple of 16, zero padded).  One wave per
// 16 x 16 tile on the matrix pipe; the operands are L2 resident (one thread per entry with a serial dot product was 160 us at
// rank 512, 28 of them per model).
__global__ __launch_bounds__(256) void small_gemm_kernel(int r, int rp, const double *__restrict__ A, const double *__restrict__ B, double scale,
                                                         double *__restrict__ out) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    const int nt = rp >> 4;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= nt * nt) return;
    const int ti = tile / nt, tj = tile - ti * nt;
    const double *pa = A + (int64_t)(16 * ti + l15) * rp + l4;  // A[i = l15][k = l4]
    const double *pb = B + (int64_t)l4 * rp + 16 * tj + l15;    // B[k = l4][j = l15]
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < rp; k0 += 16) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = pa[k0 + 4 * u];
            b[u] = pb[(int64_t)(k0 + 4 * u) * rp];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int row = 16 * ti + l4 + 4 * g, col = 16 * tj + l15;
        out[(int64_t)row * rp + col] = (row < r && col < r) ? acc[g] * scale : 0.0;
    }
}

// one-off, the model's PostVec block (column-major for the post-solve kernel: entry i of vector v at pvec[i * kRows + v]):
// v = blockIdx.x < 12: the moment vector in[v] itself (V[d][e], W[d]); v >= 12: Binv in[v - 12]
__global__ __launch_bounds__(256) void postvec_kernel(int r, int rp, const double *__restrict__ Binv, const double *__restrict__ in,
                                                      double *__restrict__ pvec) {
    const int v = blockIdx.x;
    const double *x = in + (int64_t)(v % 12) * rp;
    for (int i = threadIdx.x; i < rp; i += 256) {
        double s = 0.0;
        if (v < 12)
            s = x[i];
        else if (i < r)
            for (int j = 0; j < r; ++j) s = __builtin_fma(Binv[(int64_t)i * rp + j], x[j], s);
        pvec[(int64_t)i * PostVec::kRows + v] = s;
    }
}

// zbuf[b] = M_b x_b, b = blockIdx.x (PostVec layout: gp.h): b < 9: S[d][e] alpha; 9 <= b < 18: (Binv S[d][e]) alpha; 18 <= b < 27:
// (Binv S[d][e] C) a; b == 27: C a.  blockIdx.y picks a strip of 16 output rows, 16 lanes per row; a lane's (up to 32) matrix
// elements are all requested before the first FMA -- the matrices live in L2 / the Infinity Cache and a dependent load-FMA chain
// costs one round trip per element.
__global__ __launch_bounds__(256) void post_matvecs_kernel(int r, int rp, const double *__restrict__ mom,
                                                           const double *__restrict__ cmat, const double *__restrict__ alpha,
                                                           const double *__restrict__ a, double *__restrict__ zbuf) {
    const int b = blockIdx.x;
    const MomentLayout ml{rp};
    const double *Mat = b < 9 ? mom + ml.S(b / 3, b % 3) : (b < 27 ? cmat + (int64_t)(b - 8) * rp * rp : cmat);
    const double *src = b < 18 ? alpha : a;
    const int lane16 = threadIdx.x & 15;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4);  // < rp (the grid covers rp / 16 strips)
    const double *row = Mat + (int64_t)i * rp;
    double m[32], x[32];  // rp <= 512
    const int nj = rp >> 4;
#pragma unroll
    for (int jj = 0; jj < 32; ++jj)
        if (jj < nj) {
            m[jj] = row[lane16 + 16 * jj];
            x[jj] = src[lane16 + 16 * jj];  // padding entries of alpha / a are zero
        }
    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < 32; ++jj)
        if (jj < nj) s = __builtin_fma(m[jj], x[jj], s);
    s = group16_sum(s);
    if (lane16 == 0) zbuf[(int64_t)i * PostVec::kZRows + b] = i < r ? s : 0.0;  // column-major: entry i of all 28 vectors is contiguous
}

// ---- post-solve: everything of GingrAlgorithm.update after the posterior coefficients (GingrAlgorithm.scala:212-246) in one small
// workgroup.  Round 4 rebuilt it around one measured fact (profiles/r03_exp_post_solve_code_touch.txt): run behind the long all-pairs
// kernels the round-3 kernel took 16-18 us against 6-9 us with warm caches -- it waited for its own CODE (20 KB of run-once
// straight-line float64 code through a cold instruction cache), not for its data.  So this version is built to EXECUTE few bytes:
//   * the second coefficient projection alpha' = Binv proj / eps is linear in the 3 x 3 pose quantities, proj = sum (B - I)_de V[d][e]
//     + sum B_de S[d][e] alpha_c + sum h_d W[d], so Binv is applied BEFORE the pose is known: Binv V / Binv W once per model
//     (gingr_model::pvec), (Binv S[d][e]) alpha and (Binv S[d][e] C) a by the mat-vec launch in front of this kernel.  No r x r matrix is
//     read here (round 3 copied the 100 KB of Binv through LDS and ran a mat-vec on it), one variant serves every rank <= 512;
//   * thread k keeps entry k of all 52 input vectors in registers: zbuf and pvec are stored entry-major ([rp][28], [rp][24]), so a
//     thread reads two contiguous runs with 16-byte loads at immediate offsets, all in flight at once; the 36 dot products of the
//     Umeyama sums are 36 multiplies per thread and ONE transposed reduction through LDS ([rp][37] products, 144 threads add a
//     quarter of a column each, fixed order) instead of 36 wave reductions;
//   * the 3 x 3 algebra of the pose step runs with one matrix entry per lane (a 3 x 3 product is three multiply-adds per lane, the
//     16 divisions by n are one division in 16 lanes) instead of every lane repeating all of it; the polar iteration and the
//     Euler round trip (svd3.h; the reference rebuilds R from the stored angles, so it cannot be dropped) are as before;
//   * the state is committed by 20 lanes from a staged copy instead of ~40 scalar stores of one thread.
// 16.5 KB + 3.9 KB of callees (1 024 threads, 138 KB of LDS)  ->  see tools/kernel_resources.sh / DESIGN.md section 4 for the figures.
//
// Failure semantics of GingrAlgorithm.update (G/api/GingrAlgorithm.scala:192-254):
//   posterior failed (Try of computePosterior, here: the solve flagged st->err)
//       iteration 0                      -> state unchanged                                          (:206-208)
//       iteration > 0, deterministic     -> ModelFlexibilityError                                    (:203-205)
//       iteration > 0, probabilistic     -> retryCounter == 0 ? ModelFlexibilityError
//                                           : { retryCounter -= 1; state unchanged }                  (:196-202)
//   posterior fine                       -> retryCounter = min(10, retryCounter + 1)                  (:210)
//       a coefficients() projection (or the alignment between them) failed -> ModelFlexibilityError at ANY iteration
//                                                                                                     (:248-251)
// Non-finite values count as failures: in the reference they make Breeze's SVD throw inside the Try.

// scratch of the pose step (doubles in LDS)
struct PoseLds {
    double D[36];     // the dot products: [0..2] W[d].alpha, [3..5] W[d].alpha_c, [6..14] V[b][d].alpha (index d*3+b),
                      // [15..23] V[d][b].alpha_c, [24..32] alpha_c.za[d][b], [33..35] alpha.za[d][d]
    double R[9];      // rotation of the current state
    double su[3], sv[3], gt[3], q[3];
    double Mvu[9];
    double sums[16];  // [0..2] sum x~, [3..5] sum y~, [6..14] sum y~ x~^T (row-major), [15] sum |x~|^2; x~ = x - c0, y~ = y - c0
    double qn[16];    // sums / n
    double Sxy[9];
    double R2[9];
    double coef[21];  // (B - I)[9], B[9], h[3]: the 3 x 3 quantities of the second projection, B = R2^T R
    double stage[20]; // the committed DevState: R[9], euler[3], center[3], t[3], scale, sigma2
};

// One wave: Umeyama between the current shape u~_i = p~_i + Q0_i alpha (unposed) and the blended posterior mean
// newshape - c0 = R v~_i + g~, v~_i = p~_i + Q0_i alpha_c, from the 36 dot products (moment form), then the 3 x 3 quantities of the
// second projection e_i = R2^T (newshape_i - t2) - p_i = (B - I) p~_i + B Q0_i alpha_c + h.  Lane l < 9 owns matrix entry (l / 3, l % 3).
// cst (device): Pp[9] = sum p~ p~^T, Ps[3] = sum p~, c0[3], n  (PostVec::consts)
__device__ void post_pose_step(const PostSolveArgs &A, const DevState *st, const double *__restrict__ cst, PoseLds &L, int *bad) {
    const int l = threadIdx.x & 63;
    const int l9 = l < 9 ? l : 8, a = l9 / 3, b = l9 - 3 * a, l3 = l < 3 ? l : 2;
    const double Ppl = cst[l9], Psl = cst[9 + l3], c0l = cst[12 + l3], n = cst[15];
    const double Rl = st->R[l9], cenl = st->center[l3], tl = st->t[l3];
    if (l < 9) {
        L.R[l] = Rl;
        L.Mvu[l] = Ppl + L.D[6 + l] + L.D[15 + l] + L.D[24 + l];
    }
    if (l < 3) {
        L.su[l] = Psl + L.D[l];
        L.sv[l] = Psl + L.D[3 + l];
        L.q[l] = c0l - cenl;
    }
    double s15 = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) s15 += cst[4 * d] + 2.0 * L.D[6 + 4 * d] + L.D[33 + d];
    __builtin_amdgcn_wave_barrier();
    if (l < 3) L.gt[l] = L.R[3 * l] * L.q[0] + L.R[3 * l + 1] * L.q[1] + L.R[3 * l + 2] * L.q[2] + cenl + tl - c0l;
    __builtin_amdgcn_wave_barrier();
    if (l < 3) {
        L.sums[l] = L.su[l];
        L.sums[3 + l] = L.R[3 * l] * L.sv[0] + L.R[3 * l + 1] * L.sv[1] + L.R[3 * l + 2] * L.sv[2] + n * L.gt[l];
    }
    if (l < 9) L.sums[6 + l] = L.R[3 * a] * L.Mvu[b] + L.R[3 * a + 1] * L.Mvu[3 + b] + L.R[3 * a + 2] * L.Mvu[6 + b] + L.gt[a] * L.su[b];
    if (l == 15) L.sums[15] = s15;
    __builtin_amdgcn_wave_barrier();
    double R2[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, eul[3] = {0, 0, 0}, t2[3] = {0, 0, 0}, c = 1.0;
    const double c0[3] = {cst[12], cst[13], cst[14]};
    bool fin = true;
    if (A.global_transform != GINGR_NO_TRANSFORMS) {  // (identityTransformation otherwise, GingrAlgorithm.scala:230)
        L.qn[l & 15] = L.sums[l & 15] / n;  // mu_x, mu_y, the second moments and the variance term: one division in 16 lanes
        __builtin_amdgcn_wave_barrier();
        if (l < 9) L.Sxy[l] = L.qn[6 + l] - L.qn[3 + a] * L.qn[b];
        const double mux[3] = {L.qn[0], L.qn[1], L.qn[2]}, muy[3] = {L.qn[3], L.qn[4], L.qn[5]};
        const double sig2x = L.qn[15] - (mux[0] * mux[0] + mux[1] * mux[1] + mux[2] * mux[2]);
        __builtin_amdgcn_wave_barrier();
        double S[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) S[q] = L.Sxy[q];
        // R = U diag(1, 1, sign det) V^T and, for similarity transforms, c = (d1 + d2 + sign d3) / var_x.  With det > 0 (every
        // non-degenerate registration) R is the polar factor of Sxy and d1 + d2 + d3 = trace(R^T Sxy): no SVD (svd3.h)
        double Rr[9], trace_ds = 0.0;
        if (!polar3_rotation(S, Rr, &trace_ds)) {
            double U[9], Dg[3], V[9];
            svd3(S, U, Dg, V);
            const double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
            const double s3 = det < 0 ? -1.0 : 1.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Rr[i * 3 + j] = U[i * 3] * V[j * 3] + U[i * 3 + 1] * V[j * 3 + 1] + s3 * U[i * 3 + 2] * V[j * 3 + 2];
            trace_ds = Dg[0] + Dg[1] + s3 * Dg[2];
        }
        c = (A.global_transform == GINGR_SIMILARITY_TRANSFORMS) ? trace_ds / sig2x : 1.0;
        // t = mu_y - c R mu_x in absolute coordinates (rotation about the origin)
        double mxa[3], mya[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            mxa[i] = mux[i] + c0[i];
            mya[i] = muy[i] + c0[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) t2[i] = mya[i] - c * (Rr[i * 3] * mxa[0] + Rr[i * 3 + 1] * mxa[1] + Rr[i * 3 + 2] * mxa[2]);
        // the registration result carries its rotation as Euler angles (rigid3DLandmarkRegistration builds Rotation3D)
        rot_to_euler_wave(Rr, eul);
        euler_to_rot_wave(eul, R2);
        fin = finite_d(c);
#pragma unroll
        for (int q = 0; q < 9; ++q) fin = fin && finite_d(R2[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) fin = fin && finite_d(t2[q]);
    }
    if (l == 0) {
        if (!fin) *bad = 1;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            L.R2[q] = R2[q];
            L.stage[q] = R2[q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            L.stage[9 + q] = eul[q];
            L.stage[12 + q] = 0.0;  // Umeyama about Point(0,0,0), GingrAlgorithm.scala:81,266
            L.stage[15 + q] = t2[q];
        }
        L.stage[18] = c;
        if (A.is_icp == 2) {  // the pairs flavour: the trait's default updateSigma2 (GingrAlgorithm.scala:256-258), sigma2 stays
            L.stage[19] = st->sigma2;
        } else if (A.is_icp) {
            const double ns = st->sigma2 - A.icp_step;  // ICP.scala:96-99
            L.stage[19] = ns > A.icp_end ? ns : A.icp_end;
        } else {
            const double *sc = A.scalars;  // CPD.scala:142-145
            L.stage[19] = (sc[1] - 2 * sc[2] + sc[3]) / (sc[0] * 3.0);
        }
    }
    __builtin_amdgcn_wave_barrier();
    // B = R2^T R, h = R2^T (g~ + c0 - t2) - c0   (p_i = p~_i + c0)
    if (l < 9) {
        const double v = L.R2[a] * L.R[b] + L.R2[3 + a] * L.R[3 + b] + L.R2[6 + a] * L.R[6 + b];
        L.coef[l] = v - (a == b ? 1.0 : 0.0);
        L.coef[9 + l] = v;
    }
    if (l < 3) {
        const double w0 = L.gt[0] + c0[0] - t2[0], w1 = L.gt[1] + c0[1] - t2[1], w2 = L.gt[2] + c0[2] - t2[2];
        L.coef[18 + l] = (L.R2[l] * w0 + L.R2[3 + l] * w1 + L.R2[6 + l] * w2) - c0l;
    }
}

constexpr int kPostMinThreads = 256;

// A.zbuf: [rp][28] of launch_post_matvecs; A.pvec: the model's PostVec block.  blockDim = max(256, rp rounded up to 64);
// dynamic LDS: 37 rp doubles.
__global__ __launch_bounds__(512) void post_solve_kernel(PostSolveArgs A) {
    extern __shared__ double prod[];  // [rp][37]: the 36 products of entry k (odd row stride: the column sums below spread over the banks)
    __shared__ PoseLds L;
    __shared__ int bad;
    constexpr int ld = 37;
    const int r = A.r, rp = A.rp, tid = threadIdx.x;
    DevState *st = A.state;
    if (tid == 0 && A.zero_slot) *A.zero_slot = 0.0;  // see SweepArgs::absmax_slot: the fit pass behind this kernel takes a maximum into it
    if (st->status == GINGR_FIT_MODEL_FLEXIBILITY_ERROR || st->stopped) return;  // a failed fit stays as it is (run stops, :149-157);
                                                                                 // so does one the run's own rule stopped at
    const PostVec pvl{rp};
    // ---- column tid of every input vector: all loads in flight at once
    double za[9], bz[9], V[9], W[3], BV[9], BW[3], al = 0.0, ac = 0.0;
    if (tid < rp) {
        const double *zb = A.zbuf + (int64_t)tid * PostVec::kZRows, *pv = A.pvec + (int64_t)tid * PostVec::kRows;
        double bs[9], bt[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            za[q] = zb[PostVec::kZa + q];
            bs[q] = zb[PostVec::kBSa + q];
            bt[q] = zb[PostVec::kBTa + q];
            V[q] = pv[PostVec::kV + q];
            BV[q] = pv[PostVec::kBV + q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            W[q] = pv[PostVec::kW + q];
            BW[q] = pv[PostVec::kBW + q];
        }
        const double a1 = zb[PostVec::kA1];  // alpha_1 = C a: coefficients of the posterior mean (transformedModelInit.coefficients,
        al = tid < r ? A.alpha[tid] : 0.0;        // :212-216; Q^T (Q a) = S_tot a and the R / R^T round trip of the displacement cancels)
        ac = tid < r ? al + (a1 - al) * A.step : 0.0;  // the step blend (:218-220)
        // Binv S[d][e] alpha_c = (1 - step) (Binv S[d][e]) alpha + step (Binv S[d][e] C) a
#pragma unroll
        for (int q = 0; q < 9; ++q) bz[q] = (1.0 - A.step) * bs[q] + A.step * bt[q];
        // ---- the 36 products of the dot products (PoseLds::D), column tid
        double *p = prod + tid * ld;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            p[d] = W[d] * al;
            p[3 + d] = W[d] * ac;
            p[33 + d] = al * za[4 * d];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                p[6 + d * 3 + b] = V[b * 3 + d] * al;
                p[15 + d * 3 + b] = V[d * 3 + b] * ac;
                p[24 + d * 3 + b] = ac * za[d * 3 + b];
            }
        }
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid < 144) {  // thread (t, part) adds the products k = part, part + 4, ... of dot product t; then (p0 + p1) + (p2 + p3)
        const int t = tid >> 2, part = tid & 3;
        const double *colp = prod + part * ld + t;
        double s = 0.0;
        for (int k = 0; k < rp; k += 4) s += colp[k * ld];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (part == 0) L.D[t] = s;
    }
    __syncthreads();
    if (tid < 64) post_pose_step(A, st, A.pvec + pvl.consts(), L, &bad);
    __syncthreads();
    // ---- second projection (transformedModel.coefficients(newshape), :234-237), Binv already applied to every term
    double anew = 0.0;
    if (tid < rp) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            s = __builtin_fma(L.coef[q], BV[q], s);
            s = __builtin_fma(L.coef[9 + q], bz[q], s);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) s = __builtin_fma(L.coef[18 + d], BW[d], s);
        anew = tid < r ? s / GINGR_COEFF_NOISE : 0.0;
        if (!finite_d(anew)) bad = 1;
    }
    __syncthreads();
    const bool posterior_failed = st->err != 0;
    const bool failed = posterior_failed || bad != 0;
    const double sigma2_before = st->sigma2;
    __syncthreads();  // (every thread has read st->err and sigma2 before they are rewritten)
    if (!failed) {
        if (tid < rp) A.alpha[tid] = anew;
        if (tid < 20) reinterpret_cast<double *>(st)[tid] = L.stage[tid];  // R, euler, center, t, scale, sigma2
    }
    if (tid == 0) {
        if (posterior_failed) {
            if (st->iteration > 0) {
                if (A.probabilistic && A.retry && *A.retry > 0)
                    *A.retry -= 1;
                else
                    st->status = GINGR_FIT_MODEL_FLEXIBILITY_ERROR;
            }
        } else {
            if (A.retry) *A.retry = *A.retry + 1 < GINGR_RETRY_INIT ? *A.retry + 1 : GINGR_RETRY_INIT;
            if (bad != 0) st->status = GINGR_FIT_MODEL_FLEXIBILITY_ERROR;
        }
        st->pad = failed ? (st->err != 0 ? st->err : GINGR_ERR_NONFINITE) : 0;  // last error, readable by the host
        st->err = 0;
        st->iteration += 1;  // GingrGeneratorWrapper.propose: updateIteration()
        // the dropWhile of GingrAlgorithm.run (:142-153) looks at (last state, this state): converged -- or failed -- and the chain ends HERE
        if (A.stop_threshold >= 0.0 && fabs(sigma2_before - (failed ? sigma2_before : L.stage[19])) < A.stop_threshold) st->stopped = 1;
    }
}

__global__ void state_init_kernel(DevState *st, const gingr_state_scalars *h, double *zero_slot) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    state_init_body(st, h, zero_slot);
}

}  // namespace

void launch_post_solve(gingr_ctx *ctx, const PostSolveArgs &a) {
    const size_t lds = (size_t)37 * a.rp * sizeof(double);
    const int nt = std::max<int>(kPostMinThreads, (int)round_up(a.rp, 64));
    if (lds > 48 * 1024)  // (per function AND per device: set whenever it is needed, never cached in a process-wide static)
        set_dynamic_lds(&post_solve_kernel, (size_t)(lds));
    hipLaunchKernelGGL(post_solve_kernel, dim3(1), dim3(nt), lds, ctx->stream, a);
}

void launch_post_matvecs(gingr_ctx *ctx, const gingr_model *m, const double *alpha, const double *a, double *zbuf) {
    hipLaunchKernelGGL(post_matvecs_kernel, dim3(PostVec::kZRows, (unsigned)(m->rp / 16)), dim3(256), 0, ctx->stream, (int)m->r, (int)m->rp,
                       m->mom, m->cmat, alpha, a, zbuf);
}

void launch_postvec(gingr_ctx *ctx, int32_t r, int32_t rp, const double *Binv, const double *moment_vectors, double *pvec) {
    hipLaunchKernelGGL(postvec_kernel, dim3((unsigned)PostVec::kRows), dim3(256), 0, ctx->stream, (int)r, (int)rp, Binv, moment_vectors, pvec);
}

void launch_small_gemm(gingr_ctx *ctx, int32_t r, int32_t rp, const double *A, const double *B, double scale, double *out) {
    const int64_t tiles = (int64_t)(rp / 16) * (rp / 16);
    hipLaunchKernelGGL(small_gemm_kernel, dim3((unsigned)ceil_div(tiles, 4)), dim3(256), 0, ctx->stream, (int)r, (int)rp, A, B, scale, out);
}


void launch_state_init(gingr_ctx *ctx, DevState *st, const gingr_state_scalars *host_scalars_dev, double *zero_slot) {
    hipLaunchKernelGGL(state_init_kernel, dim3(1), dim3(64), 0, ctx->stream, st, host_scalars_dev, zero_slot);
}
