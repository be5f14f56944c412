// A resident model augmented with a second one on the same reference (C ABI in include/gingr_hip.h: gingr_model_augment) -- what a
// scalismo user gets from PointDistributionModel.augmentModel(pcaModel, biasModel): the model whose covariance is the sum of the two.
//   F = [Q_a | Q_b]                     (Q = U sqrt(lambda): what Q0 holds; never formed)
//   G = F^T F = [[S_a, C], [C^T, S_b]]  S_a, S_b: the resident moments S_tot of the two models, C = Q_a^T Q_b (cross_gram_kernel)
//   G = V diag(lambda) V^T              the solvers of eig.hip on G + (trace / n) I (G is singular for b == a or ra + rb > 3 M)
//   Q0 = Q_a V[:ra, :k] + Q_b V[ra:, :k]  (basis_rotate2_kernel: one pass over both bases, every output row written once)
//   mean = mean_a + mean_b, variance lambda[:k], rows in the Morton order of ref + mean_a + mean_b
// The two models order their rows by the Morton code of their own ref + mean: a vertex sits at different rows of the two bases, and
// at a third one of the result.  Every sum is taken in a fixed order (slab partials combined by one thread each, no float atomics):
// two builds of the same input give the same bits.
// The shifted eigen step, the factor rows and the moment trace are the shared tail of posterior_model.hip (gp.h), the choice of k is
// spectrum_plan.h, the complete-model check is model.hip's (gp.h).
#include "basis_rotate.h"
#include "spectrum_plan.h"

#include <algorithm>
#include <cmath>

namespace {

// ---- C = Q_a^T Q_b.  A workgroup of 4 waves computes one 64 x 64 patch (4 x 4 MFMA tiles) of C over one slab of vertices of a, walked
// in a's row order; the waves interleave the 4-vertex steps of the slab and are summed through LDS in a fixed order (gram_kernel,
// gp_gram.hip).  A step is four vertices, coordinate by coordinate:
//   D(16x16) += A(16x4) B(4x16),  A[i][k] = Q_a[3 (s0 + k) + d][a0 + i],  B[k][j] = Q_b[3 iperm_b[perm_a[s0 + k]] + d][b0 + j]
// lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D: lane holds column j = l & 15 of the rows i = (l >> 4) + 4 reg.
// The lane group k = l >> 4 owns vertex s0 + k: it reads the vertex's row in b once per step and then the three contiguous rows of each
// basis.  Column interleave as in gram_kernel: tile t of the patch holds the columns {64 p + 4 (l & 15) + t}, so the four fragment values a
// lane needs per side and row are 32 contiguous bytes.  Vertices past M (the last step of the last slab) read row 3 M + d of both
// bases -- the zero rows behind every basis (kBasisRowSlack); slab lengths are multiples of 16, so no other step runs past its slab.
// Padded columns are zero in both bases: zero in, zero out.  The next step's fragments are loaded before this step's 48 MFMAs.
__global__ __launch_bounds__(256) void cross_gram_kernel(const double *__restrict__ Qa, int rpa, const int32_t *__restrict__ perm_a,
                                                         const double *__restrict__ Qb, int rpb, const int32_t *__restrict__ iperm_b, int64_t M,
                                                         int64_t verts_per_slab, int npb, double *__restrict__ partial) {
    __shared__ double red[16 * 4 * 64];
    const int pa = blockIdx.y / npb, pb = blockIdx.y - pa * npb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t v0 = (int64_t)blockIdx.x * verts_per_slab;
    const int64_t v1 = min(M, v0 + verts_per_slab);
    v4f64 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0, 0, 0, 0};
    const bool vla = pa * 64 + 4 * cl < rpa, vlb = pb * 64 + 4 * cl < rpb;  // rp is a multiple of 16: all-or-nothing per lane
    const double *pa_col = Qa + pa * 64 + 4 * cl, *pb_col = Qb + pb * 64 + 4 * cl;
    auto load = [&](int64_t s0, d4 fa[3], d4 fb[3]) {
        const int64_t s = s0 + kq;
        const int64_t ra = s < M ? s : M, rb = s < M ? (int64_t)iperm_b[perm_a[s]] : M;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            fa[d] = vla ? *reinterpret_cast<const d4 *>(pa_col + (3 * ra + d) * rpa) : d4{0, 0, 0, 0};
            fb[d] = vlb ? *reinterpret_cast<const d4 *>(pb_col + (3 * rb + d) * rpb) : d4{0, 0, 0, 0};
        }
    };
    d4 ca[3], cb[3];
    int64_t s0 = v0 + 4 * wave;
    if (s0 < v1) load(s0, ca, cb);
    for (; s0 < v1; s0 += 16) {
        d4 na[3], nb[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) na[d] = nb[d] = d4{0, 0, 0, 0};
        if (s0 + 16 < v1) load(s0 + 16, na, nb);
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[d][i], cb[d][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            ca[d] = na[d];
            cb[d] = nb[d];
        }
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
    double *out = partial + (int64_t)blockIdx.x * rpa * rpb;
    // D[i_row][j_col]: i_row = kq + 4 reg is the A-side lane index, j_col = cl the B-side lane index
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = pa * 64 + 4 * (kq + 4 * reg) + i;
                const int gj = pb * 64 + 4 * cl + j;
                if (gi < rpa && gj < rpb) out[(int64_t)gi * rpb + gj] = acc[i][j][reg];
            }
}

// C[e] = sum over slabs in a fixed order (gram_reduce_kernel, gp_gram.hip): 32 consecutive elements x 8 slab groups per workgroup; group
// g adds the slabs g, g + 8, ... in ascending order, the groups are combined as ((0+1)+(2+3))+((4+5)+(6+7))
__global__ __launch_bounds__(256) void cross_gram_reduce_kernel(const double *__restrict__ partial, int nslabs, int n, double *__restrict__ C) {
    __shared__ double sh[8][33];
    const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int idx = blockIdx.x * 32 + el;
    double s = 0.0;
    if (idx < n) {
        const double *p = partial + idx;
#pragma unroll 8
        for (int b = g; b < nslabs; b += 8) s += p[(int64_t)b * n];
    }
    sh[g][el] = s;
    __syncthreads();
    if (g == 0 && idx < n) C[idx] = ((sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el])) + ((sh[4][el] + sh[5][el]) + (sh[6][el] + sh[7][el]));
}

// ---- Qn[3 s + d][:] = Q_a[3 s_a + d][:] T_a + Q_b[3 s_b + d][:] T_b for the device rows s < M of the new model, s_a = iperm_a[perm_new[s]],
// s_b = iperm_b[perm_new[s]].  basis_rotate_kernel (posterior_model.hip) with two sources: the same workgroup shape, tiles and stores
// (basis_rotate.h); both sources accumulate into the same accumulator tiles, a first and then b, and every row of Qn is written once.
// T_a [rpa][rp], T_b [rpb][rp], zero beyond the ranks.  The lanes of vertices past the last one read the zero rows behind the bases.
template <int NT>
__device__ __forceinline__ void rotate2_chunk(const double *__restrict__ qa, int rpa, const double *__restrict__ Ta, const double *__restrict__ qb,
                                              int rpb, const double *__restrict__ Tb, int rp, int n0, int kq, int cl, double *__restrict__ out,
                                              int64_t vleft) {
    const Rot3 identity{{1, 0, 0, 0, 1, 0, 0, 0, 1}};  // (1 x + (0 y + 0 z) is x: the store of basis_rotate.h as it is)
    v4f64 acc[3][NT];
    rotate_clear<NT>(acc);
    rotate_accumulate<NT>(acc, qa, rpa, rp, Ta, n0, kq, cl);
    rotate_accumulate<NT>(acc, qb, rpb, rp, Tb, n0, kq, cl);
    rotate_store<NT>(acc, rp, n0, kq, cl, identity, out, vleft);
}

__global__ __launch_bounds__(64 * kRotWaves) void basis_rotate2_kernel(const double *__restrict__ Qa, int rpa, const int32_t *__restrict__ iperm_a,
                                                                       const double *__restrict__ Ta, const double *__restrict__ Qb, int rpb,
                                                                       const int32_t *__restrict__ iperm_b, const double *__restrict__ Tb, int64_t M,
                                                                       int rp, const int32_t *__restrict__ perm_new, int nchunks,
                                                                       double *__restrict__ Qn) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t vb = blockIdx.x / nchunks;
    const int chunk = (int)(blockIdx.x - vb * nchunks);
    const int64_t v0 = (vb * kRotWaves + wave) * kRotVerts;
    if (v0 >= M) return;
    const int64_t v = v0 + cl;
    const int32_t id = v < M ? perm_new[v] : 0;
    const int64_t sa = v < M ? (int64_t)iperm_a[id] : M, sb = v < M ? (int64_t)iperm_b[id] : M;
    const double *qa = Qa + 3 * sa * (int64_t)rpa, *qb = Qb + 3 * sb * (int64_t)rpb;
    double *out = Qn + 3 * v0 * (int64_t)rp;
    const int nt = rp / 16, t0 = chunk * kRotChunkTiles;
    switch (min(nt - t0, kRotChunkTiles)) {
        case 1: rotate2_chunk<1>(qa, rpa, Ta, qb, rpb, Tb, rp, 16 * t0, kq, cl, out, M - v0); break;
        case 2: rotate2_chunk<2>(qa, rpa, Ta, qb, rpb, Tb, rp, 16 * t0, kq, cl, out, M - v0); break;
        case 3: rotate2_chunk<3>(qa, rpa, Ta, qb, rpb, Tb, rp, 16 * t0, kq, cl, out, M - v0); break;
        case 4: rotate2_chunk<4>(qa, rpa, Ta, qb, rpb, Tb, rp, 16 * t0, kq, cl, out, M - v0); break;
        default: break;
    }
}

// ---- the r x r step
// Gs [n][n], n = ra + rb: [[S_a, C], [C^T, S_b]] + shift on the diagonal (S_a: row stride rpa; C [rpa][rpb]; S_b: row stride rpb).  Both
// off-diagonal blocks read the same entry of C: Gs is symmetric to the bit.  *bad is set when an entry is not finite.
__global__ __launch_bounds__(256) void augment_gram_kernel(const double *__restrict__ Sa, int ra, int rpa, const double *__restrict__ C,
                                                           const double *__restrict__ Sb, int rb, int rpb, double shift, double *__restrict__ Gs,
                                                           int32_t *__restrict__ bad) {
    const int n = ra + rb;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    double v;
    if (i < ra)
        v = j < ra ? Sa[(int64_t)i * rpa + j] : C[(int64_t)i * rpb + (j - ra)];
    else
        v = j < ra ? C[(int64_t)j * rpb + (i - ra)] : Sb[(int64_t)(i - ra) * rpb + (j - ra)];
    if (!isfinite(v)) atomicOr(bad, 1);
    Gs[e] = v + (i == j ? shift : 0.0);
}

}  // namespace

// (declared in basis_rotate.h: model_metrics.hip takes Q0^T D through the same pass, D a block of columns in the model's row order)
void cross_gram_plan(int64_t M, int32_t rpa, int32_t rpb, int *npa, int *npb, int *nslabs, int64_t *verts_per_slab) {
    *npa = (rpa + 63) / 64;
    *npb = (rpb + 63) / 64;
    // ~3 workgroups of 4 waves per CU; a slab writes a full rpa x rpb partial: below ~64 vertices per slab the partials cost more
    // than the rows they summarise
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(768 / (*npa * *npb), ceil_div(M, 64)));
    *verts_per_slab = round_up(ceil_div(M, want), 16);
    *nslabs = (int)ceil_div(M, *verts_per_slab);
}

// C [rpa][rpb] = Q_a^T Q_b on ctx->stream; ws: nslabs rpa rpb doubles (cross_gram_plan)
void launch_cross_gram(gingr_ctx *ctx, const gingr_model *a, const gingr_model *b, double *ws, double *C) {
    int npa, npb, nslabs;
    int64_t vps;
    cross_gram_plan(a->M, a->rp, b->rp, &npa, &npb, &nslabs, &vps);
    const int n = a->rp * b->rp;
    {
        TimerScope ts(ctx, 11);
        hipLaunchKernelGGL(cross_gram_kernel, dim3((unsigned)nslabs, (unsigned)(npa * npb)), dim3(256), 0, ctx->stream, a->Q0, (int)a->rp, a->perm,
                           b->Q0, (int)b->rp, b->iperm, a->M, vps, npb, ws);
    }
    hipLaunchKernelGGL(cross_gram_reduce_kernel, dim3((unsigned)ceil_div(n, 32)), dim3(256), 0, ctx->stream, ws, nslabs, n, C);
}

namespace {

void launch_basis_rotate2(gingr_ctx *ctx, const gingr_model *a, const double *Ta, const gingr_model *b, const double *Tb, gingr_model *dst) {
    const int nchunks = (int)ceil_div(dst->rp / 16, kRotChunkTiles);
    const int64_t blocks = ceil_div(dst->M, (int64_t)kRotWaves * kRotVerts) * nchunks;
    TimerScope ts(ctx, 12);
    hipLaunchKernelGGL(basis_rotate2_kernel, dim3((unsigned)blocks), dim3(64 * kRotWaves), 0, ctx->stream, a->Q0, (int)a->rp, a->iperm, Ta, b->Q0,
                       (int)b->rp, b->iperm, Tb, dst->M, (int)dst->rp, dst->perm, nchunks, dst->Q0);
}

}  // namespace

extern "C" {

int gingr_model_augment(gingr_ctx *ctx, const gingr_model *a, const gingr_model *b, double relative_tolerance, int32_t max_rank, gingr_model **out,
                        gingr_augment_info *info) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    const char *who = "model_augment";
    if (!a || !b) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (const char *fault = complete_model_fault(ctx, a))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the first model %s (both must be complete, finalized models of this context)", who, fault);
    if (const char *fault = complete_model_fault(ctx, b))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the second model %s (both must be complete, finalized models of this context)", who, fault);
    if (a->M != b->M)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the models have %lld and %lld points, need the same reference", who, (long long)a->M,
                               (long long)b->M);
    if (max_rank < 0 || !(relative_tolerance >= 0.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: max_rank and relative_tolerance must not be negative", who);
    const int64_t M = a->M;
    const int32_t ra = a->r, rb = b->r, rpa = a->rp, rpb = b->rp;
    const int n = ra + rb;
    if (n > 512)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d + %d = %d columns, at most 512: truncate the models first", who, (int)ra, (int)rb, n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // ---- 1. reference and mean displacement pass through the host once (they fix the new row order)
    std::vector<double> href((size_t)3 * M), hmean((size_t)3 * M), other((size_t)3 * M);
    GINGR_TRY(gingr_model_download(ctx, a, href.data(), nullptr, nullptr, nullptr));
    GINGR_TRY(gingr_model_download(ctx, b, other.data(), nullptr, nullptr, nullptr));
    for (int64_t e = 0; e < 3 * M; ++e)
        if (!(href[(size_t)e] == other[(size_t)e]))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the references differ at point %lld (%.17g against %.17g in coordinate %d)", who,
                                   (long long)(e / 3), href[(size_t)e], other[(size_t)e], (int)(e % 3));
    GINGR_TRY(gingr_model_download(ctx, a, nullptr, hmean.data(), nullptr, nullptr));
    GINGR_TRY(gingr_model_download(ctx, b, nullptr, other.data(), nullptr, nullptr));
    for (int64_t e = 0; e < 3 * M; ++e) {
        hmean[(size_t)e] += other[(size_t)e];
        if (!std::isfinite(hmean[(size_t)e])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite mean", who);
    }

    // ---- 2. G = [[S_a, C], [C^T, S_b]]: the two moments as stored (not diagonal for an uploaded basis that is not orthonormal) and the
    // cross block, the only new product
    const double *Sa = a->mom + MomentLayout{rpa}.stot(), *Sb = b->mom + MomentLayout{rpb}.stot();
    double tr_a = 0.0, tr_b = 0.0;
    GINGR_TRY(moment_trace(ctx, Sa, ra, rpa, &tr_a));
    GINGR_TRY(moment_trace(ctx, Sb, rb, rpb, &tr_b));
    const double trace = tr_a + tr_b;
    if (!std::isfinite(trace)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Gram matrix of the two bases", who);
    DevBuf ws, C, Gs, evals, V, Ta, Tb, flag;
    {
        int npa, npb, nslabs;
        int64_t vps;
        cross_gram_plan(M, rpa, rpb, &npa, &npb, &nslabs, &vps);
        HIP_TRY(ctx, ws.alloc((size_t)nslabs * rpa * rpb * sizeof(double)));
    }
    HIP_TRY(ctx, C.alloc((size_t)rpa * rpb * sizeof(double)));
    HIP_TRY(ctx, Gs.alloc((size_t)n * n * sizeof(double)));
    HIP_TRY(ctx, evals.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, V.alloc((size_t)n * n * sizeof(double)));
    HIP_TRY(ctx, flag.alloc(sizeof(int32_t)));
    HIP_TRY(ctx, hipMemsetAsync(flag.p, 0, sizeof(int32_t), ctx->stream));
    launch_cross_gram(ctx, a, b, ws.as<double>(), C.as<double>());
    // G is singular when b == a or ra + rb > 3 M, with a null space of many dimensions: the solvers get G + shift I, shift = trace / n
    // the mean eigenvalue -- the same eigenvectors, every eigenvalue moved by exactly the shift, condition number at most n + 1
    // (pca_model.hip, step 5, has the reasons)
    const double shift = trace / (double)n;
    hipLaunchKernelGGL(augment_gram_kernel, dim3((unsigned)ceil_div((int64_t)n * n, 256)), dim3(256), 0, ctx->stream, Sa, (int)ra, (int)rpa,
                       C.as<double>(), Sb, (int)rb, (int)rpb, shift, Gs.as<double>(), flag.as<int32_t>());
    GINGR_TRY(check_launch(ctx));
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ws.release();
    if (bad) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Gram matrix of the two bases", who);

    // ---- 3. G = V diag(lambda) V^T, lambda descending
    std::vector<double> lam;
    GINGR_TRY(eig_descending_to_host(ctx, Gs.as<double>(), n, n, shift, who, "eigenvalue", evals.as<double>(), V.as<double>(), lam));
    // (lam is un-shifted already: the cut subtracts nothing more)
    const spectrum_plan::Cut cut = spectrum_plan::cut(lam.data(), n, 0.0, n, max_rank, relative_tolerance);
    const int k = cut.k;
    if (k < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: no eigenvalue of the summed covariance passes the cutoff (rank 0)", who);

    // ---- 4. Q0 = Q_a V[:ra, :k] + Q_b V[ra:, :k] into the model proper
    const int kp = (int)round_up(k, 16);
    HIP_TRY(ctx, Ta.alloc((size_t)rpa * kp * sizeof(double)));
    HIP_TRY(ctx, Tb.alloc((size_t)rpb * kp * sizeof(double)));
    launch_factor_rows(ctx, V.as<double>(), n, 0, (int)ra, (int)rpa, k, kp, Ta.as<double>());
    launch_factor_rows(ctx, V.as<double>(), n, (int)ra, (int)rb, (int)rpb, k, kp, Tb.as<double>());
    GINGR_TRY(check_launch(ctx));
    auto fill = [&](gingr_model *nm) -> int {
        launch_basis_rotate2(ctx, a, Ta.as<double>(), b, Tb.as<double>(), nm);
        return check_launch(ctx);
    };
    GINGR_TRY(model_create_impl(ctx, M, k, href.data(), hmean.data(), lam.data(), 0, M, fill, out));
    if (info) {
        info->columns = n;
        info->rank = k;
        info->total_variance = trace;
        info->kept_variance = cut.kept;
    }
    return GINGR_OK;
}

}  // extern "C"
