// A PCA shape model from shapes in correspondence, built on the device (C ABI in include/gingr_hip.h: gingr_model_from_shapes) -- what a
// scalismo user gets from DataCollection.gpa(...) followed by PointDistributionModel.createUsingPCA(...).
//   alignment     0 none; 1 every shape rigidly onto the reference (Kabsch, no scale); 2 generalised Procrustes: sweeps of "align all
//                 to the target, target := mean of the aligned shapes" from target = reference
//   mu            mean shape; the model's mean displacement is mu - reference (mode 2: the reference is the final target)
//   Xc            [3M][n] = (X_i - mu) / sqrt(n - 1), written straight into the basis layout of a model (the "raw" model)
//   Xc^T Xc       = V diag(lambda) V^T: the raw model's moment S_tot (launch_gram) and the solvers of eig.hip.  A centred Gram matrix is
//                 singular (its columns sum to zero, often with a larger null space), so they decompose Xc^T Xc + (trace / n) I
//   Q0            = Xc V[:, :k] = U sqrt(lambda) (launch_basis_rotate, identity rotation), variance lambda[:k]
// The shifted eigen step, the factor rows and the moment trace are the shared tail of posterior_model.hip (gp.h), the choice of k is
// spectrum_plan.h, the finite checks and the staged upload are model.hip's (gp.h).
// Every sum is taken in a fixed order (block partials combined by one thread or one workgroup, no float atomics): two builds of the
// same input give the same bits.
#include "fitter.h"
#include "spectrum_plan.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kAlignThreads = 256;
constexpr int kAlignSums = 15;        // sum x [3], sum t [3], sum t x^T [9] (both clouds relative to c0)
constexpr int kAlignRowsPerChunk = 2048;
constexpr int kAlignMaxChunks = 128;
constexpr int kRigidDoubles = 16;     // per shape: R [9] row-major, centroid of the shape [3], centroid of the target [3], pad

// shape i, plane d of the resident shapes: X + (3 i + d) M (the Cloud layout per shape, caller's point order)
__device__ __forceinline__ const double *plane(const double *X, int64_t M, int i, int d) { return X + ((int64_t)3 * i + d) * M; }

// Block (c, i): the kAlignSums sums of shape i against the target over the rows of chunk c, into part[(i * chunks + c) * kAlignSums].
// Inside the block: every thread its rows in ascending order, a butterfly over the wave, the four waves added in order by thread 0.
__global__ __launch_bounds__(kAlignThreads) void align_partials_kernel(const double *__restrict__ X, const double *__restrict__ tgt, int64_t M,
                                                                       int64_t rows_per_chunk, double c0x, double c0y, double c0z,
                                                                       double *__restrict__ part) {
    __shared__ double sh[kAlignThreads / 64][kAlignSums];
    const int i = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = (int64_t)c * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    const double *px = plane(X, M, i, 0), *py = plane(X, M, i, 1), *pz = plane(X, M, i, 2);
    double s[kAlignSums];
#pragma unroll
    for (int q = 0; q < kAlignSums; ++q) s[q] = 0.0;
    for (int64_t m = r0 + tid; m < r1; m += kAlignThreads) {
        const double x[3] = {px[m] - c0x, py[m] - c0y, pz[m] - c0z};
        const double t[3] = {tgt[m] - c0x, tgt[M + m] - c0y, tgt[2 * M + m] - c0z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] += x[a];
            s[3 + a] += t[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[6 + 3 * a + b] = __builtin_fma(t[a], x[b], s[6 + 3 * a + b]);
        }
    }
#pragma unroll
    for (int q = 0; q < kAlignSums; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kAlignSums; ++q) sh[tid >> 6][q] = s[q];
    }
    __syncthreads();
    if (tid < kAlignSums) {
        double acc = sh[0][tid];
        for (int w = 1; w < kAlignThreads / 64; ++w) acc += sh[w][tid];
        part[((int64_t)i * gridDim.x + c) * kAlignSums + tid] = acc;
    }
}

// One thread per shape: the chunk partials in ascending order, then Kabsch -- centroids, the cross-covariance sum t x^T / M - mu_t mu_x^T,
// its Kabsch rotation (kabsch3_rotation, svd3.h: the polar factor or, where that does not apply, the SVD with the last singular vector
// flipped when the determinant is negative -- the convention of rigid_transform_kernel, rigid_icp.hip).  rigid[i] = {R, centroid of the shape,
// centroid of the target}: the aligned point is R (x - cx) + ct.
__global__ __launch_bounds__(64) void align_finish_kernel(const double *__restrict__ part, int n, int chunks, int64_t M, double c0x, double c0y,
                                                          double c0z, double *__restrict__ rigid) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double s[kAlignSums];
    for (int q = 0; q < kAlignSums; ++q) s[q] = 0.0;
    for (int c = 0; c < chunks; ++c)
        for (int q = 0; q < kAlignSums; ++q) s[q] += part[((int64_t)i * chunks + c) * kAlignSums + q];
    const double inv = 1.0 / (double)M;
    double mux[3], mut[3], S[9];
    for (int a = 0; a < 3; ++a) {
        mux[a] = s[a] * inv;
        mut[a] = s[3 + a] * inv;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S[3 * a + b] = s[6 + 3 * a + b] * inv - mut[a] * mux[b];
    double R[9], tr = 0.0;
    kabsch3_rotation(S, R, &tr);
    double *o = rigid + (int64_t)i * kRigidDoubles;
    for (int q = 0; q < 9; ++q) o[q] = R[q];
    const double c0[3] = {c0x, c0y, c0z};
    for (int a = 0; a < 3; ++a) {
        o[9 + a] = mux[a] + c0[a];
        o[12 + a] = mut[a] + c0[a];
    }
    o[15] = 0.0;
}

// Thread m: X_i[m] = R_i (X_i[m] - cx_i) + ct_i for every shape in ascending order, in place.  update_target: the mean of the aligned
// points becomes target[m], and the block's sum of |new - old|^2 goes to change_part[block] (tree over the block in a fixed shape).
__global__ __launch_bounds__(256) void align_apply_kernel(double *__restrict__ X, int n, int64_t M, const double *__restrict__ rigid,
                                                          int update_target, double *__restrict__ tgt, double *__restrict__ change_part) {
    __shared__ double sh[256];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
    if (m < M) {
        for (int i = 0; i < n; ++i) {
            const double *g = rigid + (int64_t)i * kRigidDoubles;
            double *px = X + ((int64_t)3 * i) * M + m, *py = px + M, *pz = py + M;
            const double x = *px - g[9], y = *py - g[10], z = *pz - g[11];
            const double ax = __builtin_fma(g[0], x, __builtin_fma(g[1], y, g[2] * z)) + g[12];
            const double ay = __builtin_fma(g[3], x, __builtin_fma(g[4], y, g[5] * z)) + g[13];
            const double az = __builtin_fma(g[6], x, __builtin_fma(g[7], y, g[8] * z)) + g[14];
            *px = ax;
            *py = ay;
            *pz = az;
            acc[0] += ax;
            acc[1] += ay;
            acc[2] += az;
        }
        if (update_target) {
            const double inv = 1.0 / (double)n;
            for (int d = 0; d < 3; ++d) {
                const double nt = acc[d] * inv, diff = nt - tgt[d * M + m];
                d2 = __builtin_fma(diff, diff, d2);
                tgt[d * M + m] = nt;
            }
        }
    }
    if (!update_target) return;
    sh[threadIdx.x] = d2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) change_part[blockIdx.x] = sh[0];
}

// out[0] = sqrt(sum of the block partials / M): the RMS distance per point between successive targets; one workgroup, fixed order
__global__ __launch_bounds__(256) void gpa_change_kernel(const double *__restrict__ change_part, int nblocks, int64_t M, double *__restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += change_part[b];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sqrt(sh[0] / (double)M);
}

// mu[e] = (sum_i X_i[e]) / n over the 3 M plane entries e, shapes in ascending order; mu_aos (caller's order, interleaved) for the host
__global__ __launch_bounds__(256) void shape_mean_kernel(const double *__restrict__ X, int n, int64_t M, double *__restrict__ mu,
                                                         double *__restrict__ mu_aos) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * M) return;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += X[(int64_t)3 * i * M + e];
    const double v = acc / (double)n;
    mu[e] = v;
    const int64_t d = e / M, m = e - d * M;
    mu_aos[3 * m + d] = v;
}

constexpr int kPackVerts = 64;  // vertices of a tile (one wave reads 512 contiguous bytes of a shape plane)
constexpr int kPackCols = 64;   // shapes of a tile (one wave writes 512 contiguous bytes of a basis row)

// Q[3 iperm[m] + d][j] = (X_j[d][m] - mu[d][m]) scale for j < n, 0 for n <= j < np.  Block (b, d): the vertices [64 b, 64 b + 64) in the
// CALLER's order, 64 shapes at a time through LDS: the reads run along a shape plane (a wave = one shape, 64 consecutive vertices),
// the writes along a basis row (a wave = 64 consecutive columns of one row: whole cache lines, np is a multiple of 16); the row
// permutation only decides which row a write goes to.  The tile is padded to 65 columns: the transposed reads of a wave (stride 65
// doubles) fall into different banks.
__global__ __launch_bounds__(256) void center_pack_kernel(const double *__restrict__ X, const double *__restrict__ mu, int n, int np, int64_t M,
                                                          double scale, const int32_t *__restrict__ iperm, double *__restrict__ Q) {
    __shared__ double tile[kPackCols][kPackVerts + 1];
    __shared__ int64_t row[kPackVerts];
    const int d = blockIdx.y, tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * kPackVerts;
    const int v = tid & 63;
    const bool live = m0 + v < M;
    const double mean = live ? mu[(int64_t)d * M + m0 + v] : 0.0;
    if (tid < kPackVerts) row[tid] = live ? (int64_t)3 * iperm[m0 + tid] + d : -1;
    for (int j0 = 0; j0 < np; j0 += kPackCols) {
        __syncthreads();
        for (int jj = tid >> 6; jj < kPackCols; jj += 4) {
            const int j = j0 + jj;
            tile[jj][v] = (live && j < n) ? (plane(X, M, j, d)[m0 + v] - mean) * scale : 0.0;
        }
        __syncthreads();
        const int jj = tid & 63, j = j0 + jj;
        if (j < np)
            for (int vv = tid >> 6; vv < kPackVerts; vv += 4)
                if (row[vv] >= 0) Q[row[vv] * np + j] = tile[jj][vv];
    }
}

// Gs [n][n] = the leading n x n block of G (row stride ldg) + shift on the diagonal
__global__ __launch_bounds__(256) void gram_shift_kernel(const double *__restrict__ G, int ldg, int n, double shift, double *__restrict__ Gs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    Gs[e] = G[(int64_t)i * ldg + j] + (i == j ? shift : 0.0);
}

// the pinned-flag read-back of the fitter (pull_small, fitter.hip) without a fitter: eight pinned words (the last one the flag) and the
// read-back kernel's workgroup counter
struct SmallPull {
    gingr_ctx *ctx = nullptr;
    PinnedWords w;
    SmallPull() = default;
    SmallPull(const SmallPull &) = delete;
    SmallPull &operator=(const SmallPull &) = delete;
    ~SmallPull() {
        if (w.pin) (void)hipHostFree(w.pin);
        dev_free(w.done);
    }
    int init(gingr_ctx *c) {
        ctx = c;
        w.pin_doubles = 8;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&w.pin), w.pin_doubles * sizeof(double), hipHostMallocDefault));
        GINGR_TRY(dev_alloc(ctx, &w.done, 1));
        w.pin[w.pin_doubles - 1] = 0.0;
        if (hipMemset(w.done, 0, sizeof(int32_t)) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void **>(&w.pin_dev), w.pin, 0) != hipSuccess) {
            (void)hipGetLastError();
            w.pin_dev = nullptr;  // (pull_small then copies and synchronises)
        }
        return GINGR_OK;
    }
    int pull(const double *src, double *value) {
        GINGR_TRY(pull_small(ctx, w, src, 1, w.pin));
        *value = w.pin[0];
        return GINGR_OK;
    }
};

}  // namespace

extern "C" {

int gingr_model_from_shapes(gingr_ctx *ctx, int64_t M, int32_t n_shapes, const double *ref_xyz, const double *shapes_xyz, int32_t alignment,
                            int32_t gpa_max_iterations, double gpa_tolerance, double relative_tolerance, int32_t max_rank, gingr_model **out,
                            gingr_pca_info *info) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    const char *who = "model_from_shapes";
    if (!ref_xyz || !shapes_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (n_shapes < 2 || n_shapes > 512)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d shapes, need 2 <= n_shapes <= 512", who, (int)n_shapes);
    if (M < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld < 1", who, (long long)M);
    if (alignment < 0 || alignment > 2)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: alignment %d (0 none, 1 rigid to the reference, 2 generalised Procrustes)", who,
                               (int)alignment);
    if (max_rank < 0 || !(relative_tolerance >= 0.0) || !(gpa_tolerance >= 0.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: max_rank, relative_tolerance and gpa_tolerance must not be negative", who);
    if (M > (int64_t)0x7fffffff / 3) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld too large", who, (long long)M);
    const int n = n_shapes;
    GINGR_TRY(check_finite(ctx, ref_xyz, 3 * M, 1, who, "reference"));
    GINGR_TRY(check_finite(ctx, shapes_xyz, 3 * M, n, who, "shape"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int np = (int)round_up(n, 16);
    const int sweeps_max = gpa_max_iterations > 0 ? gpa_max_iterations : 3;

    // ---- 1. the shapes as planes on the device (for_each_shape_stage, model.hip; the staging buffer serves step 3 once more)
    DevBuf X, stage, tgt, mu, aos;
    HIP_TRY(ctx, X.alloc((size_t)n * 3 * M * sizeof(double)));
    HIP_TRY(ctx, tgt.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, mu.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, aos.alloc((size_t)3 * M * sizeof(double)));
    GINGR_TRY(for_each_shape_stage(ctx, M, n, shapes_xyz, stage, [&](int cnt, int i0) -> int {
        for (int q = 0; q < cnt; ++q)
            launch_aos_to_soa(ctx, stage.as<double>() + (size_t)q * 3 * M, M, X.as<double>() + (size_t)(i0 + q) * 3 * M);
        return GINGR_OK;
    }));
    HIP_TRY(ctx, hipMemcpyAsync(aos.p, ref_xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos.as<double>(), M, tgt.as<double>());
    GINGR_TRY(check_launch(ctx));

    // ---- 2. alignment
    int sweeps = 0;
    double last_change = 0.0;
    if (alignment != 0) {
        double c0[3] = {0, 0, 0};  // both clouds are summed relative to the reference's centroid (the sums of products keep their digits)
        for (int64_t i = 0; i < M; ++i)
            for (int d = 0; d < 3; ++d) c0[d] += ref_xyz[3 * i + d];
        for (int d = 0; d < 3; ++d) c0[d] /= (double)M;
        const int chunks = (int)std::min<int64_t>(kAlignMaxChunks, ceil_div(M, kAlignRowsPerChunk));
        const int64_t rows_per_chunk = ceil_div(M, chunks);
        const int ablocks = (int)ceil_div(M, 256);
        DevBuf part, rigid, cpart, change;
        SmallPull pull;
        HIP_TRY(ctx, part.alloc((size_t)n * chunks * kAlignSums * sizeof(double)));
        HIP_TRY(ctx, rigid.alloc((size_t)n * kRigidDoubles * sizeof(double)));
        HIP_TRY(ctx, cpart.alloc((size_t)ablocks * sizeof(double)));
        HIP_TRY(ctx, change.alloc(sizeof(double)));
        GINGR_TRY(pull.init(ctx));
        const int todo = alignment == 1 ? 1 : sweeps_max;
        for (int sweep = 0; sweep < todo; ++sweep) {
            hipLaunchKernelGGL(align_partials_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(kAlignThreads), 0, ctx->stream, X.as<double>(),
                               tgt.as<double>(), M, rows_per_chunk, c0[0], c0[1], c0[2], part.as<double>());
            hipLaunchKernelGGL(align_finish_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, ctx->stream, part.as<double>(), n, chunks, M,
                               c0[0], c0[1], c0[2], rigid.as<double>());
            hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)ablocks), dim3(256), 0, ctx->stream, X.as<double>(), n, M, rigid.as<double>(),
                               alignment == 2 ? 1 : 0, tgt.as<double>(), cpart.as<double>());
            GINGR_TRY(check_launch(ctx));
            if (alignment == 2) {
                hipLaunchKernelGGL(gpa_change_kernel, dim3(1), dim3(256), 0, ctx->stream, cpart.as<double>(), ablocks, M, change.as<double>());
                GINGR_TRY(check_launch(ctx));
                GINGR_TRY(pull.pull(change.as<double>(), &last_change));
                ++sweeps;
                if (!std::isfinite(last_change)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Procrustes target", who);
                if (last_change < gpa_tolerance) break;
            }
        }
    }

    // ---- 3. mean shape; reference and mean displacement of the model pass through the host once (they fix its row order)
    std::vector<double> href((size_t)3 * M), hmean((size_t)3 * M);
    hipLaunchKernelGGL(shape_mean_kernel, dim3((unsigned)ceil_div(3 * M, 256)), dim3(256), 0, ctx->stream, X.as<double>(), n, M, mu.as<double>(),
                       aos.as<double>());
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(hmean.data(), aos.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (alignment == 2) {
        launch_soa_to_aos(ctx, tgt.as<double>(), M, stage.as<double>());
        GINGR_TRY(check_launch(ctx));
        HIP_TRY(ctx, hipMemcpyAsync(href.data(), stage.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (alignment != 2) std::copy(ref_xyz, ref_xyz + 3 * M, href.begin());
    double mu_sq = 0.0;
    for (int64_t e = 0; e < 3 * M; ++e) {
        if (!std::isfinite(hmean[(size_t)e])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite mean shape", who);
        mu_sq += hmean[(size_t)e] * hmean[(size_t)e];
        hmean[(size_t)e] -= href[(size_t)e];
    }

    // ---- 4. the centred data as the basis of a raw model of n columns: its moment S_tot is the Gram matrix Xc^T Xc
    gingr_model *raw = nullptr;
    struct RawGuard {
        gingr_model *&m;
        ~RawGuard() { gingr_model_destroy(m); }
    } raw_guard{raw};
    {
        const std::vector<double> ones((size_t)n, 1.0);
        auto fill = [&](gingr_model *m) -> int {
            hipLaunchKernelGGL(center_pack_kernel, dim3((unsigned)ceil_div(M, kPackVerts), 3), dim3(256), 0, ctx->stream, X.as<double>(),
                               mu.as<double>(), n, np, M, 1.0 / std::sqrt((double)(n - 1)), m->iperm, m->Q0);
            return check_launch(ctx);
        };
        GINGR_TRY(model_create_impl(ctx, M, n, href.data(), hmean.data(), ones.data(), 0, M, fill, &raw, false));
    }
    // (model_create_impl synchronised: the shapes are not read again)
    X.release();
    stage.release();
    const double *G = raw->mom + MomentLayout{raw->rp}.stot();
    double trace = 0.0;
    GINGR_TRY(moment_trace(ctx, G, n, np, &trace));
    if (!std::isfinite(trace)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Gram matrix of the centred shapes", who);
    // identical shapes leave the rounding of the mean behind: the n - 1 additions of shape_mean_kernel and its division move an entry
    // by at most n (eps / 2) |mu_e|, so the trace, n / (n - 1) sum_e (x_e - mu_e)^2, stays below n^2 eps^2 |mu|^2 / 2.  A total
    // variance within that bound (or within 64 eps^2 |mu|^2 for the smallest n) is no variance.
    const double eps = 2.220446049250313e-16;
    if (!(trace > (64.0 + (double)n * n) * eps * eps * mu_sq))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: all shapes are identical (rank 0)", who);

    // ---- 5. Xc^T Xc = V diag(lambda) V^T, lambda descending.  A centred Gram matrix is singular -- its columns sum to zero, and n shapes
    // drawn from a model of rank r < n - 1 (a chain's samples) or of fewer than n - 1 coordinates leave a null space of several
    // dimensions.  The Cholesky-based kernels of eig.hip hand such a matrix to the two-sided kernel, whose rotation threshold is
    // relative to the two diagonal entries: inside a null space of more than one dimension those are rounding noise themselves and
    // the sweeps need not end (n = 20 shapes of 5 points: no convergence in 60 sweeps).  So the solvers get Xc^T Xc + shift I with
    // shift = trace / n, the mean eigenvalue: the same eigenvectors, every eigenvalue moved by exactly the shift, condition number at
    // most n + 1 -- the positive definite input the fast kernels are built for, with the two-sided one still behind them.  The
    // eigenvalues come back within eps (lambda_1 + shift) <= 2 eps lambda_1 in absolute terms, which is all the Gram route had to
    // offer for the small ones anyway.
    const double shift = trace / (double)n;
    DevBuf evals, V, T, Gs;
    HIP_TRY(ctx, evals.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, V.alloc((size_t)n * n * sizeof(double)));
    HIP_TRY(ctx, Gs.alloc((size_t)n * n * sizeof(double)));
    hipLaunchKernelGGL(gram_shift_kernel, dim3((unsigned)ceil_div((int64_t)n * n, 256)), dim3(256), 0, ctx->stream, G, np, n, shift, Gs.as<double>());
    GINGR_TRY(check_launch(ctx));
    std::vector<double> lam;
    GINGR_TRY(eig_descending_to_host(ctx, Gs.as<double>(), n, n, shift, who, "eigenvalue", evals.as<double>(), V.as<double>(), lam));
    // centred shapes span at most n - 1 directions (lam is un-shifted already: the cut subtracts nothing more)
    const spectrum_plan::Cut cut = spectrum_plan::cut(lam.data(), n, 0.0, n - 1, max_rank, relative_tolerance);
    const int k = cut.k;
    if (k < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: all shapes are identical (rank 0)", who);

    // ---- 6. Q0 = Xc V[:, :k] into the model proper
    const int kp = (int)round_up(k, 16);
    HIP_TRY(ctx, T.alloc((size_t)np * kp * sizeof(double)));
    launch_factor_rows(ctx, V.as<double>(), n, 0, n, np, k, kp, T.as<double>());
    GINGR_TRY(check_launch(ctx));
    const Rot3 identity{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    auto fill = [&](gingr_model *nm) -> int {
        launch_basis_rotate(ctx, raw, T.as<double>(), identity, nm);
        return check_launch(ctx);
    };
    GINGR_TRY(model_create_impl(ctx, M, k, href.data(), hmean.data(), lam.data(), 0, M, fill, out));
    if (info) {
        info->rank = k;
        info->gpa_sweeps = sweeps;
        info->gpa_last_change = last_change;
        info->total_variance = cut.total;
        info->kept_variance = cut.kept;
    }
    return GINGR_OK;
}

}  // extern "C"
