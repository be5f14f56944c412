// The kernel extension (model_extend.h): a kernel-built model at points off its reference.
//   gingr_model_extend       Q(x)[d, :] = kvec_d(x) C_d for M_new points, written straight into the new model's Q0
//   gingr_model_warp_points  s (R (x + u(x) - c) + c + t),  u(x)[d] = kvec_d(x) (C_d alpha): no basis of the points is formed
// kvec_d(x)[j] = k_d(x, p_{d,j}) is the build's own kernel value (gpmm_kernel_value.h) with x in the place of the non-pivot argument.
//
// The extension pass is a GEMM whose left operand is evaluated, not loaded.  A wave owns 16 points, the rows of a 16x16x4 float64 MFMA
// tile (accumulator layout and whole-cache-line store as basis_rotate.h has them): per step of four pivots every lane evaluates ONE kernel
// value -- lane l the pair (point l & 15, pivot j0 + (l >> 4)) -- which is the A operand; B is C_d, read from L2.  With one kernel for
// the three coordinates the value feeds all three products.  A wave keeps a chunk of 64 columns (3 x 4 accumulator tiles) in VGPRs; the
// chunks of wider models are dealt to different workgroups (grid.y), which evaluate the kernel again.  The pivots are summed in pivot
// order, four per MFMA, whatever the number of points: a point's row depends on nothing but the point, and there are no atomics.
#include "model_extend.h"

#include "gp_device.h"
#include "gpmm_kernel_value.h"
#include "kernel_warp_plan.h"
#include "model_extend_plan.h"

#include <algorithm>
#include <cmath>

namespace {

namespace ep = model_extend_plan;
using gpmm_factor::kKernelRadial;

__device__ __forceinline__ double ext_value(const ExtKernel &k, double cx, double cy, double cz, double px, double py, double pz, const double *T) {
    if (k.spec.kind == kKernelRadial) return gpmm_factor::radial_value_xyz(k.spec.mix, k.family, cx, cy, cz, px, py, pz, T);
    return gpmm_factor::kspec_value_xyz(k.spec, cx, cy, cz, px, py, pz, T);
}

// what the passes read, by value
struct ExtDev {
    ExtKernel k[3];
    const double *P[3];  // [3][np]
    const double *C[3];  // [np][rp]
    int32_t n[3];
    int32_t np;
};

// ---- the build's gather: LPt[c n + i] = L[c][pivot i], pxyz[a n + i] = coordinate a of pivot i's point
__global__ __launch_bounds__(256) void ext_gather_kernel(const double *__restrict__ L, int64_t N, const int32_t *__restrict__ pivots, int32_t n,
                                                         int generic, Cloud pts, double *__restrict__ LPt, double *__restrict__ pxyz) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int32_t c = (int32_t)(idx / n), i = (int32_t)(idx - (int64_t)c * n);
    const int32_t e = pivots[i];
    LPt[idx] = L[(int64_t)c * N + e];
    if (c == 0) {
        const int64_t pt = generic ? e / 3 : e;
        pxyz[i] = pts.x[pt];
        pxyz[n + i] = pts.y[pt];
        pxyz[2 * n + i] = pts.z[pt];
    }
}

// ---- forming one coordinate: its pivots' coordinates, its triangle of the factor, the right-hand side V_d in the model's columns.
// ord [nd]: the coordinate's pivots as ordinals of the build's sequence; wcol [rp]: the eigenvector of model column q, -1: none;
// vrow(i) = shared ? i : ord[i] is the eigenvector's component of pivot i.  P [3][np], LP [nd][nd], W [np][rp]; rows past nd are zero.
__global__ __launch_bounds__(256) void ext_form_kernel(const double *__restrict__ LPt, const double *__restrict__ pxyz, int32_t n,
                                                       const int32_t *__restrict__ ord, int32_t nd, int32_t np, const double *__restrict__ V,
                                                       int32_t vstride, int vrow_is_ord, const int32_t *__restrict__ wcol, int32_t rp,
                                                       double *__restrict__ P, double *__restrict__ LP, double *__restrict__ W) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < 3 * (int64_t)np) {
        const int a = (int)(idx / np), j = (int)(idx - (int64_t)a * np);
        P[idx] = j < nd ? pxyz[(int64_t)a * n + ord[j]] : 0.0;
    }
    if (idx < (int64_t)nd * nd) {
        const int i = (int)(idx / nd), j = (int)(idx - (int64_t)i * nd);
        LP[idx] = j <= i ? LPt[(int64_t)ord[j] * n + ord[i]] : 0.0;
    }
    if (idx < (int64_t)np * rp) {
        const int i = (int)(idx / rp), q = (int)(idx - (int64_t)i * rp);
        double v = 0.0;
        if (i < nd && wcol[q] >= 0) v = V[(int64_t)(vrow_is_ord ? ord[i] : i) * vstride + wcol[q]];
        W[idx] = v;
    }
}

// C <- LP^-T C: the back substitution of L_P^T C = V, one thread per column, rows from the last pivot to the first, the sum of a row in
// ascending order.  One-off per model.
__global__ __launch_bounds__(64) void ext_backsolve_kernel(const double *__restrict__ LP, int32_t nd, int32_t rp, double *__restrict__ C) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= rp) return;
    for (int j = nd - 1; j >= 0; --j) {
        double s = C[(int64_t)j * rp + q];
        for (int i = j + 1; i < nd; ++i) s = __builtin_fma(-LP[(int64_t)i * nd + j], C[(int64_t)i * rp + q], s);
        C[(int64_t)j * rp + q] = s / LP[(int64_t)j * nd + j];
    }
}

// Cn[i][q] = q < k ? Cs[i][q] : 0   (gingr_model_truncate)
__global__ __launch_bounds__(256) void ext_cut_kernel(const double *__restrict__ Cs, int32_t rps, int32_t rows, int32_t k, int32_t rpn,
                                                      double *__restrict__ Cn) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * rpn) return;
    const int i = (int)(idx / rpn), q = (int)(idx - (int64_t)i * rpn);
    Cn[idx] = q < k ? Cs[(int64_t)i * rps + q] : 0.0;
}

// ---- the extension pass.  grid (point_blocks, chunks); Z: the new points in the new model's row order; Q0 [3 Z.n][rp].
template <bool SHARED>
__global__ __launch_bounds__(64 * ep::kWaves) void extend_kernel(Cloud Z, ExtDev e, int32_t rp, double *__restrict__ Q0) {
    __shared__ double T[GINGR_EXP_TABLE];
    fastexp_table_init(T);
    __syncthreads();
    constexpr int NT = ep::kChunkTiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const int64_t v0 = ((int64_t)blockIdx.x * ep::kWaves + wave) * ep::kWaveRows;
    if (v0 >= Z.n) return;
    const int64_t pi = v0 + cl < Z.n ? v0 + cl : Z.n - 1;  // (a lane past the end evaluates a copy of the last point; its rows are not stored)
    const double x = Z.x[pi], y = Z.y[pi], z = Z.z[pi];
    const int n0 = blockIdx.y * ep::kChunkCols;
    const int nt = (rp - n0) / 16 < NT ? (rp - n0) / 16 : NT;  // tiles of this chunk (workgroup-uniform)
    const int np = e.np;
    v4f64 acc[3][NT];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[d][t] = v4f64{0, 0, 0, 0};
    if (SHARED) {
        const double *Px = e.P[0];
        for (int j0 = 0; j0 < e.n[0]; j0 += ep::kPivotStep) {  // n[0] >= n[1] >= n[2]: prefixes of one pivot sequence
            const int j = j0 + kq;                             // (< np: the lists are padded, the rows of C behind n[d] are zero)
            const double kv = ext_value(e.k[0], x, y, z, Px[j], Px[np + j], Px[2 * np + j], T);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double a = j < e.n[d] ? kv : 0.0;
                const double *crow = e.C[d] + (int64_t)j * rp + n0 + cl;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < nt) acc[d][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, crow[16 * t], acc[d][t], 0, 0, 0);
            }
        }
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double *Px = e.P[d];
            for (int j0 = 0; j0 < e.n[d]; j0 += ep::kPivotStep) {
                const int j = j0 + kq;
                const double kv = ext_value(e.k[d], x, y, z, Px[j], Px[np + j], Px[2 * np + j], T);
                const double a = j < e.n[d] ? kv : 0.0;
                const double *crow = e.C[d] + (int64_t)j * rp + n0 + cl;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < nt) acc[d][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, crow[16 * t], acc[d][t], 0, 0, 0);
            }
        }
    }
    // D: the lane holds column cl of the rows kq + 4 g.  For one register and tile the 16 lanes of a row of lanes write 128 contiguous,
    // 128-byte aligned bytes of one result row (rp is a multiple of 16): every store instruction fills whole cache lines.
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int64_t v = v0 + kq + 4 * g;
        if (v >= Z.n) continue;
        double *orow = Q0 + 3 * v * rp + n0 + cl;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) orow[(int64_t)d * rp + 16 * t] = acc[d][t][g];
    }
}

// ---- the warp: w[d][j] = sum_q C_d[j][q] alpha[q] (ascending q), then one thread per point
__global__ __launch_bounds__(256) void ext_coeff_kernel(ExtDev e, int32_t r, int32_t rp, const double *__restrict__ alpha, double *__restrict__ w) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * e.np) return;
    const int d = idx / e.np, j = idx - d * e.np;
    double s = 0.0;
    if (j < e.n[d])
        for (int q = 0; q < r; ++q) s = __builtin_fma(e.C[d][(int64_t)j * rp + q], alpha[q], s);
    w[idx] = s;
}

struct WarpPose {
    double R[9], c[3], t[3], s;
};

// z_p <- s (R (z_p + u(z_p) - c) + c + t) in place (planes of stride n); the arithmetic of the pose as the fitters' sweep has it
template <bool SHARED>
__global__ __launch_bounds__(256) void ext_warp_kernel(int64_t n, double *__restrict__ zz, ExtDev e, const double *__restrict__ w, WarpPose pose) {
    __shared__ double T[GINGR_EXP_TABLE];
    fastexp_table_init(T);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = zz[p], y = zz[n + p], z = zz[2 * n + p];
    const int np = e.np;
    double u[3] = {0.0, 0.0, 0.0};
    if (SHARED) {
        const double *Px = e.P[0];
        for (int j = 0; j < e.n[0]; ++j) {
            const double kv = ext_value(e.k[0], x, y, z, Px[j], Px[np + j], Px[2 * np + j], T);
#pragma unroll
            for (int d = 0; d < 3; ++d) u[d] = __builtin_fma(kv, w[d * np + j], u[d]);  // (w is zero behind n[d])
        }
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double *Px = e.P[d];
            for (int j = 0; j < e.n[d]; ++j)
                u[d] = __builtin_fma(ext_value(e.k[d], x, y, z, Px[j], Px[np + j], Px[2 * np + j], T), w[d * np + j], u[d]);
        }
    }
    const double ix = x + u[0] - pose.c[0], iy = y + u[1] - pose.c[1], iz = z + u[2] - pose.c[2];
    const double *R = pose.R;
    zz[p] = pose.s * (R[0] * ix + R[1] * iy + R[2] * iz + pose.c[0] + pose.t[0]);
    zz[n + p] = pose.s * (R[3] * ix + R[4] * iy + R[5] * iz + pose.c[1] + pose.t[1]);
    zz[2 * n + p] = pose.s * (R[6] * ix + R[7] * iy + R[8] * iz + pose.c[2] + pose.t[2]);
}

// ---- host
int upload_ints(gingr_ctx *ctx, const std::vector<int32_t> &h, DevBuf &d) {
    HIP_TRY(ctx, d.alloc(std::max<size_t>(h.size(), 1) * sizeof(int32_t)));
    if (!h.empty()) HIP_TRY(ctx, hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return GINGR_OK;
}

// the per-coordinate lists and C from the build's raw material, once
int form(gingr_ctx *ctx, KernelExtension &x) {
    if (x.formed) return GINGR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t n = x.n, rp = x.rp;
    std::vector<int32_t> hp((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(hp.data(), x.pivots, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const ep::Lists lists = ep::pivot_lists(hp.data(), n, !x.shared, x.cnt);
    int32_t most = 0;
    for (int d = 0; d < 3; ++d) {
        x.cnt[d] = (int32_t)lists.ord[d].size();
        x.ids[d] = lists.ids[d];
        most = std::max(most, x.cnt[d]);
    }
    x.np = ep::padded(most);
    DevBuf ord[3], wcol[3], LP[3];
    for (int d = 0; d < 3; ++d) {
        const int32_t nd = x.cnt[d];
        std::vector<int32_t> wc((size_t)rp, -1);
        for (int32_t q = 0; q < x.r; ++q)
            if (!x.shared)
                wc[(size_t)q] = q;
            else if (x.qdim[(size_t)q] == d)
                wc[(size_t)q] = x.qidx[(size_t)q];
        GINGR_TRY(upload_ints(ctx, lists.ord[d], ord[d]));
        GINGR_TRY(upload_ints(ctx, wc, wcol[d]));
        HIP_TRY(ctx, x.P[d].alloc((size_t)3 * x.np * sizeof(double)));
        HIP_TRY(ctx, x.C[d].alloc((size_t)x.np * rp * sizeof(double)));
        HIP_TRY(ctx, LP[d].alloc(std::max<size_t>((size_t)nd * nd, 1) * sizeof(double)));
        const int b = x.shared && nd > 0 ? x.block_of[d] : 0;  // (a coordinate without a column has no block)
        const int64_t work = std::max<int64_t>(std::max<int64_t>(3 * (int64_t)x.np, (int64_t)nd * nd), (int64_t)x.np * rp);
        hipLaunchKernelGGL(ext_form_kernel, dim3((unsigned)ceil_div(work, 256)), dim3(256), 0, ctx->stream, x.LPt, x.pxyz, n,
                           ord[d].as<int32_t>(), nd, x.np, nd > 0 ? x.V[b] : nullptr, x.vn[b], x.shared ? 0 : 1,
                           wcol[d].as<int32_t>(), rp, x.P[d].as<double>(), LP[d].as<double>(), x.C[d].as<double>());
        if (nd > 0)
            hipLaunchKernelGGL(ext_backsolve_kernel, dim3((unsigned)ceil_div(rp, 64)), dim3(64), 0, ctx->stream, LP[d].as<double>(), nd, rp,
                               x.C[d].as<double>());
    }
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers leave scope
    x.raw.release();
    x.formed = true;
    return GINGR_OK;
}

// the model's extension, formed; a model without one: GINGR_ERR_STATE with the reason
int extension_of(gingr_ctx *ctx, const gingr_model *m, const char *who, KernelExtension **out) {
    if (m->ctx != ctx) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the model belongs to another context", who);
    if (!m->ext) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: the model carries no kernel extension: %s", who, m->ext_missing);
    GINGR_TRY(form(ctx, *m->ext));
    *out = m->ext.get();
    return GINGR_OK;
}

ExtDev device_view(const KernelExtension &x) {
    ExtDev e;
    memset(&e, 0, sizeof(e));
    for (int d = 0; d < 3; ++d) {
        e.k[d] = x.kernel[d];
        e.P[d] = x.P[d].as<double>();
        e.C[d] = x.C[d].as<double>();
        e.n[d] = x.cnt[d];
    }
    e.np = x.np;
    return e;
}

}  // namespace

int kernel_extension_keep(gingr_ctx *ctx, const gpmm_factor::Factor &f, int32_t n, bool generic, const double *const V[3], const int32_t vn[3],
                          KernelExtension &x) {
    x.n = n;
    size_t doubles = (size_t)n * n + (size_t)3 * n;
    for (int b = 0; b < 3; ++b) {
        x.vn[b] = V[b] ? vn[b] : 0;
        doubles += (size_t)x.vn[b] * x.vn[b];
    }
    HIP_TRY(ctx, x.raw.alloc(doubles * sizeof(double) + (size_t)n * sizeof(int32_t)));
    double *at = x.raw.as<double>(), *LPt = at, *pxyz = at + (size_t)n * n;
    at = pxyz + (size_t)3 * n;
    for (int b = 0; b < 3; ++b) {
        if (x.vn[b] < 1) continue;
        HIP_TRY(ctx, hipMemcpyAsync(at, V[b], (size_t)x.vn[b] * x.vn[b] * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        x.V[b] = at;
        at += (size_t)x.vn[b] * x.vn[b];
    }
    int32_t *piv = reinterpret_cast<int32_t *>(at);
    HIP_TRY(ctx, hipMemcpyAsync(piv, f.pivots.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(ext_gather_kernel, dim3((unsigned)ceil_div((int64_t)n * n, 256)), dim3(256), 0, ctx->stream, f.Lb.as<double>(), f.n, piv, n,
                       generic ? 1 : 0, f.pts, LPt, pxyz);
    x.LPt = LPt, x.pxyz = pxyz, x.pivots = piv;
    return check_launch(ctx);
}

int kernel_extension_truncate(gingr_ctx *ctx, const gingr_model *src, int32_t k, std::shared_ptr<KernelExtension> *out) {
    out->reset();
    if (!src->ext) return GINGR_OK;
    GINGR_TRY(form(ctx, *src->ext));
    const KernelExtension &s = *src->ext;
    auto x = std::make_shared<KernelExtension>();
    x->shared = s.shared, x->r = k, x->rp = (int32_t)round_up(k, 16), x->np = s.np, x->formed = true;
    for (int d = 0; d < 3; ++d) {
        x->kernel[d] = s.kernel[d], x->cnt[d] = s.cnt[d], x->ids[d] = s.ids[d];
        HIP_TRY(ctx, x->P[d].alloc((size_t)3 * s.np * sizeof(double)));
        HIP_TRY(ctx, x->C[d].alloc((size_t)s.np * x->rp * sizeof(double)));
        HIP_TRY(ctx, hipMemcpyAsync(x->P[d].p, s.P[d].p, (size_t)3 * s.np * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(ext_cut_kernel, dim3((unsigned)ceil_div((int64_t)s.np * x->rp, 256)), dim3(256), 0, ctx->stream, s.C[d].as<double>(), s.rp,
                           s.np, k, x->rp, x->C[d].as<double>());
    }
    GINGR_TRY(check_launch(ctx));
    *out = x;
    return GINGR_OK;
}

extern "C" {

int gingr_model_kernel_extension(const gingr_model *model, int32_t *available, int32_t counts[3], int32_t *shared_kernel) {
    if (!model || !available) return GINGR_ERR_BAD_ARGUMENT;
    *available = model->ext ? 1 : 0;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (shared_kernel) *shared_kernel = 0;
    if (!model->ext) return GINGR_OK;
    // a pure query where the counts are known from the build (one kernel for the three coordinates, or formed already); the pivots per
    // coordinate of a generic factorisation are only counted when the extension is formed, which can fail like any device work
    if (!model->ext->shared && !model->ext->formed) GINGR_TRY(form(model->ctx, *model->ext));
    if (counts)
        for (int d = 0; d < 3; ++d) counts[d] = model->ext->cnt[d];
    if (shared_kernel) *shared_kernel = model->ext->shared ? 1 : 0;
    return GINGR_OK;
}

int gingr_model_get_kernel_extension(gingr_ctx *ctx, const gingr_model *model, int32_t d, int32_t *pivot_ids, double *coeff) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!model || d < 0 || d > 2) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_get_kernel_extension: need a model and a coordinate 0..2");
    KernelExtension *x = nullptr;
    GINGR_TRY(extension_of(ctx, model, "model_get_kernel_extension", &x));
    const int32_t nd = x->cnt[d];
    if (pivot_ids) std::copy(x->ids[d].begin(), x->ids[d].end(), pivot_ids);
    if (coeff && nd > 0) {
        std::vector<double> h((size_t)nd * x->rp);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), x->C[d].p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int32_t j = 0; j < nd; ++j) std::copy(h.begin() + (size_t)j * x->rp, h.begin() + (size_t)j * x->rp + x->r, coeff + (size_t)j * x->r);
    }
    return GINGR_OK;
}

int gingr_model_extend(gingr_ctx *ctx, const gingr_model *src, int64_t M_new, const double *new_ref_xyz, gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!src || !new_ref_xyz || M_new < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_extend: need a model and M_new >= 1 points");
    KernelExtension *x = nullptr;
    GINGR_TRY(extension_of(ctx, src, "model_extend", &x));
    GINGR_TRY(check_finite(ctx, new_ref_xyz, 3, M_new, "model_extend", "point"));
    const ExtDev e = device_view(*x);
    const std::vector<double> zero_mean((size_t)3 * M_new, 0.0);
    DevBuf stage, Z;
    auto fill = [&](gingr_model *m) -> int {
        const int64_t M = m->M;
        HIP_TRY(ctx, stage.alloc((size_t)3 * M * sizeof(double)));
        HIP_TRY(ctx, Z.alloc((size_t)3 * M * sizeof(double)));
        double *zs = Z.as<double>();
        GINGR_TRY(upload_cloud(ctx, stage.as<double>(), new_ref_xyz, M, zs, m->perm));  // the new model's own row order
        const Cloud Zc{zs, zs + M, zs + 2 * M, M};
        const dim3 grid((unsigned)ep::point_blocks(M), (unsigned)ep::chunks(m->rp));
        hipLaunchKernelGGL(x->shared ? extend_kernel<true> : extend_kernel<false>, grid, dim3(64 * ep::kWaves), 0, ctx->stream, Zc, e, m->rp, m->Q0);
        return check_launch(ctx);
    };
    GINGR_TRY(model_create_impl(ctx, M_new, src->r, new_ref_xyz, zero_mean.data(), src->variance.data(), 0, M_new, fill, out));
    (*out)->ext = src->ext;  // the same pivots and the same C
    return GINGR_OK;
}

int gingr_model_warp_points(gingr_ctx *ctx, const gingr_model *model, const double *alpha, const double euler[3], const double center[3],
                            const double translation[3], double scale, int64_t P, const double *points_xyz, double *out_xyz) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!model || !alpha || !euler || !center || !translation || !points_xyz || !out_xyz || P < 1)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "model_warp_points: need a model, coefficients, a pose and P >= 1 points");
    KernelExtension *x = nullptr;
    GINGR_TRY(extension_of(ctx, model, "model_warp_points", &x));
    GINGR_TRY(check_finite(ctx, points_xyz, 3, P, "model_warp_points", "point"));
    GINGR_TRY(check_finite(ctx, alpha, 1, model->r, "model_warp_points", "coefficient"));
    const ExtDev e = device_view(*x);
    WarpPose pose;
    euler_to_rot(euler, pose.R);
    for (int q = 0; q < 3; ++q) pose.c[q] = center[q], pose.t[q] = translation[q];
    pose.s = scale;
    const kernel_warp_plan::Plan plan = kernel_warp_plan::make_plan(P, 0);  // the slabs of the classic routes' warp, no partial sums
    DevBuf da, w, stage, Z;
    HIP_TRY(ctx, da.alloc((size_t)model->r * sizeof(double)));
    HIP_TRY(ctx, w.alloc((size_t)3 * e.np * sizeof(double) + 8));
    HIP_TRY(ctx, stage.alloc((size_t)plan.cloud_doubles() * sizeof(double)));
    HIP_TRY(ctx, Z.alloc((size_t)plan.cloud_doubles() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(da.p, alpha, (size_t)model->r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (e.np > 0)
        hipLaunchKernelGGL(ext_coeff_kernel, dim3((unsigned)ceil_div(3 * e.np, 256)), dim3(256), 0, ctx->stream, e, model->r, model->rp, da.as<double>(),
                           w.as<double>());
    GINGR_TRY(check_launch(ctx));
    for (int64_t s = 0; s < plan.slabs; ++s) {
        const int64_t p0 = plan.slab_begin(s), n = plan.slab_count(s);
        GINGR_TRY(upload_cloud(ctx, stage.as<double>(), points_xyz + 3 * p0, n, Z.as<double>()));
        hipLaunchKernelGGL(x->shared ? ext_warp_kernel<true> : ext_warp_kernel<false>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, n,
                           Z.as<double>(), e, w.as<double>(), pose);
        GINGR_TRY(check_launch(ctx));
        GINGR_TRY(download_cloud(ctx, stage.as<double>(), Z.as<double>(), n, out_xyz + 3 * p0));
    }
    return GINGR_OK;
}

}  // extern "C"
