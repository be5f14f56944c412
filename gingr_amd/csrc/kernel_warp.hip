// The kernel warp: the fitted map of a classic CPD or BCPD task at points off the template,
//   out_p = A (z_p + sum_m g(z_p, y_m) c_m) + t,   g(a, b) = exp(-|a - b|^2 / (2 beta^2)),
// y the task's original template, c its coefficients (non-rigid CPD: W; BCPD: (c2 / lambda) (r - nu o v^)), A = s L and t the
// linear head (include/gingr_hip.h states the map per kind).  The rigid and affine kinds have no sum: the finish kernel alone.
//
// One streaming pass of the kind of bcpd_colsum_kernel: one thread per query, the centres staged in LDS as 256 records (y_m, c_m) of
// six doubles (a record is read by every lane of a wave at once: three 16-byte broadcasts), float64 throughout, the exponential from
// the 2048-entry table in its round-to-nearest form (fastexp.h, degree 3).  d^2 is formed as gauss_block_kernel forms it -- the
// differences, then the same FMA chain -- so g(y_m', y_m) has the bits of the dense route's G.  Where the queries' and the centres'
// extent could push the exponent's argument out of the table's range the clamped copy of the loop runs (a wave-uniform branch); a
// clamped entry is +0 either way.  17 float64 VALU instructions per pair: 3 differences, 3 for d^2, 8 for the exponential, 3 FMAs.
// No atomics: grid (query tiles, chunks of the centres), three partials per query and chunk, added in chunk order by the finish
// kernel, which also applies the `+ z` and the head.  The chunks are kernel_warp_plan.h's: their boundaries depend on M alone, so a
// query's image does not depend on the other queries of the call, nor on how the call is cut into slabs.
#include "kernel_warp.h"
#include "cloud_sums.h"
#include "fastexp.h"
#include "kernel_warp_plan.h"

#include <cmath>

namespace {

namespace wp = kernel_warp_plan;
constexpr int kTile = (int)wp::kTile;

// part[chunk][d][p] = sum over the chunk's centres of g(z_p, y_m) c_md;  aux = {largest |coordinate| of the queries, of the centres}
__global__ __launch_bounds__(256) void kernel_warp_kernel(Cloud Z, Cloud Y, const double *__restrict__ coeff, int64_t coeff_stride,
                                                          double sigma, const double *__restrict__ aux, int64_t chunk_len,
                                                          double *__restrict__ part) {
    __shared__ double T[GINGR_EXP_TABLE];
    __shared__ double rec[kTile * 6] __attribute__((aligned(16)));
    fastexp_table_init(T);
    const int tid = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kTile + tid, po = p < Z.n ? p : Z.n - 1;  // (a thread past the end computes a copy of the last query)
    const double px = Z.x[po], py = Z.y[po], pz = Z.z[po];
    const double c = fastexp_scale_for_variance(sigma * sigma);  // as gauss_block_kernel, sigma = 2^1/2 beta
    const double am = aux[0] + aux[1];  // 3 am^2 bounds every squared distance between a query and a centre
    const bool clamp = fastexp_needs_clamp(3.0 * am * am, c);  // wave-uniform
    const double lim = fastexp_d2_limit(c);
    const int64_t m0 = (int64_t)blockIdx.y * chunk_len, m1 = m0 + chunk_len < Y.n ? m0 + chunk_len : Y.n;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int64_t mb = m0; mb < m1; mb += kTile) {
        __syncthreads();  // the previous tile has been consumed (first round: nothing to wait for but the table)
        const int64_t m = mb + tid;
        const bool in = m < m1;
        rec[6 * tid] = in ? Y.x[m] : 0.0;
        rec[6 * tid + 1] = in ? Y.y[m] : 0.0;
        rec[6 * tid + 2] = in ? Y.z[m] : 0.0;
        rec[6 * tid + 3] = in ? coeff[m] : 0.0;
        rec[6 * tid + 4] = in ? coeff[coeff_stride + m] : 0.0;
        rec[6 * tid + 5] = in ? coeff[2 * coeff_stride + m] : 0.0;
        __syncthreads();
        const int cnt = (int)(m1 - mb < kTile ? m1 - mb : kTile);  // records past the end are never evaluated
        if (clamp) {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double dx = px - rec[6 * k], dy = py - rec[6 * k + 1], dz = pz - rec[6 * k + 2];
                const double d2 = fastexp_clamp_d2(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)), lim);
                const double e = fastexp2_scaled<3>(d2, c, T);
                ax = __builtin_fma(rec[6 * k + 3], e, ax);
                ay = __builtin_fma(rec[6 * k + 4], e, ay);
                az = __builtin_fma(rec[6 * k + 5], e, az);
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double dx = px - rec[6 * k], dy = py - rec[6 * k + 1], dz = pz - rec[6 * k + 2];
                const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
                const double e = fastexp2_scaled<3>(d2, c, T);
                ax = __builtin_fma(rec[6 * k + 3], e, ax);
                ay = __builtin_fma(rec[6 * k + 4], e, ay);
                az = __builtin_fma(rec[6 * k + 5], e, az);
            }
        }
    }
    if (p < Z.n) {
        double *q = part + (int64_t)blockIdx.y * 3 * Z.n + p;
        q[0] = ax;
        q[Z.n] = ay;
        q[2 * Z.n] = az;
    }
}

// z_p <- A (z_p + the chunk partials in chunk order) + t, in place (planes of stride n).  chunks = 0: no sum; params13 = nullptr: A = I, t = 0.
__global__ __launch_bounds__(256) void kernel_warp_finish_kernel(int64_t n, const double *__restrict__ part, int chunks,
                                                                 const double *__restrict__ params13, double *__restrict__ z) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double u[3] = {z[p], z[n + p], z[2 * n + p]};
    if (chunks > 0) {
        double v[3] = {0, 0, 0};
        for (int ch = 0; ch < chunks; ++ch)
#pragma unroll
            for (int d = 0; d < 3; ++d) v[d] += part[((int64_t)ch * 3 + d) * n + p];
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] += v[d];
    }
    if (params13) {
        double o[3];
        similarity_apply(params13, u[0], u[1], u[2], o);
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] = o[d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) z[d * n + p] = u[d];
}

int grow(gingr_ctx *ctx, DevBuf &b, int64_t doubles) {
    const size_t bytes = (size_t)doubles * sizeof(double);
    if (b.p && b.bytes >= bytes) return GINGR_OK;
    if (b.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();  // (a refused allocation must not surface again in the next call's launch check)
        b.release();
        return gingr_set_error(ctx, GINGR_ERR_HIP, "transform_points: out of device memory (%lld bytes)", (long long)bytes);
    }
    return GINGR_OK;
}

}  // namespace

int kernel_warp_points(gingr_ctx *ctx, KernelWarpWork &work, Cloud Y, const double *coeff, int64_t coeff_stride, double beta,
                       const double *params13, bool no_sum, int64_t P, const double *points_xyz, double *out_xyz) {
    const wp::Plan plan = wp::make_plan(P, no_sum ? 0 : Y.n);
    if (plan.chunks > wp::kMaxChunks) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "transform_points: the template is too large");
    hipStream_t st = ctx->stream;
    GINGR_TRY(grow(ctx, work.stage, plan.cloud_doubles()));
    GINGR_TRY(grow(ctx, work.Z, plan.cloud_doubles()));
    if (!no_sum) {
        GINGR_TRY(grow(ctx, work.part, plan.partial_doubles()));
        if (!work.centres_measured) {  // the centres of a handle never change
            GINGR_TRY(grow(ctx, work.aux, 2));
            launch_cloud_absmax(ctx, Y, nullptr, work.aux.as<double>() + 1);
            work.centres_measured = true;
        }
    }
    double *Zs = work.Z.as<double>();
    for (int64_t s = 0; s < plan.slabs; ++s) {
        const int64_t p0 = plan.slab_begin(s), n = plan.slab_count(s);
        GINGR_TRY(upload_cloud(ctx, work.stage.as<double>(), points_xyz + 3 * p0, n, Zs));
        if (!no_sum) {
            const Cloud Z{Zs, Zs + n, Zs + 2 * n, n};
            launch_cloud_absmax(ctx, Z, nullptr, work.aux.as<double>());
            hipLaunchKernelGGL(kernel_warp_kernel, dim3((unsigned)plan.grid_x(s), (unsigned)plan.grid_y()), dim3(256), 0, st, Z, Y, coeff,
                               coeff_stride, sqrt(2.0) * beta, work.aux.as<double>(), plan.chunk_length, work.part.as<double>());
        }
        hipLaunchKernelGGL(kernel_warp_finish_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, n, work.part.as<double>(),
                           (int)plan.chunks, params13, Zs);
        HIP_TRY(ctx, hipGetLastError());
        GINGR_TRY(download_cloud(ctx, work.stage.as<double>(), Zs, n, out_xyz + 3 * p0));
    }
    return GINGR_OK;
}
