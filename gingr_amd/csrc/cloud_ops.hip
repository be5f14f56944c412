// Small per-cloud kernels of the update path for gfx950 (MI355X): centroid, extent, tile boxes, Gaussian kernel blocks, the sum of
// squared pair distances, layout conversions, the all-pairs distance extrema (gingr_pointset_distance_extrema) -- and the library's one
// copy of the host-side k-d leaf order (kd_order.h).
//
// Reference loops replaced (G/ = src/main/scala/gingr/):
//   gauss_block  : GaussianKernel(sigma)*scaling          G/api/gpmm/GPMMHelper.scala:99-102
//   sumsq_pairs  : computeInitialSigma2                   G/api/registration/config/CPD.scala:81-90
#include "common.h"
#include "block_sum.h"
#include "box_device.h"
#include "cpd_plan.h"
#include "fastexp.h"
#include "kd_order.h"

namespace {

constexpr int kBlock = 256;

// boxes[tile] = {lo[3], hi[3]} of the points [tile*256, tile*256+256) of a cloud, followed (at boxes + 6 * ntiles) by the boxes
// of its four 64-point quarters, [tile*4 + q]: the k-d leaf order makes those compact too (finer exact-zero culling).
// With slot != nullptr also slot = max over the cloud of |coordinate - ctr| (atomic max on the bit pattern of a non-negative
// double: order independent, deterministic); the slot must have been zeroed by an EARLIER launch on the stream.
constexpr int kBoxTilesPerBlock = 8;
// One workgroup handles kBoxTilesPerBlock consecutive tiles (wave q the quarter q of each), so the launch ends with one atomic per
// 2048 points: agent-scope atomics on one word are served at the memory side, one after the other (~0.13 us each: with one tile per
// workgroup the 196 tiles of 50k points took 26 us, all of it the atomics).  The 64-lane minima / maxima are not butterflies of
// cross-lane shuffles (6 dependent LDS round trips per quantity: 14 us for the 48 quantities of a wave) but column scans: the wave
// parks its values in LDS, [quantity][lane], and lane j < 48 scans the 64 entries of ITS quantity, starting at entry j so that the
// lanes of one read sit in different banks.  fmin ignores NaN like the butterfly did (a NaN point never widens a box).
__global__ __launch_bounds__(256) void tile_bbox_kernel(Cloud c, double *__restrict__ boxes, const double *__restrict__ ctr,
                                                        double *__restrict__ slot, int64_t ntiles) {
    constexpr int Q = kBoxTilesPerBlock * 3;          // quantities per wave: (tile, coordinate)
    __shared__ double park[4][Q][64];
    __shared__ double sh[kBoxTilesPerBlock][4][6];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t tile0 = (int64_t)blockIdx.x * kBoxTilesPerBlock;
    double v[Q];
#pragma unroll
    for (int t = 0; t < kBoxTilesPerBlock; ++t) {  // all loads in flight; an absent point is NaN: fmin / fmax skip it
        const int64_t i = (tile0 + t) * kTile + threadIdx.x;
        const bool ok = i < c.n;
        v[3 * t] = ok ? c.x[i] : __builtin_nan("");
        v[3 * t + 1] = ok ? c.y[i] : __builtin_nan("");
        v[3 * t + 2] = ok ? c.z[i] : __builtin_nan("");
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) park[wave][k][lane] = v[k];
    __builtin_amdgcn_wave_barrier();  // wave-local data: LDS serves one wave's accesses in order
    if (lane < 2 * Q) {
        const int k = lane >> 1;
        const double sgn = (lane & 1) ? -1.0 : 1.0;  // odd lanes: maximum as -min(-x)
        double m = __builtin_huge_val();
#pragma unroll 8
        for (int e = 0; e < 64; ++e) m = fmin(m, sgn * park[wave][k][(e + lane) & 63]);
        const int t = k / 3, d = k % 3;
        const double r = sgn * m;  // (+huge, -huge) for a quarter without points, as before
        if (tile0 + t < ntiles) {
            boxes[ntiles * 6 + ((tile0 + t) * 4 + wave) * 6 + (lane & 1) * 3 + d] = r;
            sh[t][wave][(lane & 1) * 3 + d] = r;
        }
    }
    __syncthreads();
    double m = 0.0;
    if (threadIdx.x < kBoxTilesPerBlock * 3) {  // thread (t, d): both bounds of coordinate d of tile t
        const int t = threadIdx.x / 3, d = threadIdx.x % 3;
        if (tile0 + t < ntiles) {
            const double lo = fmin(fmin(sh[t][0][d], sh[t][1][d]), fmin(sh[t][2][d], sh[t][3][d]));
            const double hi = fmax(fmax(sh[t][0][3 + d], sh[t][1][3 + d]), fmax(sh[t][2][3 + d], sh[t][3][3 + d]));
            boxes[(tile0 + t) * 6 + d] = lo;
            boxes[(tile0 + t) * 6 + 3 + d] = hi;
            const double cc = ctr ? ctr[d] : 0.0;
            m = fmax(fabs(lo - cc), fabs(hi - cc));
        }
    }
    if (slot && wave == 0) {  // kBoxTilesPerBlock * 3 <= 64: the candidates all sit in wave 0
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        if (lane == 0) {
            // non-negative doubles order like their bit patterns; only a value above what is already there needs the atomic
            const unsigned long long mb = __builtin_bit_cast(unsigned long long, m);
            if (mb > __hip_atomic_load(reinterpret_cast<unsigned long long *>(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(reinterpret_cast<unsigned long long *>(slot), mb);
        }
    }
}

// centroid of a cloud into out[0..2] (single workgroup, fixed order)
__global__ __launch_bounds__(1024) void cloud_centroid_kernel(Cloud c, double *__restrict__ out) {
    __shared__ double sh[3][1024];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t i = threadIdx.x; i < c.n; i += 1024) {
        sx += c.x[i];
        sy += c.y[i];
        sz += c.z[i];
    }
    sh[0][threadIdx.x] = sx;
    sh[1][threadIdx.x] = sy;
    sh[2][threadIdx.x] = sz;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int d = 0; d < 3; ++d) sh[d][threadIdx.x] += sh[d][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        const double v = sh[threadIdx.x][0] / (double)c.n;
        out[threadIdx.x] = (v == v && fabs(v) < 1e300) ? v : 0.0;  // a non-finite centroid would poison every pair
    }
}

// slot = max over the cloud of |x - cx|, |y - cy|, |z - cz| (ctr may be nullptr = origin).  Atomic max on the bit
// pattern of a non-negative double: order independent, hence deterministic.  The slot must be zeroed before the launch.
__global__ __launch_bounds__(256) void cloud_absmax_kernel(Cloud c, const double *__restrict__ ctr, double *__restrict__ slot) {
    __shared__ double sh[256];
    const double cx = ctr ? ctr[0] : 0.0, cy = ctr ? ctr[1] : 0.0, cz = ctr ? ctr[2] : 0.0;
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < c.n; i += (int64_t)gridDim.x * 256)
        m = fmax(m, fmax(fabs(c.x[i] - cx), fmax(fabs(c.y[i] - cy), fabs(c.z[i] - cz))));
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = sh[0];
        if (!(v == v)) v = __builtin_huge_val();  // NaN coordinates: force the clamped exact path
        atomicMax(reinterpret_cast<unsigned long long *>(slot), __builtin_bit_cast(unsigned long long, v));
    }
}

// ---------------------------------------------------------------- Gaussian kernel block
__global__ __launch_bounds__(kBlock) void gauss_block_kernel(Cloud A, Cloud B, double sigma, double scaling,
                                                             double *__restrict__ out) {
    __shared__ double T[GINGR_EXP_TABLE];
    fastexp_table_init(T);
    __syncthreads();
    const double c = fastexp_scale_for_variance(sigma * sigma);
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= B.n) return;
    const double dx = A.x[i] - B.x[j], dy = A.y[i] - B.y[j], dz = A.z[i] - B.z[j];
    const double d2 = fastexp_clamp_d2(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)), fastexp_d2_limit(c));
    out[i * B.n + j] = scaling * fastexp2_scaled(d2, c, T);
}

// ---------------------------------------------------------------- sum of squared pair distances (initial sigma2)
__global__ __launch_bounds__(kBlock) void sumsq_pairs_kernel(Cloud A, Cloud B, double *__restrict__ partial) {
    __shared__ P4 tile[kTile];
    __shared__ double sh[kBlock];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
    const bool ok = i < A.n;
    const double ax = ok ? A.x[i] : 0.0, ay = ok ? A.y[i] : 0.0, az = ok ? A.z[i] : 0.0;
    double acc = 0.0;
    for (int64_t jb = 0; jb < B.n; jb += kTile) {
        __syncthreads();
        const int64_t j = jb + tid;
        if (j < B.n) tile[tid] = P4{B.x[j], B.y[j], B.z[j], 0.0};
        __syncthreads();
        const int cnt = (int)min((int64_t)kTile, B.n - jb);
        for (int jj = 0; jj < cnt; ++jj) {
            const P4 p = tile[jj];
            const double dx = p.x - ax, dy = p.y - ay, dz = p.z - az;
            acc += dx * dx + dy * dy + dz * dz;
        }
    }
    if (!ok) acc = 0.0;
    __syncthreads();
    const double tot = block_sum<kBlock>(acc, sh);
    if (tid == 0) partial[blockIdx.x] = tot;
}

// The same sum from moments: sum_ij |a_i - b_j|^2 = n_B sum |a_i - c|^2 + n_A sum |b_j - c|^2 - 2 (sum (a_i - c)) . (sum (b_j - c)) for any c
// (here a_0, so that the three terms are of the size of the result: no cancellation beyond a digit) -- O(n_A + n_B) instead of the
// pair loop's 1.3 ms at 50k x 50k; it differs from the reference's double loop (CPD.scala:81-90) by rounding only, as the pair
// loop's tree of partial sums did.  partial: [2][kMomentBlocks][4].
constexpr int kMomentBlocks = 64;
__global__ __launch_bounds__(kBlock) void cloud_moments_kernel(Cloud A, Cloud B, double *__restrict__ partial) {
    __shared__ double sh[kBlock];
    const Cloud C = blockIdx.y == 0 ? A : B;
    const double cx = A.x[0], cy = A.y[0], cz = A.z[0];
    double sx = 0.0, sy = 0.0, sz = 0.0, s2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < C.n; i += (int64_t)kMomentBlocks * kBlock) {
        const double dx = C.x[i] - cx, dy = C.y[i] - cy, dz = C.z[i] - cz;
        sx += dx, sy += dy, sz += dz;
        s2 += dx * dx + dy * dy + dz * dz;
    }
    double *out = partial + ((int64_t)blockIdx.y * kMomentBlocks + blockIdx.x) * 4;
    const double v[4] = {sx, sy, sz, s2};
    for (int k = 0; k < 4; ++k) {
        __syncthreads();
        const double tot = block_sum<kBlock>(v[k], sh);
        if (threadIdx.x == 0) out[k] = tot;
    }
}
__global__ void sumsq_from_moments_kernel(const double *__restrict__ partial, int64_t nA, int64_t nB, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int c = 0; c < 2; ++c)
        for (int b = 0; b < kMomentBlocks; ++b)
            for (int k = 0; k < 4; ++k) m[c][k] += partial[((int64_t)c * kMomentBlocks + b) * 4 + k];
    out[0] = ((double)nB * m[0][3] + (double)nA * m[1][3]) - 2.0 * (m[0][0] * m[1][0] + m[0][1] * m[1][1] + m[0][2] * m[1][2]);
}

__global__ __launch_bounds__(1024) void sum_vector_kernel(const double *__restrict__ v, int64_t n, double scale,
                                                          double *__restrict__ out) {
    __shared__ double sh[1024];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) acc += v[i];
    const double tot = block_sum<1024>(acc, sh);
    if (threadIdx.x == 0) out[0] = tot * scale;
}

__global__ void aos_to_soa_kernel(const double *__restrict__ aos, int64_t n, const int32_t *__restrict__ perm,
                                  double *__restrict__ soa) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t o = perm ? perm[i] : i;
    soa[i] = aos[3 * o];
    soa[n + i] = aos[3 * o + 1];
    soa[2 * n + i] = aos[3 * o + 2];
}

__global__ void soa_to_aos_kernel(const double *__restrict__ soa, int64_t n, const int32_t *__restrict__ perm,
                                  double *__restrict__ aos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t o = perm ? perm[i] : i;
    aos[3 * o] = soa[i];
    aos[3 * o + 1] = soa[n + i];
    aos[3 * o + 2] = soa[2 * n + i];
}

__global__ void scatter_kernel(const double *__restrict__ in, int64_t n, const int32_t *__restrict__ perm,
                               double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[perm ? perm[i] : i] = in[i];
}

// all-pairs extrema of |p_i - p_j|^2 (unfused), i != j: per-workgroup partials.  The distance of a pair is the same number in both
// orders (the coordinate differences are exact negations of each other, their squares equal), so only the tile pairs on and above the
// diagonal are visited: workgroup (bi, c) takes the 256 points of tile bi against the column tiles bi + c ch ... bi + (c + 1) ch - 1;
// workgroups past the last tile write the neutral pair (0, +inf).  A maximum and a minimum do not depend on the order of the scan: the
// result is the one-row-per-thread scan's of rounds 1-5 bit for bit (that one ran on ceil(n / 256) workgroups -- 196 for 50k points,
// fewer than the device has compute units -- and visited every pair twice: 2.5 ms at 50k).  The `j != i` test only exists in the
// diagonal tile.
constexpr int kExtTile = 256;
__global__ __launch_bounds__(kExtTile) void dist_extrema_kernel(Cloud pts, int ch, double *__restrict__ pmax, double *__restrict__ pmin) {
    __shared__ double tx[kExtTile], ty[kExtTile], tz[kExtTile];
    __shared__ double sh[kExtTile];
    const int t = threadIdx.x;
    const int64_t nt = (pts.n + kExtTile - 1) / kExtTile;
    const int64_t bi = blockIdx.x;
    const int64_t jt0 = bi + (int64_t)blockIdx.y * ch, jt1 = min(nt, jt0 + ch);  // workgroup-uniform
    const int64_t i = bi * kExtTile + t;
    const bool ok = i < pts.n;
    const double x = ok ? pts.x[i] : 0.0, y = ok ? pts.y[i] : 0.0, z = ok ? pts.z[i] : 0.0;
    double mx = 0.0, mn = __builtin_huge_val();
    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t jb = jt * kExtTile;
        __syncthreads();
        if (jb + t < pts.n) {
            tx[t] = pts.x[jb + t];
            ty[t] = pts.y[jb + t];
            tz[t] = pts.z[jb + t];
        }
        __syncthreads();
        const int cnt = (int)min((int64_t)kExtTile, pts.n - jb);
        if (!ok) continue;
        if (jt == bi) {  // the diagonal tile: every pair of it from both sides, the point itself left out of the minimum
#pragma unroll 4
            for (int jj = 0; jj < cnt; ++jj) {
                const double dx = x - tx[jj], dy = y - ty[jj], dz = z - tz[jj];
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                mx = fmax(mx, d2);
                if (jj != t) mn = fmin(mn, d2);
            }
        } else {
#pragma unroll 4
            for (int jj = 0; jj < cnt; ++jj) {
                const double dx = x - tx[jj], dy = y - ty[jj], dz = z - tz[jj];
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                mx = fmax(mx, d2);
                mn = fmin(mn, d2);
            }
        }
    }
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    __syncthreads();
    sh[t] = mx;
    __syncthreads();
    for (int off = kExtTile / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] = fmax(sh[t], sh[t + off]);
        __syncthreads();
    }
    if (t == 0) pmax[slot] = sh[0];
    __syncthreads();
    sh[t] = mn;
    __syncthreads();
    for (int off = kExtTile / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] = fmin(sh[t], sh[t + off]);
        __syncthreads();
    }
    if (t == 0) pmin[slot] = sh[0];
}

}  // namespace

void launch_cloud_centroid(gingr_ctx *ctx, Cloud c, double *out3) {
    hipLaunchKernelGGL(cloud_centroid_kernel, dim3(1), dim3(1024), 0, ctx->stream, c, out3);
}

void launch_cloud_absmax(gingr_ctx *ctx, Cloud c, const double *ctr, double *slot) {
    (void)hipMemsetAsync(slot, 0, sizeof(double), ctx->stream);
    const int nb = (int)(ceil_div(c.n, 256) < 64 ? ceil_div(c.n, 256) : 64);
    hipLaunchKernelGGL(cloud_absmax_kernel, dim3(nb > 0 ? nb : 1), dim3(256), 0, ctx->stream, c, ctr, slot);
}

void launch_tile_bbox(gingr_ctx *ctx, Cloud c, double *boxes, const double *ctr, double *absmax_slot) {
    if (c.n <= 0) return;
    const int64_t ntiles = ceil_div(c.n, kTile);
    hipLaunchKernelGGL(tile_bbox_kernel, dim3((unsigned)ceil_div(ntiles, kBoxTilesPerBlock)), dim3(256), 0, ctx->stream, c, boxes, ctr,
                       absmax_slot, ntiles);
}

void launch_gauss_block(gingr_ctx *ctx, Cloud A, Cloud B, double sigma, double scaling, double *out) {
    // gridDim.y is limited to 65535 rows per launch
    const int64_t max_rows = 65535;
    for (int64_t r0 = 0; r0 < A.n; r0 += max_rows) {
        const int64_t nr = A.n - r0 < max_rows ? A.n - r0 : max_rows;
        Cloud sub{A.x + r0, A.y + r0, A.z + r0, nr};
        dim3 grid((unsigned)ceil_div(B.n, kBlock), (unsigned)nr);
        hipLaunchKernelGGL(gauss_block_kernel, grid, dim3(kBlock), 0, ctx->stream, sub, B, sigma, scaling, out + r0 * B.n);
    }
}

int64_t sumsq_pairs_ws_doubles(int64_t nA) { return std::max<int64_t>(ceil_div(nA, kBlock), 2 * kMomentBlocks * 4); }

void launch_sumsq_pairs(gingr_ctx *ctx, Cloud A, Cloud B, double *ws, double *out_scalar) {
    if (A.n * B.n >= (int64_t)1 << 20) {  // (small problems keep the pair loop: nothing to gain, and its bits are what the tests of old pin)
        hipLaunchKernelGGL(cloud_moments_kernel, dim3(kMomentBlocks, 2), dim3(kBlock), 0, ctx->stream, A, B, ws);
        hipLaunchKernelGGL(sumsq_from_moments_kernel, dim3(1), dim3(64), 0, ctx->stream, ws, A.n, B.n, out_scalar);
        return;
    }
    const int64_t nb = ceil_div(A.n, kBlock);
    hipLaunchKernelGGL(sumsq_pairs_kernel, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, A, B, ws);
    hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(1024), 0, ctx->stream, ws, nb, 1.0, out_scalar);
}

void launch_aos_to_soa(gingr_ctx *ctx, const double *aos, int64_t n, double *soa, const int32_t *perm) {
    if (n <= 0) return;
    hipLaunchKernelGGL(aos_to_soa_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, aos, n, perm, soa);
}

void launch_soa_to_aos(gingr_ctx *ctx, const double *soa, int64_t n, double *aos, const int32_t *perm) {
    if (n <= 0) return;
    hipLaunchKernelGGL(soa_to_aos_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, soa, n, perm, aos);
}

int upload_cloud(gingr_ctx *ctx, double *stage, const double *xyz, int64_t n, double *soa, const int32_t *perm) {
    HIP_TRY(ctx, hipMemcpyAsync(stage, xyz, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, stage, n, soa, perm);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffer is reused
    return GINGR_OK;
}

int download_cloud(gingr_ctx *ctx, double *stage, const double *soa, int64_t n, double *xyz, const int32_t *perm) {
    launch_soa_to_aos(ctx, soa, n, stage, perm);
    HIP_TRY(ctx, hipMemcpyAsync(xyz, stage, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffer is reused
    return GINGR_OK;
}

int first_variance(gingr_ctx *ctx, Cloud A, Cloud B, double factor, double *ws, double *slot, double *out) {
    launch_sumsq_pairs(ctx, A, B, ws, slot);
    double tot = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&tot, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = factor * tot / (3.0 * (double)B.n * (double)A.n);
    return GINGR_OK;
}

int finish_iterate(gingr_ctx *ctx, int32_t *flags, int words, int decides, const char *name) {
    HIP_TRY(ctx, hipGetLastError());
    int32_t err[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(err, flags, words * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!err[decides]) return GINGR_OK;
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, words * sizeof(int32_t), ctx->stream));
    return gingr_set_error(ctx, err[decides], "%s: %s", name, err[decides] == GINGR_ERR_NOT_SPD ? "system not positive definite" : "non-finite result");
}

void launch_scatter(gingr_ctx *ctx, const double *in, int64_t n, const int32_t *perm, double *out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, in, n, perm, out);
}
void kd_leaf_order(const double *xyz, int64_t n, std::vector<int32_t> &perm) { kd_leaf_order(xyz, n, perm, KdParallel{}); }

extern "C" {

int gingr_pointset_distance_extrema(gingr_ctx *ctx, const double *xyz, int64_t n, double *max_distance,
                                    double *min_distance) {
    if (!ctx || !xyz || n < 1 || !max_distance || !min_distance)
        return ctx ? gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "distance_extrema: bad argument") : GINGR_ERR_BAD_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // tiles of 256 points; a workgroup takes `ch` column tiles (eight, more for large clouds so that there are at most 64 chunks per tile
    // row): about nt^2 / (2 ch) working workgroups -- 2 500 at 50k points
    const int64_t nt = ceil_div(n, (int64_t)kExtTile);
    const int ch = (int)std::max<int64_t>(8, ceil_div(nt, (int64_t)64));
    const int gy = (int)ceil_div(nt, (int64_t)ch);
    if (nt > 0x7fffffff / 64) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "distance_extrema: %lld points are too many", (long long)n);
    const int64_t nb = nt * gy;
    DevBuf aos, soa, pm;
    HIP_TRY(ctx, aos.alloc((size_t)3 * n * sizeof(double)));
    HIP_TRY(ctx, soa.alloc((size_t)3 * n * sizeof(double)));
    HIP_TRY(ctx, pm.alloc((size_t)2 * nb * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(aos.p, xyz, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos.as<double>(), n, soa.as<double>());
    const double *s = soa.as<double>();
    hipLaunchKernelGGL(dist_extrema_kernel, dim3((unsigned)nt, (unsigned)gy), dim3(kExtTile), 0, ctx->stream, Cloud{s, s + n, s + 2 * n, n}, ch,
                       pm.as<double>(), pm.as<double>() + nb);
    GINGR_TRY(check_launch(ctx));
    std::vector<double> h((size_t)2 * nb);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), pm.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double mx = 0.0, mn = HUGE_VAL;
    for (int64_t b = 0; b < nb; ++b) {
        mx = std::max(mx, h[(size_t)b]);
        mn = std::min(mn, h[(size_t)nb + b]);
    }
    *max_distance = std::sqrt(mx);   // max of sqrt = sqrt of max (sqrt is monotone and correctly rounded)
    *min_distance = std::sqrt(mn);   // +inf for a single point
    return GINGR_OK;
}

}  // extern "C"
