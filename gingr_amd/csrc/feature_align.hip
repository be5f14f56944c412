// Feature-based global alignment: what takes a PARTIAL scan from an arbitrary pose into the basin of the local methods (C ABI in
// include/gingr_hip.h: gingr_cloud_fpfh, gingr_feature_match, gingr_rigid_poses_from_triples; bins, the degenerate-triple test and the
// grid of the match: feature_align_plan.h; the definitions in numpy: tests/feature_alignment_restatement.py).  The descriptor is THIS
// PACKAGE'S DEFINITION of Fast Point Feature Histograms (Rusu 2009), not a toolkit's: the neighbourhood is the k-nearest list of
// cloud_knn.hip cut at a radius, and bins, skips and weights are fixed in the header.
//   spfh kernel     a wave per point, a lane per entry of its neighbour list (k <= 64: the list is exactly one wave).  The lane computes
//                   the pair's three features and bins; the tallies are integer atomics on the wave's 33 words of LDS, so nothing
//                   depends on the order; counts, valid and SPFH = 100 counts / valid leave the wave
//   fpfh kernel     a wave per point, a lane per bin: it walks the neighbour rows IN LIST ORDER, adds SPFH_j / d_j and 1 / d_j, and
//                   rescales its third to sum 100 (the eleven words of a third added in ascending order by every lane of it)
//   match kernel    a query row per lane, in registers; kMatchTile rows of b staged in LDS and read as broadcasts; products and sums
//                   separately rounded in ascending column order (-ffp-contract=off: the bits of the expression on a CPU); a later
//                   row replaces only on a strictly smaller sum.  The rows of b are cut into chunks (the planner); a second kernel
//                   combines the chunks in ascending order by the same rule.  No MFMA: the norm-expansion form changes bits and ties
//   triples kernel  a triple of pairs per lane: the degenerate test, the sums of the three pairs centred on the triple's own target
//                   mean and kabsch_step_from_sums (rigid_step.h), the step search_step_kernel of rigid_search.hip takes
// No float atomic, every float sum in a fixed order: two calls give the same bits.
#include "common.h"
#include "feature_align_plan.h"
#include "rigid_step.h"

#include <cmath>
#include <vector>

namespace fap = feature_align_plan;

namespace {

// counts [N][33], valid [N] (both nullable), spfh [N][33].  idx / d2 [N][k]: the lists of gingr_cloud_knn; normals [N][3] unit or zero.
__global__ __launch_bounds__(64 * fap::kPointsPerBlock) void spfh_kernel(Cloud c, const double *__restrict__ normals, int k,
                                                                         const int32_t *__restrict__ idx, const double *__restrict__ d2,
                                                                         double r2, int32_t *__restrict__ counts, int32_t *__restrict__ valid,
                                                                         double *__restrict__ spfh) {
    __shared__ int32_t hist[fap::kPointsPerBlock][fap::kWords];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * fap::kPointsPerBlock + wv;
    if (lane < fap::kWords) hist[wv][lane] = 0;
    __syncthreads();
    bool counted = false;
    if (i < c.n && lane < k) {
        const int64_t j = idx[i * k + lane];
        const double dd = d2[i * k + lane];
        if (j >= 0 && j < c.n && dd > 0.0 && dd <= r2) {
            const double ux = normals[3 * i], uy = normals[3 * i + 1], uz = normals[3 * i + 2];
            const double nx = normals[3 * j], ny = normals[3 * j + 1], nz = normals[3 * j + 2];
            const bool has = (ux != 0.0 || uy != 0.0 || uz != 0.0) && (nx != 0.0 || ny != 0.0 || nz != 0.0);
            const double dx = c.x[j] - c.x[i], dy = c.y[j] - c.y[i], dz = c.z[j] - c.z[i];
            const double len = sqrt((dx * dx + dy * dy) + dz * dz);
            const double ex = dx / len, ey = dy / len, ez = dz / len;
            const double phi = (ux * ex + uy * ey) + uz * ez;
            double vx = ey * uz - ez * uy, vy = ez * ux - ex * uz, vz = ex * uy - ey * ux;  // dn x u
            const double v2 = (vx * vx + vy * vy) + vz * vz;
            if (has && v2 > fap::kSkip) {
                const double vl = sqrt(v2);
                vx /= vl, vy /= vl, vz /= vl;
                const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;  // u x v
                const double alpha = (vx * nx + vy * ny) + vz * nz;
                const double theta = atan2((wx * nx + wy * ny) + wz * nz, (ux * nx + uy * ny) + uz * nz);
                counted = true;
                atomicAdd(&hist[wv][fap::bin_of_cosine(alpha)], 1);  // (LDS, integers)
                atomicAdd(&hist[wv][fap::kBins + fap::bin_of_cosine(phi)], 1);
                atomicAdd(&hist[wv][2 * fap::kBins + fap::bin_of_angle(theta)], 1);
            }
        }
    }
    const int nv = (int)__popcll(__ballot(counted));
    __syncthreads();
    if (i < c.n && lane < fap::kWords) {
        const int32_t h = hist[wv][lane];
        if (counts) counts[i * fap::kWords + lane] = h;
        spfh[i * fap::kWords + lane] = nv > 0 ? 100.0 * (double)h / (double)nv : 0.0;
    }
    if (i < c.n && lane == 0 && valid) valid[i] = nv;
}

__global__ __launch_bounds__(64 * fap::kPointsPerBlock) void fpfh_kernel(int64_t N, int k, const int32_t *__restrict__ idx,
                                                                         const double *__restrict__ d2, double r2,
                                                                         const double *__restrict__ spfh, double *__restrict__ out) {
    __shared__ double row[fap::kPointsPerBlock][fap::kWords];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * fap::kPointsPerBlock + wv;
    const bool mine = i < N && lane < fap::kWords;
    double f = 0.0;
    if (mine) {
        double num = 0.0, den = 0.0;
        for (int s = 0; s < k; ++s) {  // (the list is the same for every lane of the wave)
            const int64_t j = idx[i * k + s];
            const double dd = d2[i * k + s];
            if (!(j >= 0 && j < N && dd > 0.0 && dd <= r2)) continue;
            const double dj = sqrt(dd);
            num += spfh[j * fap::kWords + lane] / dj;
            den += 1.0 / dj;
        }
        f = spfh[i * fap::kWords + lane] + (den > 0.0 ? num / den : 0.0);
        row[wv][lane] = f;
    }
    __syncthreads();
    if (mine) {
        const int third = lane / fap::kBins;
        double s = 0.0;
        for (int b = 0; b < fap::kBins; ++b) s += row[wv][third * fap::kBins + b];
        out[i * fap::kWords + lane] = s != 0.0 ? f * (100.0 / s) : f;
    }
}

// Chunk blockIdx.y of the rows of b against the query rows of the workgroup: pidx / pd2 [chunks][M].  W: the padded row width.
template <int W>
__global__ __launch_bounds__(fap::kMatchThreads) void match_kernel(int64_t M, const double *__restrict__ a, int64_t N, const double *__restrict__ b,
                                                                   int D, int64_t chunk_rows, int32_t *__restrict__ pidx,
                                                                   double *__restrict__ pd2) {
    __shared__ double tile[fap::kMatchTile * W];
    const int t = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * fap::kMatchThreads + t;
    double row[W];
#pragma unroll
    for (int cc = 0; cc < W; ++cc) row[cc] = (q < M && cc < D) ? a[q * D + cc] : 0.0;
    double best = __builtin_huge_val();
    int32_t bi = -1;
    const int64_t first = (int64_t)blockIdx.y * chunk_rows, end = first + chunk_rows < N ? first + chunk_rows : N;
    for (int64_t base = first; base < end; base += fap::kMatchTile) {
        const int rows = (int)(end - base < fap::kMatchTile ? end - base : fap::kMatchTile);
        __syncthreads();  // (the previous tile has been read)
        for (int e = t; e < rows * W; e += fap::kMatchThreads) {
            const int r = e / W, cc = e - r * W;
            tile[e] = cc < D ? b[(base + r) * D + cc] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int cc = 0; cc < W; ++cc) {
                const double d = row[cc] - tile[r * W + cc];
                acc = acc + d * d;  // (a padded column adds +0)
            }
            if (acc < best || bi < 0) best = acc, bi = (int32_t)(base + r);
        }
    }
    if (q < M) pidx[(int64_t)blockIdx.y * M + q] = bi, pd2[(int64_t)blockIdx.y * M + q] = best;
}

__global__ __launch_bounds__(256) void match_combine_kernel(int64_t M, int chunks, const int32_t *__restrict__ pidx, const double *__restrict__ pd2,
                                                            int32_t *__restrict__ idx, double *__restrict__ d2) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= M) return;
    double best = pd2[q];
    int32_t bi = pidx[q];
    for (int ch = 1; ch < chunks; ++ch) {  // ascending rows: only a strictly smaller sum replaces
        const double v = pd2[(int64_t)ch * M + q];
        if (v < best) best = v, bi = pidx[(int64_t)ch * M + q];
    }
    idx[q] = bi, d2[q] = best;
}

// moving [M][3], target [N][3] interleaved; tm / tt [H][3]; poses [H][12], degenerate [H]
__global__ __launch_bounds__(fap::kTripleThreads) void poses_from_triples_kernel(int64_t M, const double *__restrict__ moving, int64_t N,
                                                                                 const double *__restrict__ target, int64_t H,
                                                                                 const int32_t *__restrict__ tm, const int32_t *__restrict__ tt,
                                                                                 double *__restrict__ poses, int32_t *__restrict__ degenerate) {
    const int64_t h = (int64_t)blockIdx.x * fap::kTripleThreads + threadIdx.x;
    if (h >= H) return;
    const int32_t im[3] = {tm[3 * h], tm[3 * h + 1], tm[3 * h + 2]}, it[3] = {tt[3 * h], tt[3 * h + 1], tt[3 * h + 2]};
    bool bad = fap::triple_repeats(im) || fap::triple_repeats(it);
    for (int a = 0; a < 3; ++a) bad = bad || im[a] < 0 || im[a] >= M || it[a] < 0 || it[a] >= N;  // (refused on the host: no read out of bounds)
    double p[3][3], y[3][3];
    if (!bad) {
        for (int a = 0; a < 3; ++a)
            for (int d = 0; d < 3; ++d) p[a][d] = moving[3 * (int64_t)im[a] + d], y[a][d] = target[3 * (int64_t)it[a] + d];
        bad = fap::triangle_degenerate(p[0], p[1], p[2]) || fap::triangle_degenerate(y[0], y[1], y[2]);
    }
    double T[12];
    if (!bad) {
        double c[3], S[16];
        for (int d = 0; d < 3; ++d) c[d] = ((y[0][d] + y[1][d]) + y[2][d]) / 3.0;
        for (int q = 0; q < 16; ++q) S[q] = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double p0 = p[a][0] - c[0], p1 = p[a][1] - c[1], p2 = p[a][2] - c[2];
            const double y0 = y[a][0] - c[0], y1 = y[a][1] - c[1], y2 = y[a][2] - c[2];
            S[0] += 1.0;
            S[1] += p0; S[2] += p1; S[3] += p2;
            S[4] += y0; S[5] += y1; S[6] += y2;
            S[7] += y0 * p0; S[8] += y0 * p1; S[9] += y0 * p2;
            S[10] += y1 * p0; S[11] += y1 * p1; S[12] += y1 * p2;
            S[13] += y2 * p0; S[14] += y2 * p1; S[15] += y2 * p2;
        }
        kabsch_step_from_sums(S, c, T, T + 9);
        for (int q = 0; q < 12; ++q) bad = bad || !(fabs(T[q]) <= kDblMax);
    }
    for (int q = 0; q < 12; ++q) poses[12 * h + q] = bad ? __builtin_nan("") : T[q];
    degenerate[h] = bad ? 1 : 0;
}

bool all_finite(const double *v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

template <int W>
void launch_match(gingr_ctx *ctx, int64_t M, const double *a, int64_t N, const double *b, int D, int64_t chunks, int64_t chunk_rows, int32_t *pidx,
                  double *pd2) {
    hipLaunchKernelGGL((match_kernel<W>), dim3((unsigned)ceil_div(M, fap::kMatchThreads), (unsigned)chunks), dim3(fap::kMatchThreads), 0,
                       ctx->stream, M, a, N, b, D, chunk_rows, pidx, pd2);
}

}  // namespace

extern "C" {

int gingr_cloud_fpfh(gingr_ctx *ctx, int64_t N, const double *xyz, const double *normals, int32_t k, double radius, int32_t *counts_out,
                     int32_t *valid_out, double *fpfh_out, gingr_cloud_knn_info *info) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!xyz || !normals || !fpfh_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_fpfh: null argument");
    if (N > ((int64_t)1 << 27)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_fpfh: need N <= 2^27");
    const int bad = fap::check_fpfh(N, (int)k, radius);
    if (bad == 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_fpfh: need %d <= k <= %d and k <= N", fap::kMinK, fap::kMaxK);
    if (bad == 2) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "cloud_fpfh: radius = %g, need a finite radius > 0", radius);
    if (!all_finite(xyz, 3 * N)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "cloud_fpfh: non-finite coordinate");
    if (!all_finite(normals, 3 * N)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "cloud_fpfh: non-finite normal");
    // the normals by the rule of gingr_fitter_set_target_normals: unit to 2^-48 as they are, else scaled and normalised; zero = none
    const size_t n = (size_t)N, nk = n * (size_t)k, nw = n * (size_t)fap::kWords;
    std::vector<double> unit(3 * n);
    for (int64_t j = 0; j < N; ++j) {
        const double x = normals[3 * j], y = normals[3 * j + 1], z = normals[3 * j + 2];
        const double big = std::fmax(std::fabs(x), std::fmax(std::fabs(y), std::fabs(z)));
        double ux = 0.0, uy = 0.0, uz = 0.0;
        if (big > 0.0) {
            const double n2 = (x * x + y * y) + z * z;
            if (std::fabs(n2 - 1.0) <= 0x1p-48) {
                ux = x, uy = y, uz = z;
            } else {
                const double sx = x / big, sy = y / big, sz = z / big, len = std::sqrt((sx * sx + sy * sy) + sz * sz);
                ux = sx / len, uy = sy / len, uz = sz / len;
            }
        }
        unit[3 * (size_t)j] = ux, unit[3 * (size_t)j + 1] = uy, unit[3 * (size_t)j + 2] = uz;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf stage, soa, dn, didx, dd2, dcounts, dvalid, dspfh, dout;
    HIP_TRY(ctx, stage.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, soa.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, dn.alloc(3 * n * sizeof(double)));
    HIP_TRY(ctx, didx.alloc(nk * sizeof(int32_t)));
    HIP_TRY(ctx, dd2.alloc(nk * sizeof(double)));
    if (counts_out) HIP_TRY(ctx, dcounts.alloc(nw * sizeof(int32_t)));
    if (valid_out) HIP_TRY(ctx, dvalid.alloc(n * sizeof(int32_t)));
    HIP_TRY(ctx, dspfh.alloc(nw * sizeof(double)));
    HIP_TRY(ctx, dout.alloc(nw * sizeof(double)));
    GINGR_TRY(upload_cloud(ctx, stage.as<double>(), xyz, N, soa.as<double>()));
    HIP_TRY(ctx, hipMemcpyAsync(dn.p, unit.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const Cloud c{soa.as<double>(), soa.as<double>() + N, soa.as<double>() + 2 * N, N};
    GINGR_TRY(cloud_knn_device(ctx, c, k, didx.as<int32_t>(), dd2.as<double>(), info, "cloud_fpfh"));  // (the list stays on the device)
    const double r2 = radius * radius;
    const dim3 grid((unsigned)ceil_div(N, fap::kPointsPerBlock)), block(64 * fap::kPointsPerBlock);
    {
        TimerScope ts(ctx, 27);
        hipLaunchKernelGGL(spfh_kernel, grid, block, 0, ctx->stream, c, dn.as<double>(), (int)k, didx.as<int32_t>(), dd2.as<double>(), r2,
                           counts_out ? dcounts.as<int32_t>() : nullptr, valid_out ? dvalid.as<int32_t>() : nullptr, dspfh.as<double>());
        hipLaunchKernelGGL(fpfh_kernel, grid, block, 0, ctx->stream, N, (int)k, didx.as<int32_t>(), dd2.as<double>(), r2, dspfh.as<double>(),
                           dout.as<double>());
    }
    GINGR_TRY(check_launch(ctx));
    if (counts_out) HIP_TRY(ctx, hipMemcpyAsync(counts_out, dcounts.p, nw * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (valid_out) HIP_TRY(ctx, hipMemcpyAsync(valid_out, dvalid.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fpfh_out, dout.p, nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_feature_match(gingr_ctx *ctx, int64_t M, const double *a, int64_t N, const double *b, int32_t D, int32_t *idx_out, double *d2_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!a || !b || !idx_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "feature_match: null argument");
    if (!fap::check_match(M, N, (int)D) || M > INT32_MAX || N > INT32_MAX)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "feature_match: M = %lld, N = %lld, D = %d: sizes >= 1 (below 2^31), 1 <= D <= %d",
                               (long long)M, (long long)N, (int)D, fap::kMaxD);
    if (!all_finite(a, M * D) || !all_finite(b, N * D)) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "feature_match: non-finite entry");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t chunks = fap::match_chunks(M, N), chunk_rows = fap::match_chunk_rows(M, N);
    const size_t m = (size_t)M;
    DevBuf da, db, pidx, pd2, didx, dd2;
    HIP_TRY(ctx, da.alloc(m * D * sizeof(double)));
    HIP_TRY(ctx, db.alloc((size_t)N * D * sizeof(double)));
    HIP_TRY(ctx, pidx.alloc(m * chunks * sizeof(int32_t)));
    HIP_TRY(ctx, pd2.alloc(m * chunks * sizeof(double)));
    HIP_TRY(ctx, didx.alloc(m * sizeof(int32_t)));
    HIP_TRY(ctx, dd2.alloc(m * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(da.p, a, m * D * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(db.p, b, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    {
        TimerScope ts(ctx, 28);
        const int W = fap::match_width((int)D);
        if (W == 16)
            launch_match<16>(ctx, M, da.as<double>(), N, db.as<double>(), (int)D, chunks, chunk_rows, pidx.as<int32_t>(), pd2.as<double>());
        else if (W == 40)
            launch_match<40>(ctx, M, da.as<double>(), N, db.as<double>(), (int)D, chunks, chunk_rows, pidx.as<int32_t>(), pd2.as<double>());
        else
            launch_match<64>(ctx, M, da.as<double>(), N, db.as<double>(), (int)D, chunks, chunk_rows, pidx.as<int32_t>(), pd2.as<double>());
        hipLaunchKernelGGL(match_combine_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, (int)chunks, pidx.as<int32_t>(),
                           pd2.as<double>(), didx.as<int32_t>(), dd2.as<double>());
    }
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(idx_out, didx.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (d2_out) HIP_TRY(ctx, hipMemcpyAsync(d2_out, dd2.p, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_rigid_poses_from_triples(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t H,
                                   const int32_t *tri_moving, const int32_t *tri_target, double *poses12_out, int32_t *degenerate_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!moving_xyz || !target_xyz || !tri_moving || !tri_target || !poses12_out)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_poses_from_triples: null argument");
    if (M < 1 || M > INT32_MAX || N < 1 || N > INT32_MAX || H < 1 || H > INT32_MAX)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_poses_from_triples: M = %lld, N = %lld, H = %lld: sizes >= 1 (below 2^31)",
                               (long long)M, (long long)N, (long long)H);
    for (int64_t q = 0; q < 3 * H; ++q)
        if (tri_moving[q] < 0 || tri_moving[q] >= M || tri_target[q] < 0 || tri_target[q] >= N)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "rigid_poses_from_triples: triple %lld has an index out of range", (long long)(q / 3));
    if (!all_finite(moving_xyz, 3 * M) || !all_finite(target_xyz, 3 * N))
        return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "rigid_poses_from_triples: non-finite coordinate");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf dm, dt, dtm, dtt, dposes, ddeg;
    HIP_TRY(ctx, dm.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, dt.alloc((size_t)3 * N * sizeof(double)));
    HIP_TRY(ctx, dtm.alloc((size_t)3 * H * sizeof(int32_t)));
    HIP_TRY(ctx, dtt.alloc((size_t)3 * H * sizeof(int32_t)));
    HIP_TRY(ctx, dposes.alloc((size_t)12 * H * sizeof(double)));
    HIP_TRY(ctx, ddeg.alloc((size_t)H * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(dm.p, moving_xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dt.p, target_xyz, (size_t)3 * N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dtm.p, tri_moving, (size_t)3 * H * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dtt.p, tri_target, (size_t)3 * H * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    {
        TimerScope ts(ctx, 29);
        hipLaunchKernelGGL(poses_from_triples_kernel, dim3((unsigned)ceil_div(H, fap::kTripleThreads)), dim3(fap::kTripleThreads), 0, ctx->stream,
                           M, dm.as<double>(), N, dt.as<double>(), H, dtm.as<int32_t>(), dtt.as<int32_t>(), dposes.as<double>(),
                           ddeg.as<int32_t>());
    }
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(poses12_out, dposes.p, (size_t)12 * H * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (degenerate_out) HIP_TRY(ctx, hipMemcpyAsync(degenerate_out, ddeg.p, (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

}  // extern "C"
