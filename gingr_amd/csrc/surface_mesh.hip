// What the surface correspondence needs of a mesh before any search -- cell and vertex normals, the bounding boxes of the triangle
// tiles -- and the distance statistics behind the evaluators.
#include "surface_device.h"

#include <cmath>

namespace {

// unit normal (B - A) x (C - A)
__device__ __forceinline__ V3 unit_cell_normal(V3 A, V3 B, V3 C) {
    const V3 n = cross3(sub(B, A), sub(C, A));
    const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
    return V3{n.x / len, n.y / len, n.z / len};
}

// cn (SoA [3][T]) = unit normal (b - a) x (c - a) of every triangle
__global__ __launch_bounds__(256) void cell_normals_kernel(Cloud v, const int32_t *__restrict__ tri, int64_t T,
                                                           double *__restrict__ cn) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const Corners c = gather_corners(v, tri, t);
    const V3 n = unit_cell_normal(c.A, c.B, c.C);
    cn[t] = n.x;
    cn[T + t] = n.y;
    cn[2 * T + t] = n.z;
}

// vn (SoA [3][n]) = mean of the adjacent cell normals, adjacency lists in ascending ORIGINAL triangle index
__global__ __launch_bounds__(256) void vertex_normals_kernel(const int32_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj_tri,
                                                             const double *__restrict__ cn, int64_t T, int64_t n,
                                                             double *__restrict__ vn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int32_t b = adj_ptr[i], e = adj_ptr[i + 1];
    for (int32_t k = b; k < e; ++k) {
        const int32_t t = adj_tri[k];
        sx += cn[t];
        sy += cn[T + t];
        sz += cn[2 * T + t];
    }
    const double cnt = e > b ? (double)(e - b) : 1.0;
    vn[i] = sx / cnt;
    vn[n + i] = sy / cnt;
    vn[2 * n + i] = sz / cnt;
}

// boxes[tile] = {lo[3], hi[3]} over the corners of the triangles [tile*256, tile*256+256), followed (at boxes + 6 * ntiles) by the
// boxes of its four 64-triangle quarters [tile*4 + q] (the triangle order is a k-d order down to 64-triangle leaves)
// cn (nullable, SoA [3][T]): the unit cell normals as cell_normals_kernel writes them (same expressions), from the corners this kernel
// reads anyway -- one launch less per surface correspondence.
__global__ __launch_bounds__(256) void tri_tile_bbox_kernel(Cloud v, const int32_t *__restrict__ tri, int64_t T,
                                                            double *__restrict__ boxes, double *__restrict__ tribox,
                                                            double *__restrict__ cn) {
    __shared__ double sh[6][256];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
    double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    if (t < T) {
        V3 P[3];
        for (int c = 0; c < 3; ++c) {
            const int32_t a = tri[3 * t + c];
            const double p[3] = {v.x[a], v.y[a], v.z[a]};
            P[c] = V3{p[0], p[1], p[2]};
            for (int d = 0; d < 3; ++d) {
                lo[d] = fmin(lo[d], p[d]);
                hi[d] = fmax(hi[d], p[d]);
            }
        }
        if (cn) {
            const V3 n = unit_cell_normal(P[0], P[1], P[2]);
            cn[t] = n.x;
            cn[T + t] = n.y;
            cn[2 * T + t] = n.z;
        }
    }
    if (tribox && t < T) {  // per-triangle boxes: the scan kernels stage these (one 48-byte read) instead of rebuilding them from
        double *tb = tribox + 6 * t;  // three index loads and nine gathered coordinates per visited triangle and workgroup
        tb[0] = lo[0], tb[1] = lo[1], tb[2] = lo[2], tb[3] = hi[0], tb[4] = hi[1], tb[5] = hi[2];
    }
    for (int d = 0; d < 3; ++d) {
        sh[d][threadIdx.x] = lo[d];
        sh[3 + d][threadIdx.x] = hi[d];
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int d = 0; d < 3; ++d) {
                sh[d][threadIdx.x] = fmin(sh[d][threadIdx.x], sh[d][threadIdx.x + off]);
                sh[3 + d][threadIdx.x] = fmax(sh[3 + d][threadIdx.x], sh[3 + d][threadIdx.x + off]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) boxes[(int64_t)blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
    // quarter boxes: wave w reduces its own 64 triangles with shuffles
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], off));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], off));
        }
    if ((threadIdx.x & 63) == 0) {
        double *sub = boxes + (int64_t)gridDim.x * 6 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 6;
        for (int d = 0; d < 3; ++d) {
            sub[d] = lo[d];
            sub[3 + d] = hi[d];
        }
    }
}

// ---------------------------------------------------------------------------------------- surface distance statistics
// IndependentPointDistanceEvaluator (G/api/sampling/evaluators/IndependentPointDistanceEvaluator.scala:54-70) and the accuracy
// metrics of RegistrationComparison (G/api/helper/RegistrationComparison.scala:24-73) are reductions over
// d_i = |p_i - closestPointOnSurface(p_i)|: partial[b] = {sum d, max d, count, sum log N(d; 0, sdev)} of block b, points counted
// when orig[i] < orig_limit (the first orig_limit points in the caller's numbering; orig == null: all) and, with `boundary`,
// when the mesh vertex nearest to the surface point is not a boundary vertex (:67-69).  Fixed grid, fixed reduction order.
constexpr int kStatBlocks = 64;

__global__ __launch_bounds__(256) void dist_stats_kernel(int64_t n, const double *__restrict__ d2, const int32_t *__restrict__ orig,
                                                         int64_t orig_limit, const int32_t *__restrict__ nn,
                                                         const int32_t *__restrict__ boundary, double sdev, double lognorm,
                                                         double *__restrict__ partial) {
    __shared__ double sh[4][256];
    double s = 0.0, mx = 0.0, cnt = 0.0, ll = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kStatBlocks * 256) {
        bool take = !orig || orig[i] < orig_limit;
        if (take && boundary) {
            const int32_t j = nn[i];
            take = j >= 0 && !boundary[j];
        }
        if (!take) continue;
        const double d = sqrt(d2[i]);
        s += d;
        mx = fmax(mx, d);
        cnt += 1.0;
        if (sdev > 0.0) {
            const double u = d / sdev;
            ll += -u * u / 2.0 - lognorm;  // breeze Gaussian.logPdf
        }
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = mx;
    sh[2][threadIdx.x] = cnt;
    sh[3][threadIdx.x] = ll;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
            sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + off]);
            sh[2][threadIdx.x] += sh[2][threadIdx.x + off];
            sh[3][threadIdx.x] += sh[3][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void dist_stats_finish_kernel(const double *__restrict__ partial, double *__restrict__ out) {
    if (threadIdx.x >= 4) return;
    double v = 0.0;
    for (int b = 0; b < kStatBlocks; ++b) {
        const double x = partial[b * 4 + threadIdx.x];
        v = threadIdx.x == 1 ? fmax(v, x) : v + x;
    }
    out[threadIdx.x] = v;
}

// Both launches in one for up to kStatBlocks * 256 points (a Metropolis-Hastings step evaluates the likelihood of ~1 600 vertices:
// two dependent launches of 4 us each were all latency).  One wave stands for one block of dist_stats_kernel -- lane l holds the
// elements t = l, l + 64, l + 128, l + 192 of its block -- and adds them in the order of that kernel's LDS tree ((t, t + 128), (t, t + 64),
// then the lanes 32, 16, ... 1 apart), the blocks are added in ascending order as dist_stats_finish_kernel does: the same bits.
__global__ __launch_bounds__(1024) void dist_stats_small_kernel(int64_t n, const double *__restrict__ d2, const int32_t *__restrict__ orig,
                                                                int64_t orig_limit, const int32_t *__restrict__ nn,
                                                                const int32_t *__restrict__ boundary, double sdev, double lognorm,
                                                                double *__restrict__ out) {
    __shared__ double part[kStatBlocks][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblocks = (int)((n + 255) / 256);  // (blocks past the last point hold zeros: adding them changes nothing)
    for (int b = wave; b < nblocks; b += 16) {
        double s[4], mx[4], cnt[4], ll[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = (int64_t)b * 256 + k * 64 + lane;
            s[k] = mx[k] = cnt[k] = ll[k] = 0.0;
            bool take = i < n && (!orig || orig[i] < orig_limit);
            if (take && boundary) {
                const int32_t j = nn[i];
                take = j >= 0 && !boundary[j];
            }
            if (take) {
                const double d = sqrt(d2[i]);
                s[k] = 0.0 + d;
                mx[k] = fmax(0.0, d);
                cnt[k] = 1.0;
                if (sdev > 0.0) {
                    const double u = d / sdev;
                    ll[k] = 0.0 + (-u * u / 2.0 - lognorm);
                }
            }
        }
        // off = 128, 64: between the four elements of a lane; off = 32 .. 1: between lanes
        double a = (s[0] + s[2]) + (s[1] + s[3]), m = fmax(fmax(mx[0], mx[2]), fmax(mx[1], mx[3])), c = (cnt[0] + cnt[2]) + (cnt[1] + cnt[3]),
               l = (ll[0] + ll[2]) + (ll[1] + ll[3]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off);
            m = fmax(m, __shfl_down(m, off));
            c += __shfl_down(c, off);
            l += __shfl_down(l, off);
        }
        if (lane == 0) part[b][0] = a, part[b][1] = m, part[b][2] = c, part[b][3] = l;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = 0.0;
        for (int b = 0; b < nblocks; ++b) {
            const double x = part[b][threadIdx.x];
            v = threadIdx.x == 1 ? fmax(v, x) : v + x;
        }
        out[threadIdx.x] = v;
    }
}

}  // namespace

void launch_cell_normals(gingr_ctx *ctx, Cloud v, const int32_t *tri, int64_t T, double *cn) {
    if (T <= 0) return;
    hipLaunchKernelGGL(cell_normals_kernel, dim3((unsigned)ceil_div(T, 256)), dim3(256), 0, ctx->stream, v, tri, T, cn);
}
void launch_vertex_normals(gingr_ctx *ctx, const int32_t *adj_ptr, const int32_t *adj_tri, const double *cn, int64_t T,
                           int64_t n, double *vn) {
    hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, adj_ptr, adj_tri, cn,
                       T, n, vn);
}
void launch_tri_tile_bbox(gingr_ctx *ctx, Cloud v, const int32_t *tri, int64_t T, double *boxes, double *tribox, double *cell_normals) {
    if (T <= 0) return;
    hipLaunchKernelGGL(tri_tile_bbox_kernel, dim3((unsigned)ceil_div(T, kTriTile)), dim3(256), 0, ctx->stream, v, tri, T, boxes, tribox,
                       cell_normals);
}
int distance_stats_ws_doubles() { return kStatBlocks * 4; }
void launch_distance_stats(gingr_ctx *ctx, int64_t n, const double *d2, const int32_t *orig, int64_t orig_limit, const int32_t *nn,
                           const int32_t *boundary, double sdev, double *partial, double *out4) {
    const double lognorm = sdev > 0.0 ? log(sqrt(2.0 * M_PI)) + log(sdev) : 0.0;
    if (n <= (int64_t)kStatBlocks * 256) {  // every (block, thread) of the two-launch form holds at most one point
        hipLaunchKernelGGL(dist_stats_small_kernel, dim3(1), dim3(1024), 0, ctx->stream, n, d2, orig, orig_limit, nn, boundary, sdev, lognorm, out4);
        return;
    }
    hipLaunchKernelGGL(dist_stats_kernel, dim3(kStatBlocks), dim3(256), 0, ctx->stream, n, d2, orig, orig_limit, nn, boundary, sdev,
                       lognorm, partial);
    hipLaunchKernelGGL(dist_stats_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, partial, out4);
}
