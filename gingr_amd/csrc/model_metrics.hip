// Model metrics on the device (C ABI in include/gingr_hip.h: gingr_model_instances, gingr_model_generalization,
// gingr_model_specificity): many instances of a resident model, many shapes projected onto its k leading components, many samples
// against many training shapes.  Distances are vertex to corresponding vertex.
//   D      [3 M + 48][np]  the centred shapes X - ref - mean as a block of columns in the basis layout, rows in the model's order
//   b      = Q0^T D        the cross Gram pass of augment_model.hip with D as the second "basis"
//   B      = S_tot / eps + I = L L^T, eps = GINGR_COEFF_NOISE: the matrix model_finalize_impl factors for Binv.  The factor of a leading
//            block is the leading block of the factor, and so is that of W = L^-T (dense_spd_inverse without its product): one
//            factorisation serves every rank, alpha_k = W_k W_k^T (b_k / eps) with W_k the leading k x k block (rank_solve_kernel)
//   T      [rp][n_ranks np] column q np + i = alpha_k(q) of shape i, zero from row k on
//   A      project_measure_kernel: Q0 T on float64 MFMA (the tiles of basis_rotate.h), never stored: the epilogue subtracts the column
//            of D, takes the Euclidean norm over the three coordinate tiles and keeps a sum and a maximum per column
//   P      [3 M + 48][sp]  ref + mean + Q0 T stored (instances_kernel): gingr_model_instances, and the samples of the specificity
//   B      pair_distance_kernel: sum_v |s_v - t_v| for every (sample column, training column) pair, VALU, 4 x 4 pairs per lane
// Every sum is taken in a fixed order (per-lane ascending, a butterfly of two steps, waves and slabs added by one thread in ascending
// order; no float atomics): two calls with the same input give the same bits.
#include "basis_rotate.h"
#include "dense_spd.h"
#include "model_metrics.h"
#include "model_metrics_plan.h"

#include <algorithm>
#include <cmath>

namespace mp = model_metrics_plan;

namespace {

static_assert(mp::kGroupVerts == kRotWaves * kRotVerts, "a step of the measure pass is one 16-vertex tile per wave");
static_assert(mp::kChunkCols == 16 * kRotChunkTiles, "a chunk is the column tiles a wave holds");
static_assert(mp::kRowSlack <= kBasisRowSlack, "a block of columns is read like a basis");

constexpr int kPackVerts = 64;  // vertices of a tile (device rows)
constexpr int kPackCols = 64;   // shapes of a tile

// D[3 s + d][col0 + j] = X_j[3 perm[s] + d] - ref[d][s] - mean[d][s] (center) or X_j[3 perm[s] + d] for the staged shapes j < cnt
// (X: interleaved, caller's point order; perm == nullptr: the rows keep that order).  Block (b, d): the device rows [64 b, 64 b + 64), 64 shapes at a time through LDS
// (center_pack_kernel, pca_model.hip): the reads gather a shape's vertices in the model's order, the writes run along a row of D.
__global__ __launch_bounds__(256) void shapes_pack_kernel(const double *__restrict__ X, int cnt, int col0, int np, int64_t M,
                                                          const int32_t *__restrict__ perm, const double *__restrict__ ref,
                                                          const double *__restrict__ mean, int center, double *__restrict__ D) {
    __shared__ double tile[kPackCols][kPackVerts + 1];
    const int d = blockIdx.y, tid = threadIdx.x, v = tid & 63;
    const int64_t s0 = (int64_t)blockIdx.x * kPackVerts, s = s0 + v;
    const bool live = s < M;
    const int64_t src = live ? (int64_t)3 * (perm ? perm[s] : s) + d : 0;
    const double rf = (live && center) ? ref[(int64_t)d * M + s] : 0.0, mn = (live && center) ? mean[(int64_t)d * M + s] : 0.0;
    for (int j0 = 0; j0 < cnt; j0 += kPackCols) {
        __syncthreads();
        for (int jj = tid >> 6; jj < kPackCols; jj += 4) {
            const int j = j0 + jj;
            tile[jj][v] = (live && j < cnt) ? X[(int64_t)j * 3 * M + src] - rf - mn : 0.0;
        }
        __syncthreads();
        const int jj = tid & 63, j = j0 + jj;
        if (j < cnt)
            for (int vv = tid >> 6; vv < kPackVerts; vv += 4)
                if (s0 + vv < M) D[(3 * (s0 + vv) + d) * np + col0 + j] = tile[jj][vv];
    }
}

// X_j[3 perm[s] + d] = P[3 s + d][j] for the columns j < cnt: the transpose of shapes_pack_kernel
__global__ __launch_bounds__(256) void shapes_unpack_kernel(const double *__restrict__ P, int cnt, int sp, int64_t M,
                                                            const int32_t *__restrict__ perm, double *__restrict__ X) {
    __shared__ double tile[kPackVerts][kPackCols + 1];
    const int d = blockIdx.y, tid = threadIdx.x, v = tid & 63;
    const int64_t s0 = (int64_t)blockIdx.x * kPackVerts, s = s0 + v;
    const bool live = s < M;
    const int64_t dst = live ? (int64_t)3 * perm[s] + d : 0;
    for (int j0 = 0; j0 < cnt; j0 += kPackCols) {
        __syncthreads();
        {
            const int jj = tid & 63, j = j0 + jj;
            for (int vv = tid >> 6; vv < kPackVerts; vv += 4) tile[vv][jj] = (s0 + vv < M && j < cnt) ? P[(3 * (s0 + vv) + d) * sp + j] : 0.0;
        }
        __syncthreads();
        for (int jj = tid >> 6; jj < kPackCols; jj += 4) {
            const int j = j0 + jj;
            if (live && j < cnt) X[(int64_t)j * 3 * M + dst] = tile[v][jj];
        }
    }
}

// Block i, shape i: u = b_i / eps, y = W^T u (y[j] needs the rows i' <= j alone: the same y for every rank), then row by row
// alpha_k[row] = sum_{row <= j < k} W[row][j] y[j] as one running sum over j that is written out whenever j reaches the next rank.
// T[row][q np + i] and coef[q][i][row] (nullable) get alpha_k(q)[row], zero from row k(q) on.  C: [rp][np] (b_i in column i).
__global__ __launch_bounds__(256) void rank_solve_kernel(int r, int rp, const double *__restrict__ W, int64_t ldw, const double *__restrict__ C, int np,
                                                         int n, RankList ranks, double *__restrict__ T, int64_t ldt, double *__restrict__ coef) {
    __shared__ double u[512], y[512];
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < r; k += 256) u[k] = C[(int64_t)k * np + i] / GINGR_COEFF_NOISE;
    __syncthreads();
    for (int j = tid; j < r; j += 256) {
        double acc = 0.0;
        for (int ii = 0; ii <= j; ++ii) acc = __builtin_fma(W[ii * ldw + j], u[ii], acc);
        y[j] = acc;
    }
    __syncthreads();
    for (int row = tid; row < rp; row += 256) {
        double acc = 0.0;
        int j = row;
        for (int q = 0; q < ranks.n; ++q) {
            const int k = ranks.k[q];
            for (; j < k; ++j) acc = __builtin_fma(W[row * ldw + j], y[j], acc);
            const double val = row < k ? acc : 0.0;
            T[row * ldt + (int64_t)q * np + i] = val;
            if (coef && row < r) coef[((int64_t)q * n + i) * r + row] = val;
        }
    }
}

// T [rp][ldt]: T[row][c] = alphas[c][row] for row < k, c < cnt (alphas: [cnt][r] on the device), zero elsewhere
__global__ __launch_bounds__(256) void sample_factor_kernel(const double *__restrict__ alphas, int cnt, int r, int k, int rp, int ldt,
                                                            double *__restrict__ T) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)rp * ldt) return;
    const int row = (int)(e / ldt), c = (int)(e - (int64_t)row * ldt);
    T[e] = (row < k && c < cnt) ? alphas[(int64_t)c * r + row] : 0.0;
}

// ---- ref + mean + Q0 T stored: basis_rotate_kernel (posterior_model.hip) within one model -- no row gather, the identity rotation --
// plus the mean shape in the epilogue.  T: [rp][ldt], P: [3 M + 48][ldt]; rows 3 M and beyond are not written.
template <int NT>
__device__ __forceinline__ void instances_chunk(const double *__restrict__ qrow, int rp, int ldt, const double *__restrict__ T, int n0, int kq, int cl,
                                                const double *__restrict__ ref, const double *__restrict__ mean, int64_t M, int64_t v0,
                                                double *__restrict__ out) {
    const Rot3 identity{{1, 0, 0, 0, 1, 0, 0, 0, 1}};  // (1 x + (0 y + 0 z) is x: the store of basis_rotate.h as it is)
    v4f64 acc[3][NT];
    rotate_clear<NT>(acc);
    rotate_accumulate<NT>(acc, qrow, rp, ldt, T, n0, kq, cl);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int64_t v = v0 + kq + 4 * g;
        if (v >= M) continue;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double base = ref[(int64_t)d * M + v] + mean[(int64_t)d * M + v];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[d][j][g] = base + acc[d][j][g];
        }
    }
    rotate_store<NT>(acc, ldt, n0, kq, cl, identity, out, M - v0);
}

__global__ __launch_bounds__(64 * kRotWaves) void instances_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ T, int ldt,
                                                                   const double *__restrict__ ref, const double *__restrict__ mean, int nchunks,
                                                                   double *__restrict__ P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t vb = blockIdx.x / nchunks;
    const int chunk = (int)(blockIdx.x - vb * nchunks);
    const int64_t v0 = (vb * kRotWaves + wave) * kRotVerts;
    if (v0 >= M) return;
    const int64_t v = v0 + cl;
    const double *qrow = Q0 + 3 * (v < M ? v : M) * (int64_t)rp;  // (past the last vertex: the zero rows behind the basis)
    double *out = P + 3 * v0 * (int64_t)ldt;
    const int nt = ldt / 16, t0 = chunk * kRotChunkTiles;
    switch (min(nt - t0, kRotChunkTiles)) {
        case 1: instances_chunk<1>(qrow, rp, ldt, T, 16 * t0, kq, cl, ref, mean, M, v0, out); break;
        case 2: instances_chunk<2>(qrow, rp, ldt, T, 16 * t0, kq, cl, ref, mean, M, v0, out); break;
        case 3: instances_chunk<3>(qrow, rp, ldt, T, 16 * t0, kq, cl, ref, mean, M, v0, out); break;
        case 4: instances_chunk<4>(qrow, rp, ldt, T, 16 * t0, kq, cl, ref, mean, M, v0, out); break;
        default: break;
    }
}

// ---- kernel A: reconstruct and measure.  Workgroup (slab, chunk): the eight waves walk the slab in steps of 128 vertices, 16 each; a
// wave forms the chunk's columns of Q0 T for its 16 vertices in the accumulator tiles and never stores them: for the accumulator's
// vertex (register g: kq + 4 g) and column (cl + 16 j) the three coordinates sit in the same lane and register of the three row tiles,
// so the lane subtracts the three entries of D -- column (n0 + 16 j) % np + cl: a tile lies inside one rank's np columns -- takes the
// norm and adds it to the column's sum and maximum.  A lane's sums run over its vertices in ascending order; the four lane groups of a
// column are added by a butterfly (both steps commute: every lane ends with the same bits), the eight waves in ascending order by one
// thread per column.  Vertices past M add nothing and read nothing of D; Q0 is read at its zero rows for them.
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

template <int NT>
__device__ __forceinline__ void measure_tiles(const double *__restrict__ qrow, int rp, int ldt, const double *__restrict__ T, int n0, int kq, int cl,
                                              const double *__restrict__ drow, int np, int64_t vleft, double (&sum)[kRotChunkTiles],
                                              double (&mx)[kRotChunkTiles]) {
    v4f64 acc[3][NT];
    rotate_clear<NT>(acc);
    rotate_accumulate<NT>(acc, qrow, rp, ldt, T, n0, kq, cl);
    int dcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dcol[j] = (n0 + 16 * j) % np + cl;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int i = kq + 4 * g;  // vertex of the wave this register belongs to
        if (i >= vleft) continue;
        const double *dv = drow + (int64_t)3 * i * np;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const double x = acc[0][j][g] - dv[dcol[j]], y = acc[1][j][g] - dv[np + dcol[j]], z = acc[2][j][g] - dv[2 * np + dcol[j]];
            const double dist = sqrt(__builtin_fma(x, x, __builtin_fma(y, y, z * z)));
            sum[j] += dist;
            mx[j] = nan_max(dist, mx[j]);
        }
    }
}

__global__ __launch_bounds__(64 * kRotWaves) void project_measure_kernel(const double *__restrict__ Q0, int64_t M, int rp, const double *__restrict__ T,
                                                                         int ldt, const double *__restrict__ D, int np, int64_t verts_per_slab,
                                                                         int nchunks, double *__restrict__ partial) {
    __shared__ double red[kRotWaves][2][16 * kRotChunkTiles];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
    const int64_t slab = blockIdx.x / nchunks;
    const int chunk = (int)(blockIdx.x - slab * nchunks);
    const int64_t s0 = slab * verts_per_slab, s1 = min(M, s0 + verts_per_slab);
    const int nt = ldt / 16, t0 = chunk * kRotChunkTiles, n0 = 16 * t0;
    const int ntl = min(nt - t0, kRotChunkTiles);
    double sum[kRotChunkTiles], mx[kRotChunkTiles];
#pragma unroll
    for (int j = 0; j < kRotChunkTiles; ++j) sum[j] = 0.0, mx[j] = 0.0;
    for (int64_t v0 = s0 + (int64_t)wave * kRotVerts; v0 < s1; v0 += kRotWaves * kRotVerts) {
        const int64_t v = v0 + cl;
        const double *qrow = Q0 + 3 * (v < M ? v : M) * (int64_t)rp;
        const double *drow = D + 3 * v0 * (int64_t)np;
        switch (ntl) {
            case 1: measure_tiles<1>(qrow, rp, ldt, T, n0, kq, cl, drow, np, M - v0, sum, mx); break;
            case 2: measure_tiles<2>(qrow, rp, ldt, T, n0, kq, cl, drow, np, M - v0, sum, mx); break;
            case 3: measure_tiles<3>(qrow, rp, ldt, T, n0, kq, cl, drow, np, M - v0, sum, mx); break;
            case 4: measure_tiles<4>(qrow, rp, ldt, T, n0, kq, cl, drow, np, M - v0, sum, mx); break;
            default: break;
        }
    }
#pragma unroll
    for (int j = 0; j < kRotChunkTiles; ++j) {
        sum[j] += __shfl_xor(sum[j], 16);
        sum[j] += __shfl_xor(sum[j], 32);
        mx[j] = nan_max(mx[j], __shfl_xor(mx[j], 16));
        mx[j] = nan_max(mx[j], __shfl_xor(mx[j], 32));
        if (kq == 0) {
            red[wave][0][16 * j + cl] = sum[j];
            red[wave][1][16 * j + cl] = mx[j];
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < 16 * kRotChunkTiles && n0 + c < ldt) {
        double s = red[0][0][c], m = red[0][1][c];
        for (int w = 1; w < kRotWaves; ++w) {
            s += red[w][0][c];
            m = nan_max(m, red[w][1][c]);
        }
        double *out = partial + slab * 2 * (int64_t)ldt;
        out[n0 + c] = s;
        out[ldt + n0 + c] = m;
    }
}

// avg[q][i] = (sum of the slab partials of column q np + i in ascending order) / M, max[q][i] = the largest of their maxima
__global__ __launch_bounds__(256) void measure_finish_kernel(const double *__restrict__ partial, int nslabs, int ldt, int np, int n, int n_ranks, int64_t M,
                                                             double *__restrict__ avg, double *__restrict__ mx) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ranks * n) return;
    const int q = e / n, i = e - q * n, col = q * np + i;
    double s = 0.0, m = 0.0;
    for (int b = 0; b < nslabs; ++b) {
        s += partial[(int64_t)b * 2 * ldt + col];
        m = nan_max(m, partial[(int64_t)b * 2 * ldt + ldt + col]);
    }
    avg[e] = s / (double)M;
    mx[e] = m;
}

// ---- kernel B: samples against training shapes.  P [3 M + 48][sp] the samples, Tr [3 M + 48][tp] the training shapes, both as points
// (not centred), rows in the model's order.  Workgroup (slab, tile): 64 sample columns x 64 training columns over the slab's vertices;
// lane (ts, tt) keeps the 4 x 4 pairs of the sample columns 4 ts .. 4 ts + 3 and the training columns 4 tt .. 4 tt + 3 in registers:
// six 32-byte loads per vertex for 16 pairs, the 16 lanes of a row of lanes read 512 contiguous bytes of a sample row.  Per pair and
// vertex: three subtractions, a multiply, two FMAs, a square root, an add.  A lane adds its vertices in ascending order; the slabs are
// added by pair_finish_kernel.  partial: [slab][training column][sample column].  Padded columns hold finite numbers (the mean shape
// and zeros) and are never read back.
__global__ __launch_bounds__(256) void pair_distance_kernel(const double *__restrict__ P, int sp, const double *__restrict__ Tr, int tp, int64_t M,
                                                            int64_t verts_per_slab, int tiles_t, double *__restrict__ partial) {
    const int ps = blockIdx.y / tiles_t, pt = blockIdx.y - ps * tiles_t;
    const int ts = threadIdx.x & 15, tt = threadIdx.x >> 4;
    const int cs = ps * 64 + 4 * ts, ct = pt * 64 + 4 * tt;
    if (cs >= sp || ct >= tp) return;  // (sp, tp are multiples of 16: all four columns or none; no barrier below)
    const int64_t v0 = (int64_t)blockIdx.x * verts_per_slab, v1 = min(M, v0 + verts_per_slab);
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    const double *ps_row = P + cs, *pt_row = Tr + ct;
#pragma unroll 2
    for (int64_t v = v0; v < v1; ++v) {
        d4 s[3], t[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            s[d] = *reinterpret_cast<const d4 *>(ps_row + (3 * v + d) * sp);
            t[d] = *reinterpret_cast<const d4 *>(pt_row + (3 * v + d) * tp);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double x = s[0][b] - t[0][a], y = s[1][b] - t[1][a], z = s[2][b] - t[2][a];
                acc[a][b] += sqrt(__builtin_fma(x, x, __builtin_fma(y, y, z * z)));
            }
    }
    double *out = partial + (int64_t)blockIdx.x * sp * tp;
#pragma unroll
    for (int a = 0; a < 4; ++a) *reinterpret_cast<d4 *>(out + (int64_t)(ct + a) * sp + cs) = d4{acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
}

// Thread c, sample column c < cnt: for the training shapes j in ascending order the slab partials in ascending order, / M; the smallest
// mean and its index, the lowest index on an exact tie (a later shape replaces the best only when strictly smaller).
__global__ __launch_bounds__(256) void pair_finish_kernel(const double *__restrict__ partial, int nslabs, int sp, int tp, int cnt, int n_train, int64_t M,
                                                          double *__restrict__ min_avg, int32_t *__restrict__ argmin) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cnt) return;
    double best = 0.0;
    int32_t bi = 0;
    for (int j = 0; j < n_train; ++j) {
        double s = 0.0;
        for (int b = 0; b < nslabs; ++b) s += partial[((int64_t)b * tp + j) * sp + c];
        const double m = s / (double)M;
        if (j == 0 || m < best) {
            best = m;
            bi = j;
        }
    }
    min_avg[c] = best;
    argmin[c] = bi;
}

struct MetricsElem {  // S_tot / eps + I: BinvElem of gp.hip
    const double *__restrict__ S;
    int rp;
    __device__ double operator()(int64_t row, int64_t c) const { return S[row * rp + c] / GINGR_COEFF_NOISE + (row == c ? 1.0 : 0.0); }
};

}  // namespace

// ---- host side
int metrics_check_model(gingr_ctx *ctx, const gingr_model *m, const char *who) {
    const char *fault = complete_model_fault(ctx, m);  // (a model of another context is a bad argument, the other two a state)
    return !fault ? GINGR_OK : gingr_set_error(ctx, m->ctx != ctx ? GINGR_ERR_BAD_ARGUMENT : GINGR_ERR_STATE, "%s: the model %s", who, fault);
}

int metrics_check_ranks(gingr_ctx *ctx, const gingr_model *m, int32_t n_ranks, const int32_t *ranks, const char *who, RankList *out) {
    if (n_ranks < 1 || n_ranks > mp::kMaxRanks || !ranks)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d ranks, need 1 <= n_ranks <= %d", who, (int)n_ranks, (int)mp::kMaxRanks);
    out->n = n_ranks;
    for (int32_t q = 0; q < n_ranks; ++q) {
        if (ranks[q] < 1 || ranks[q] > m->r)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: ranks[%d] = %d outside 1..%d (the model's rank)", who, (int)q, (int)ranks[q],
                                   (int)m->r);
        if (q > 0 && ranks[q] <= ranks[q - 1])
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: ranks must be strictly increasing (ranks[%d] = %d after %d)", who, (int)q,
                                   (int)ranks[q], (int)ranks[q - 1]);
        out->k[q] = ranks[q];
    }
    for (int32_t q = n_ranks; q < mp::kMaxRanks; ++q) out->k[q] = 0;
    return GINGR_OK;
}

// P [3 M + 48][ldt] = ref + mean + Q0 T on ctx->stream (the slack rows are the caller's)
void launch_instances(gingr_ctx *ctx, const gingr_model *m, const double *T, int ldt, double *P) {
    const int nchunks = (int)ceil_div(ldt / 16, kRotChunkTiles);
    const int64_t blocks = ceil_div(m->M, (int64_t)kRotWaves * kRotVerts) * nchunks;
    TimerScope ts(ctx, 20);
    hipLaunchKernelGGL(instances_kernel, dim3((unsigned)blocks), dim3(64 * kRotWaves), 0, ctx->stream, m->Q0, m->M, (int)m->rp, T, ldt, m->ref, m->mean,
                       nchunks, P);
}

// T [rp][ldt] on the device: column c < cnt = the k leading entries of alphas[c] (device, [cnt][r]), zero elsewhere.  On ctx->stream.
void launch_sample_factor(gingr_ctx *ctx, const double *alphas, int cnt, int r, int k, int rp, int ldt, double *T) {
    hipLaunchKernelGGL(sample_factor_kernel, dim3((unsigned)ceil_div((int64_t)rp * ldt, 256)), dim3(256), 0, ctx->stream, alphas, cnt, r, k, rp, ldt, T);
}

// n shapes (host, interleaved, caller's point order) as the columns [0, n) of D [3 M + 48][np], centred or as points; the padding
// columns and the slack rows are zero.  The shapes pass through the staging buffer of for_each_shape_stage (model.hip).
int pack_shape_columns(gingr_ctx *ctx, int64_t M, const int32_t *perm, const double *ref, const double *mean, int n, const double *shapes, bool center,
                       DevBuf &D, int np) {
    DevBuf stage;
    HIP_TRY(ctx, D.alloc((size_t)mp::block_rows(M) * np * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(D.p, 0, (size_t)mp::block_rows(M) * np * sizeof(double), ctx->stream));
    GINGR_TRY(for_each_shape_stage(ctx, M, n, shapes, stage, [&](int cnt, int i0) -> int {
        hipLaunchKernelGGL(shapes_pack_kernel, dim3((unsigned)ceil_div(M, kPackVerts), 3), dim3(256), 0, ctx->stream, stage.as<double>(), cnt, i0, np, M,
                           perm, ref, mean, center ? 1 : 0, D.as<double>());
        return GINGR_OK;
    }));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffer leaves scope
    return GINGR_OK;
}

// kernel A and its finish on ctx->stream: avg [n_ranks][n] and max [n_ranks][n] into res (device, 2 n_ranks n doubles) of
// |Q0 T - D| per vertex, column q np + i of T against column i of D.  Q0: [3 M + 48][rp], T: [rp][ldt], ldt = n_ranks np.
int launch_project_measure(gingr_ctx *ctx, const double *Q0, int64_t M, int rp, const double *T, int ldt, const double *D, int np, int n, int n_ranks,
                           DevBuf &partial, double *res) {
    const mp::MeasurePlan plan = mp::make_measure_plan(M, ldt);
    HIP_TRY(ctx, partial.alloc((size_t)plan.partial_doubles() * sizeof(double)));
    {
        TimerScope ts(ctx, 18);
        hipLaunchKernelGGL(project_measure_kernel, dim3((unsigned)plan.workgroups()), dim3(64 * kRotWaves), 0, ctx->stream, Q0, M, rp, T, ldt, D, np,
                           plan.verts_per_slab, (int)plan.chunks, partial.as<double>());
    }
    hipLaunchKernelGGL(measure_finish_kernel, dim3((unsigned)ceil_div((int64_t)n_ranks * n, 256)), dim3(256), 0, ctx->stream, partial.as<double>(),
                       (int)plan.slabs, ldt, np, n, n_ranks, M, res, res + (size_t)n_ranks * n);
    return check_launch(ctx);
}

// The front half of a generalization call, on ctx->stream: D [3 M + 48][np] the centred shapes, T [rp][n_ranks np] one column of
// coefficients per (rank, shape) -- column q np + i = alpha_k(q) of shape i -- and coef [n_ranks][n][r] (when wanted).  f.flag (device,
// inside f.work) is non-zero when S_tot / eps + I was not positive definite.  Nothing synchronises: f owns every buffer in flight.
int project_rank_factors(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, const RankList &rl, bool want_coef,
                         RankFactors &f) {
    DevBuf &D = f.D, &ws = f.ws, &C = f.C, &work = f.work, &T = f.T, &coef = f.coef;
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp, n_ranks = rl.n;
    const int np = (int)mp::padded_cols(n), ldt = n_ranks * np;
    // ---- D and b = Q0^T D
    GINGR_TRY(pack_shape_columns(ctx, M, model->perm, model->ref, model->mean, n, shapes_xyz, true, D, np));
    gingr_model dm;  // D as the second "basis" of the cross Gram pass, in this model's row order
    dm.M = M, dm.Q0 = D.as<double>(), dm.rp = np, dm.iperm = model->iperm;
    {
        int npa, npb, nslabs;
        int64_t vps;
        cross_gram_plan(M, rp, np, &npa, &npb, &nslabs, &vps);
        HIP_TRY(ctx, ws.alloc((size_t)nslabs * rp * np * sizeof(double)));
    }
    HIP_TRY(ctx, C.alloc((size_t)rp * np * sizeof(double)));
    launch_cross_gram(ctx, model, &dm, ws.as<double>(), C.as<double>());
    GINGR_TRY(check_launch(ctx));

    // ---- W = L^-T of S_tot / eps + I, once for every rank
    const DenseSpdWork sw(rp, DenseSpdWork::kIdentity);
    HIP_TRY(ctx, work.alloc((size_t)sw.doubles() * sizeof(double)));
    double *Aw = work.as<double>() + sw.aw(), *Linv = work.as<double>() + sw.linv();
    int32_t *flag = reinterpret_cast<int32_t *>(work.as<double>() + sw.flag());
    launch_spd_system(ctx->stream, (int)r, sw, MetricsElem{model->mom + MomentLayout{rp}.stot(), (int)rp}, SpdIdentityBorder{}, Aw, flag);
    dense_spd_inverse(ctx, Aw, sw.Mp, Linv, nullptr, flag);
    GINGR_TRY(check_launch(ctx));

    // ---- T: one column per (rank, shape)
    HIP_TRY(ctx, T.alloc((size_t)rp * ldt * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(T.p, 0, (size_t)rp * ldt * sizeof(double), ctx->stream));
    if (want_coef) HIP_TRY(ctx, coef.alloc((size_t)n_ranks * n * r * sizeof(double)));
    hipLaunchKernelGGL(rank_solve_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, (int)r, (int)rp, work.as<double>() + sw.lt(), sw.Mp, C.as<double>(),
                       np, (int)n, rl, T.as<double>(), (int64_t)ldt, want_coef ? coef.as<double>() : nullptr);
    GINGR_TRY(check_launch(ctx));

    f.flag = flag;
    return GINGR_OK;
}

extern "C" {

int gingr_model_instances(gingr_ctx *ctx, const gingr_model *model, int64_t n, const double *alphas, double *out_xyz) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_instances";
    if (!model || !alphas || !out_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    GINGR_TRY(metrics_check_model(ctx, model, who));
    if (n < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n = %lld < 1", who, (long long)n);
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    GINGR_TRY(check_finite(ctx, alphas, r, n, who, "coefficient vector"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const mp::ColumnBlocks blocks = mp::column_blocks(n);
    const int ldmax = (int)blocks.padded(0);
    // the instances leave through a staging buffer of at most 64 MB (at least one shape)
    const int per_stage = (int)std::max<int64_t>(1, std::min<int64_t>(ldmax, ((int64_t)8 << 20) / (3 * M)));
    DevBuf A, T, P, stage;
    HIP_TRY(ctx, A.alloc((size_t)ldmax * r * sizeof(double)));
    HIP_TRY(ctx, T.alloc((size_t)rp * ldmax * sizeof(double)));
    HIP_TRY(ctx, P.alloc((size_t)mp::block_rows(M) * ldmax * sizeof(double)));
    HIP_TRY(ctx, stage.alloc((size_t)per_stage * 3 * M * sizeof(double)));
    for (int64_t b = 0; b < blocks.count; ++b) {
        const int cnt = (int)blocks.length(b), ldt = (int)blocks.padded(b);
        const int64_t c0 = blocks.begin(b);
        HIP_TRY(ctx, hipMemcpyAsync(A.p, alphas + c0 * r, (size_t)cnt * r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        launch_sample_factor(ctx, A.as<double>(), cnt, (int)r, (int)r, (int)rp, ldt, T.as<double>());
        launch_instances(ctx, model, T.as<double>(), ldt, P.as<double>());
        GINGR_TRY(check_launch(ctx));
        for (int i0 = 0; i0 < cnt; i0 += per_stage) {
            const int part = std::min(per_stage, cnt - i0);
            hipLaunchKernelGGL(shapes_unpack_kernel, dim3((unsigned)ceil_div(M, kPackVerts), 3), dim3(256), 0, ctx->stream, P.as<double>() + i0, part, ldt,
                               M, model->perm, stage.as<double>());
            GINGR_TRY(check_launch(ctx));
            HIP_TRY(ctx, hipMemcpyAsync(out_xyz + (size_t)(c0 + i0) * 3 * M, stage.p, (size_t)part * 3 * M * sizeof(double), hipMemcpyDeviceToHost,
                                        ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GINGR_OK;
}

int gingr_model_generalization(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, int32_t n_ranks, const int32_t *ranks,
                               double *coeffs, double *avg, double *max_out) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_generalization";
    if (!model || !shapes_xyz || !avg || !max_out) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    GINGR_TRY(metrics_check_model(ctx, model, who));
    if (n < 1 || n > mp::kMaxShapes)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d shapes, need 1 <= n <= %d per call", who, (int)n, (int)mp::kMaxShapes);
    RankList rl;
    GINGR_TRY(metrics_check_ranks(ctx, model, n_ranks, ranks, who, &rl));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    GINGR_TRY(check_finite(ctx, shapes_xyz, 3 * M, n, who, "shape"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int np = (int)mp::padded_cols(n), ldt = n_ranks * np;

    RankFactors f;
    DevBuf partial, res;
    GINGR_TRY(project_rank_factors(ctx, model, n, shapes_xyz, rl, coeffs != nullptr, f));
    DevBuf &D = f.D, &T = f.T, &coef = f.coef;
    const int32_t *flag = f.flag;

    // ---- kernel A and its finish
    HIP_TRY(ctx, res.alloc((size_t)2 * n_ranks * n * sizeof(double)));
    GINGR_TRY(launch_project_measure(ctx, model->Q0, M, (int)rp, T.as<double>(), ldt, D.as<double>(), np, (int)n, (int)n_ranks, partial, res.as<double>()));
    int32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(avg, res.p, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(max_out, res.as<double>() + (size_t)n_ranks * n, (size_t)n_ranks * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (coeffs) HIP_TRY(ctx, hipMemcpyAsync(coeffs, coef.p, (size_t)n_ranks * n * r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "%s: Q^T Q / 1e-5 + I is not positive definite", who);
    return GINGR_OK;
}

int gingr_model_specificity(gingr_ctx *ctx, const gingr_model *model, int32_t n_train, const double *train_xyz, int64_t n_samples, const double *alphas,
                            int32_t n_ranks, const int32_t *ranks, double *min_avg, int32_t *argmin) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    const char *who = "model_specificity";
    if (!model || !train_xyz || !alphas || !min_avg || !argmin) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    GINGR_TRY(metrics_check_model(ctx, model, who));
    if (n_train < 1 || n_train > mp::kMaxShapes)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d training shapes, need 1 <= n_train <= %d", who, (int)n_train, (int)mp::kMaxShapes);
    if (n_samples < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n_samples = %lld < 1", who, (long long)n_samples);
    RankList rl;
    GINGR_TRY(metrics_check_ranks(ctx, model, n_ranks, ranks, who, &rl));
    const int64_t M = model->M;
    const int32_t r = model->r, rp = model->rp;
    GINGR_TRY(check_finite(ctx, train_xyz, 3 * M, n_train, who, "training shape"));
    GINGR_TRY(check_finite(ctx, alphas, r, n_samples, who, "coefficient vector"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int tp = (int)mp::padded_cols(n_train);
    const mp::ColumnBlocks blocks = mp::column_blocks(n_samples);
    const int ldmax = (int)blocks.padded(0);

    DevBuf Tr, A, T, P, partial, best, besti;
    GINGR_TRY(pack_shape_columns(ctx, M, model->perm, model->ref, model->mean, n_train, train_xyz, false, Tr, tp));
    HIP_TRY(ctx, A.alloc((size_t)ldmax * r * sizeof(double)));
    HIP_TRY(ctx, T.alloc((size_t)rp * ldmax * sizeof(double)));
    HIP_TRY(ctx, P.alloc((size_t)mp::block_rows(M) * ldmax * sizeof(double)));
    // (two block lengths exist, the full block and the last one: the partials of either fit)
    HIP_TRY(ctx, partial.alloc((size_t)std::max(mp::make_pair_plan(M, blocks.length(0), n_train).partial_doubles(),
                                                mp::make_pair_plan(M, blocks.length(blocks.count - 1), n_train).partial_doubles()) *
                               sizeof(double)));
    HIP_TRY(ctx, best.alloc((size_t)ldmax * sizeof(double)));
    HIP_TRY(ctx, besti.alloc((size_t)ldmax * sizeof(int32_t)));
    for (int64_t b = 0; b < blocks.count; ++b) {
        const int cnt = (int)blocks.length(b), ldt = (int)blocks.padded(b);
        const int64_t c0 = blocks.begin(b);
        const mp::PairPlan plan = mp::make_pair_plan(M, cnt, n_train);
        HIP_TRY(ctx, hipMemcpyAsync(A.p, alphas + c0 * r, (size_t)cnt * r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        for (int32_t q = 0; q < n_ranks; ++q) {
            launch_sample_factor(ctx, A.as<double>(), cnt, (int)r, (int)rl.k[q], (int)rp, ldt, T.as<double>());
            launch_instances(ctx, model, T.as<double>(), ldt, P.as<double>());
            {
                TimerScope ts(ctx, 19);
                hipLaunchKernelGGL(pair_distance_kernel, dim3((unsigned)plan.slabs, (unsigned)plan.tiles()), dim3(256), 0, ctx->stream, P.as<double>(),
                                   ldt, Tr.as<double>(), tp, M, plan.verts_per_slab, (int)plan.tiles_t, partial.as<double>());
            }
            hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, ctx->stream, partial.as<double>(), (int)plan.slabs, ldt,
                               tp, cnt, (int)n_train, M, best.as<double>(), besti.as<int32_t>());
            GINGR_TRY(check_launch(ctx));
            HIP_TRY(ctx, hipMemcpyAsync(min_avg + (size_t)q * n_samples + c0, best.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(argmin + (size_t)q * n_samples + c0, besti.p, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GINGR_OK;
}

}  // extern "C"
