// The inverse-Laplacian shape model without an n x n matrix (C ABI in include/gingr_hip.h: gingr_model_from_laplacian).  The kernel
// DiagonalKernel(LookupKernel(pinv(L)) scaling) has the eigenpairs (scaling / mu_j, v_j) of the sparse graph Laplacian L = D - A, each
// on x, y and z, so the leading 3 k components of the model are the k smallest non-zero eigenpairs of L: Chebyshev-filtered subspace
// iteration over a block X [n][m] (lap_spectral_plan.h holds every decision and the derivation of the degree rule):
//     filter     d fused steps T_next = alpha (L T_cur) + beta T_cur + gamma T_prev      (lap_cheb_kernel: the one pass of size n x m
//                                                                                          that runs d times per outer step)
//     deflate    the per-component column means subtracted (the null space of L)         (chunk partials, fixed order)
//     orthonorm. Cholesky-QR twice: X^T X (launch_gram), L^-T (dense_spd.hip), X L^-T    (lap_apply_kernel)
//     Ritz       [X | L X]^T [X | L X] in one Gram pass, its off-diagonal block through sym_eig, X V
//     residuals  |L x - theta x| / Lambda per column                                     (chunk partials, fixed order)
// The vertices are processed in the k-d leaf order of the reference (kd_order.h), the graph relabelled to it: the rows a vertex row
// gathers belong to spatial neighbours, which sit a few rows away.  No atomics, every sum in a fixed order: two builds of the same
// input give the same bits.  All working memory is allocated once per call (sym_eig keeps its own) and freed before return.
#include "dense_spd.h"
#include "fitter.h"
#include "lap_spectral_plan.h"
#include "nicp_graph.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

constexpr int kChebThreads = 256;
constexpr int kXcds = 8;          // workgroups are dealt to the XCDs round robin
constexpr int kSumChunkRows = 256;  // rows of one partial of a column sum
constexpr int kApplyRows = 8;     // rows of a wave of lap_apply_kernel

struct ChebArgs {
    const int32_t *row_ptr, *col;  // CSR of the graph in block-row labels, neighbours ascending
    const double *cur;             // T_cur, row stride ld_cur
    const double *prev;            // T_prev (nullable: gamma = 0), may be `next` itself
    double *next;                  // T_next; never `cur`
    double *copy;                  // nullable: also receives T_cur's own row (the left half of [X | L X])
    int64_t ld_cur, ld_prev, ld_next, ld_copy;
    int64_t n;
    int m, lanes_log2;             // columns; a row belongs to 2^lanes_log2 consecutive lanes (8 .. 64), 16 bytes per lane and pass
    double alpha, beta, gamma;
};

// One Chebyshev step for every vertex row: L T_cur = degree * own row - sum of the neighbour rows (ascending neighbours, one fixed
// order), then the three-term combination, all on 16-byte accesses.  A row's m doubles are read by 2^lanes_log2 consecutive lanes,
// two doubles each, in at most two passes (m <= 192): every access of a wave covers whole rows, contiguously.  Workgroup b of the
// launch takes the rows of slot (b mod 8) * (blocks / 8) + b / 8: an XCD works on one contiguous eighth of the k-d order, so the
// neighbour rows it gathers are mostly rows its own L2 has just seen.
__global__ __launch_bounds__(kChebThreads) void lap_cheb_kernel(ChebArgs a) {
    const int per_xcd = gridDim.x / kXcds;
    const int64_t slot = (int64_t)(blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds;
    const int lanes = 1 << a.lanes_log2;
    const int64_t i = slot * (kChebThreads >> a.lanes_log2) + (threadIdx.x >> a.lanes_log2);
    if (i >= a.n) return;
    const int sub = threadIdx.x & (lanes - 1);
    const int k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
    const double deg = (double)(k1 - k0);
    for (int c = 2 * sub; c < a.m; c += 2 * lanes) {
        const dbl2 own = *reinterpret_cast<const dbl2 *>(a.cur + i * a.ld_cur + c);
        dbl2 s = {0.0, 0.0};
        for (int k = k0; k < k1; ++k) s += *reinterpret_cast<const dbl2 *>(a.cur + (int64_t)a.col[k] * a.ld_cur + c);
        const dbl2 lx = deg * own - s;
        dbl2 tail = a.beta * own;
        if (a.prev) {
            const dbl2 p = *reinterpret_cast<const dbl2 *>(a.prev + i * a.ld_prev + c);
            tail = dbl2{__builtin_fma(a.gamma, p.x, tail.x), __builtin_fma(a.gamma, p.y, tail.y)};
        }
        *reinterpret_cast<dbl2 *>(a.next + i * a.ld_next + c) = dbl2{__builtin_fma(a.alpha, lx.x, tail.x), __builtin_fma(a.alpha, lx.y, tail.y)};
        if (a.copy) *reinterpret_cast<dbl2 *>(a.copy + i * a.ld_copy + c) = own;
    }
}

// splitmix64 of (original vertex, column) mapped to [-1, 1): the start block, the same for every run and every row order
__global__ __launch_bounds__(256) void lap_start_kernel(const int32_t *__restrict__ orig, int64_t n, int m, int active, double *__restrict__ X) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * m) return;
    const int64_t i = e / m;
    const int c = (int)(e - i * m);
    uint64_t z = (uint64_t)orig[i] * 0x9E3779B97F4A7C15ull + (uint64_t)(c + 1) * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    X[e] = c < active ? (double)(z >> 11) * 0x1p-52 - 1.0 : 0.0;
}

// ---- deflation: the rows of component q are list[.. ) in ascending order, cut into chunks of kSumChunkRows; chunk_ptr [chunks + 1] into
// list, comp_chunk [components + 1] into the chunks.  Three launches: chunk sums, component means, subtraction.
__global__ __launch_bounds__(256) void lap_chunk_sum_kernel(const double *__restrict__ X, int m, const int32_t *__restrict__ list,
                                                            const int32_t *__restrict__ chunk_ptr, double *__restrict__ part) {
    const int c = threadIdx.x;
    if (c >= m) return;
    double acc = 0.0;
    for (int t = chunk_ptr[blockIdx.x]; t < chunk_ptr[blockIdx.x + 1]; ++t) acc += X[(int64_t)list[t] * m + c];
    part[(int64_t)blockIdx.x * m + c] = acc;
}
__global__ __launch_bounds__(256) void lap_component_mean_kernel(const double *__restrict__ part, int m, const int32_t *__restrict__ chunk_ptr,
                                                                 const int32_t *__restrict__ comp_chunk, double *__restrict__ mean) {
    const int c = threadIdx.x, q = blockIdx.x;
    if (c >= m) return;
    const int b0 = comp_chunk[q], b1 = comp_chunk[q + 1];
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) acc += part[(int64_t)b * m + c];
    mean[(int64_t)q * m + c] = acc / (double)(chunk_ptr[b1] - chunk_ptr[b0]);
}
// (an isolated vertex is its own mean: its row becomes exactly 0)
__global__ __launch_bounds__(256) void lap_subtract_mean_kernel(double *__restrict__ X, int64_t n, int m, const int32_t *__restrict__ label,
                                                                const double *__restrict__ mean) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * m) return;
    const int64_t i = e / m;
    X[e] -= mean[(int64_t)label[i] * m + (e - i * m)];
}

// ---- residuals: part[b][c] = sum over the rows of chunk b of (LX - theta_c X)^2, then res[c] = sqrt(sum_b part[b][c]) / bound.
// evals: the Ritz values as sym_eig leaves them, DESCENDING over the `active` columns; column c of the rotated block has evals[active - 1 - c].
__global__ __launch_bounds__(256) void lap_residual_chunk_kernel(const double *__restrict__ X, const double *__restrict__ LX, int64_t n, int m,
                                                                 int active, const double *__restrict__ evals, double *__restrict__ part) {
    const int c = threadIdx.x;
    if (c >= m) return;
    const double theta = c < active ? evals[active - 1 - c] : 0.0;
    const int64_t r0 = (int64_t)blockIdx.x * kSumChunkRows, r1 = min(n, r0 + kSumChunkRows);
    double acc = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
        const double d = LX[i * m + c] - theta * X[i * m + c];
        acc = __builtin_fma(d, d, acc);
    }
    part[(int64_t)blockIdx.x * m + c] = acc;
}
__global__ __launch_bounds__(256) void lap_residual_finish_kernel(const double *__restrict__ part, int chunks, int m, double bound,
                                                                  double *__restrict__ res) {
    const int c = threadIdx.x;
    if (c >= m) return;
    double acc = 0.0;
    for (int b = 0; b < chunks; ++b) acc += part[(int64_t)b * m + c];
    res[c] = sqrt(acc) / bound;
}

// out[i][c] = sum_{k < active} in[i][k] W[k][c] for c < active, 0 for active <= c < m: the block times a small matrix (L^-T of the
// Cholesky-QR, the Ritz rotation).  A wave takes kApplyRows rows and all columns (three per lane at most); the row values are
// wave-uniform, W streams from L2 once per kApplyRows rows.  in != out.
__global__ __launch_bounds__(256) void lap_apply_kernel(const double *__restrict__ in, int64_t n, int m, int active, const double *__restrict__ W,
                                                        int64_t ldw, double *__restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * kApplyRows;
    if (r0 >= n) return;
    const double *row[kApplyRows];
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r) row[r] = in + min(r0 + r, n - 1) * m;
    double acc[kApplyRows][3];
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r)
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[r][t] = 0.0;
    for (int k = 0; k < active; ++k) {
        double w[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) w[t] = lane + 64 * t < active ? W[(int64_t)k * ldw + lane + 64 * t] : 0.0;
#pragma unroll
        for (int r = 0; r < kApplyRows; ++r) {
            const double x = row[r][k];
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[r][t] = __builtin_fma(x, w[t], acc[r][t]);
        }
    }
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r) {
        if (r0 + r >= n) break;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int c = lane + 64 * t;
            if (c < m) out[(r0 + r) * m + c] = c < active ? acc[r][t] : 0.0;
        }
    }
}

// H [active][active] (row stride m) = the symmetric part of the block X^T (L X) of G2 = [X | LX]^T [X | LX] ([2m][2m])
__global__ __launch_bounds__(256) void lap_ritz_matrix_kernel(const double *__restrict__ G2, int m, int active, double *__restrict__ H) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= active * active) return;
    const int i = e / active, j = e - i * active;
    H[i * m + j] = 0.5 * (G2[(int64_t)i * 2 * m + m + j] + G2[(int64_t)j * 2 * m + m + i]);
}
// W [m][m]: W[k][c] = component k of the eigenvector of the c-th SMALLEST Ritz value (Vs: [active][active], values descending)
__global__ __launch_bounds__(256) void lap_rotation_kernel(const double *__restrict__ Vs, int m, int active, double *__restrict__ W) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int k = e / m, c = e - k * m;
    W[e] = (k < active && c < active) ? Vs[k * active + (active - 1 - c)] : 0.0;
}

struct SpdPlain {  // the lower triangle of a Gram matrix of row stride ld
    const double *__restrict__ G;
    int ld;
    __device__ double operator()(int64_t row, int64_t c) const { return G[row * ld + c]; }
};

// scale[j] = +-base[j]: the sign that makes the component of largest magnitude of column col0 + j positive, the lowest ORIGINAL vertex
// on a tie.  One workgroup per column, the candidates of its threads combined by thread 0 in thread order.
__global__ __launch_bounds__(256) void lap_sign_kernel(const double *__restrict__ X, int64_t n, int m, int col0, const int32_t *__restrict__ orig,
                                                       const double *__restrict__ base, double *__restrict__ scale) {
    __shared__ double sv[256];
    __shared__ int32_t so[256];
    const int j = blockIdx.x, c = col0 + j;
    double best = 0.0;
    int32_t best_o = INT32_MAX;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double v = X[i * m + c];
        const int32_t o = orig[i];
        if (fabs(v) > fabs(best) || (fabs(v) == fabs(best) && o < best_o)) best = v, best_o = o;
    }
    sv[threadIdx.x] = best;
    so[threadIdx.x] = best_o;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t)
            if (fabs(sv[t]) > fabs(best) || (fabs(sv[t]) == fabs(best) && so[t] < best_o)) best = sv[t], best_o = so[t];
        scale[j] = best < 0.0 ? -base[j] : base[j];
    }
}

// The model's basis: Q0[3 s + d][3 j + d] = X[pos(perm[s])][col0 + j] scale[j], every other entry 0 (padding columns included).
// perm: the model's device row -> original vertex; pos: original vertex -> row of the block.
__global__ __launch_bounds__(256) void lap_expand_kernel(const double *__restrict__ X, int m, int col0, int k, const double *__restrict__ scale,
                                                         const int32_t *__restrict__ perm, const int32_t *__restrict__ pos, int64_t M, int rp,
                                                         double *__restrict__ Q0) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * M * rp) return;
    const int64_t row = e / rp;
    const int q = (int)(e - row * rp);
    const int64_t s = row / 3;
    const int d = (int)(row - 3 * s), j = q / 3;
    Q0[e] = (j < k && q - 3 * j == d) ? X[(int64_t)pos[perm[s]] * m + col0 + j] * scale[j] : 0.0;
}

struct LapSolver {
    gingr_ctx *ctx = nullptr;
    int64_t n = 0, n3 = 0;  // vertices; rounded up to a multiple of 3 (launch_gram takes rows three at a time)
    int m = 0, active = 0, chunks = 0, res_chunks = 0, ncomp = 0;
    double bound = 0.0;
    DevBuf row_ptr, col, orig, label, list, chunk_ptr, comp_chunk;
    DevBuf A, B, C, Z, gws, G, H, W, spd, evals, Vs, part, mean, res;

    int64_t block_doubles(int width) const { return (n3 + kBasisRowSlack) * (int64_t)width; }

    // next = alpha (L cur) + beta cur + gamma prev; `copy` (nullable) also gets cur's rows
    void cheb(const double *cur, int64_t ld_cur, const double *prev, double *next, int64_t ld_next, double *copy, int64_t ld_copy, LapStep s) {
        ChebArgs a;
        a.row_ptr = row_ptr.as<int32_t>();
        a.col = col.as<int32_t>();
        a.cur = cur;
        a.prev = prev;
        a.next = next;
        a.copy = copy;
        a.ld_cur = ld_cur;
        a.ld_prev = m;
        a.ld_next = ld_next;
        a.ld_copy = ld_copy;
        a.n = n;
        a.m = m;
        a.lanes_log2 = m <= 16 ? 3 : m <= 32 ? 4 : m <= 64 ? 5 : 6;
        a.alpha = s.alpha;
        a.beta = s.beta;
        a.gamma = s.gamma;
        const int64_t rows_per_block = kChebThreads >> a.lanes_log2;
        const int64_t blocks = round_up(ceil_div(n, rows_per_block), kXcds);
        TimerScope ts(ctx, 17);
        hipLaunchKernelGGL(lap_cheb_kernel, dim3((unsigned)blocks), dim3(kChebThreads), 0, ctx->stream, a);
    }
    void deflate(double *X) {
        hipLaunchKernelGGL(lap_chunk_sum_kernel, dim3((unsigned)chunks), dim3(256), 0, ctx->stream, X, m, list.as<int32_t>(),
                           chunk_ptr.as<int32_t>(), part.as<double>());
        hipLaunchKernelGGL(lap_component_mean_kernel, dim3((unsigned)ncomp), dim3(256), 0, ctx->stream, part.as<double>(), m,
                           chunk_ptr.as<int32_t>(), comp_chunk.as<int32_t>(), mean.as<double>());
        hipLaunchKernelGGL(lap_subtract_mean_kernel, dim3((unsigned)ceil_div(n * m, 256)), dim3(256), 0, ctx->stream, X, n, m, label.as<int32_t>(),
                           mean.as<double>());
    }
    void apply(const double *in, const double *Wm, int64_t ldw, double *out) {
        hipLaunchKernelGGL(lap_apply_kernel, dim3((unsigned)ceil_div(n, 4 * kApplyRows)), dim3(256), 0, ctx->stream, in, n, m, active, Wm, ldw, out);
    }
    // out = in R^-T with in^T in = R R^T (one pass of Cholesky-QR); in != out
    int cholesky_qr_pass(const double *in, double *out) {
        launch_gram(ctx, in, n3 / 3, m, nullptr, gws.as<double>(), G.as<double>());
        const DenseSpdWork ws(m, DenseSpdWork::kIdentity);
        double *work = spd.as<double>();
        int32_t *flag = reinterpret_cast<int32_t *>(work + ws.flag());
        launch_spd_system(ctx->stream, active, ws, SpdPlain{G.as<double>(), m}, SpdIdentityBorder{}, work + ws.aw(), flag);
        dense_spd_inverse(ctx, work + ws.aw(), ws.Mp, work + ws.linv(), nullptr, flag);
        apply(in, work + ws.lt(), ws.Mp, out);
        GINGR_TRY(check_launch(ctx));
        int32_t h = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&h, flag, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (h != 0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "model_from_laplacian: the Gram matrix of the block is not positive definite");
        return GINGR_OK;
    }
};

}  // namespace

extern "C" {

int gingr_model_from_laplacian(gingr_ctx *ctx, int64_t M, const double *ref_xyz, int64_t n_cells, const int32_t *cells, double scaling,
                               int32_t n_pairs, double tolerance, int32_t max_degree, gingr_laplacian_info *info, gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    const char *who = "model_from_laplacian";
    if (!ref_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (M < 1 || M > (int64_t)0x7fffffff / 3) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: M = %lld outside the supported range", who, (long long)M);
    if (n_pairs < 1 || n_pairs > kLapMaxPairs)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n_pairs = %d, need 1 <= n_pairs <= %d (a model holds 512 components)", who,
                               (int)n_pairs, kLapMaxPairs);
    if (n_cells < 1 || !cells) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: no cells: the Laplacian needs the triangulation", who);
    if (!(scaling > 0.0) || !std::isfinite(scaling)) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: scaling must be positive", who);
    for (int64_t e = 0; e < 3 * M; ++e)
        if (!std::isfinite(ref_xyz[e])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite reference coordinate", who);
    const int k = n_pairs;
    const double tol = tolerance > 0.0 ? tolerance : kLapDefaultTolerance;
    const int budget = max_degree > 0 ? max_degree : kLapDefaultMaxDegree;

    // ---- the graph in the k-d order of the reference
    std::vector<int32_t> edges;
    int64_t bad = -1;
    switch (lap_edges_from_cells(M, n_cells, cells, &edges, &bad)) {
        case LAP_EDGES_OK: break;
        case LAP_EDGES_BAD_INDEX:
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: cell %lld names a vertex outside [0, %lld)", who, (long long)bad, (long long)M);
        default: return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: too many cells", who);
    }
    std::vector<int32_t> perm, pos((size_t)M);  // perm[s] = original vertex of block row s; pos = its inverse
    kd_leaf_order(ref_xyz, M, perm);
    for (int64_t s = 0; s < M; ++s) pos[(size_t)perm[(size_t)s]] = (int32_t)s;
    for (size_t e = 0; e < edges.size(); e += 2) {
        const int32_t a = pos[(size_t)edges[e]], b = pos[(size_t)edges[e + 1]];
        edges[e] = std::min(a, b);
        edges[e + 1] = std::max(a, b);
    }
    NicpGraph g;
    if (nicp_graph_build(M, (int64_t)edges.size() / 2, edges.data(), &g, &bad) != NICP_GRAPH_OK)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: the edge graph could not be built (edge %lld)", who, (long long)bad);
    const int64_t dim = M - g.n_components;
    if (info) info->n_components = g.n_components, info->n_dropped = g.n_components;
    if (k > dim)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: n_pairs = %d, but the Laplacian has only %lld eigenvalues above the cut-off", who, k,
                               (long long)dim);
    int32_t max_deg = 0;
    for (int64_t i = 0; i < M; ++i) max_deg = std::max(max_deg, g.degree[(size_t)i]);
    const LapBlock blk = lap_block_plan(k, dim);
    if (info) info->block_columns = blk.m;

    // rows by component (ascending inside each), cut into chunks
    std::vector<int32_t> list((size_t)M), chunk_ptr, comp_chunk((size_t)g.n_components + 1, 0);
    {
        std::vector<int32_t> start((size_t)g.n_components + 1, 0);
        for (int64_t i = 0; i < M; ++i) ++start[(size_t)g.component[(size_t)i] + 1];
        for (int32_t q = 0; q < g.n_components; ++q) start[(size_t)q + 1] += start[(size_t)q];
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < M; ++i) list[(size_t)fill[(size_t)g.component[(size_t)i]]++] = (int32_t)i;
        for (int32_t q = 0; q < g.n_components; ++q) {
            comp_chunk[(size_t)q] = (int32_t)chunk_ptr.size();
            for (int32_t t = start[(size_t)q]; t < start[(size_t)q + 1]; t += kSumChunkRows) chunk_ptr.push_back(t);
        }
        comp_chunk[(size_t)g.n_components] = (int32_t)chunk_ptr.size();
        chunk_ptr.push_back((int32_t)M);
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LapSolver s;
    s.ctx = ctx;
    s.n = M;
    s.n3 = round_up(M, 3);
    s.m = blk.m;
    s.active = blk.active;
    s.ncomp = g.n_components;
    s.chunks = (int)chunk_ptr.size() - 1;
    s.res_chunks = (int)ceil_div(M, kSumChunkRows);
    s.bound = 2.0 * (double)max_deg;
    const int m = s.m, active = s.active;
    auto upload = [&](DevBuf &b, const std::vector<int32_t> &v) -> int {
        HIP_TRY(ctx, b.alloc(std::max<size_t>(v.size(), 1) * sizeof(int32_t)));
        if (!v.empty()) HIP_TRY(ctx, hipMemcpy(b.p, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return GINGR_OK;
    };
    GINGR_TRY(upload(s.row_ptr, g.row_ptr));
    GINGR_TRY(upload(s.col, g.col));
    GINGR_TRY(upload(s.orig, perm));
    GINGR_TRY(upload(s.label, g.component));
    GINGR_TRY(upload(s.list, list));
    GINGR_TRY(upload(s.chunk_ptr, chunk_ptr));
    GINGR_TRY(upload(s.comp_chunk, comp_chunk));
    const DenseSpdWork spd_ws(m, DenseSpdWork::kIdentity);
    DevBuf *blocks[] = {&s.A, &s.B, &s.C};
    for (DevBuf *b : blocks) {  // (the rows behind the n-th stay zero: the Gram pass reads them)
        HIP_TRY(ctx, b->alloc((size_t)s.block_doubles(m) * sizeof(double)));
        HIP_TRY(ctx, hipMemsetAsync(b->p, 0, b->bytes, ctx->stream));
    }
    HIP_TRY(ctx, s.Z.alloc((size_t)s.block_doubles(2 * m) * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(s.Z.p, 0, s.Z.bytes, ctx->stream));
    HIP_TRY(ctx, s.gws.alloc((size_t)std::max(gram_ws_doubles(s.n3 / 3, m), gram_ws_doubles(s.n3 / 3, 2 * m)) * sizeof(double)));
    HIP_TRY(ctx, s.G.alloc((size_t)4 * m * m * sizeof(double)));
    HIP_TRY(ctx, s.H.alloc((size_t)m * m * sizeof(double)));
    HIP_TRY(ctx, s.W.alloc((size_t)m * m * sizeof(double)));
    HIP_TRY(ctx, s.spd.alloc((size_t)spd_ws.doubles() * sizeof(double)));
    HIP_TRY(ctx, s.evals.alloc((size_t)m * sizeof(double)));
    HIP_TRY(ctx, s.Vs.alloc((size_t)m * m * sizeof(double)));
    HIP_TRY(ctx, s.part.alloc((size_t)std::max(s.chunks, s.res_chunks) * m * sizeof(double)));
    HIP_TRY(ctx, s.mean.alloc((size_t)s.ncomp * m * sizeof(double)));
    HIP_TRY(ctx, s.res.alloc((size_t)m * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(s.H.p, 0, s.H.bytes, ctx->stream));

    double *X = s.A.as<double>(), *Y = s.B.as<double>(), *T = s.C.as<double>();  // X: the block; Y, T: the other two buffers
    // X = the orthonormalised, deflated start block
    hipLaunchKernelGGL(lap_start_kernel, dim3((unsigned)ceil_div(M * m, 256)), dim3(256), 0, ctx->stream, s.orig.as<int32_t>(), M, m, active, X);
    s.deflate(X);
    GINGR_TRY(s.cholesky_qr_pass(X, Y));
    GINGR_TRY(s.cholesky_qr_pass(Y, X));

    std::vector<double> theta((size_t)active), res((size_t)m), desc((size_t)active);
    int wanted = k, total = 0, outer = 0;
    double max_res = 0.0;
    auto report = [&](int converged) {
        if (!info) return;
        info->outer_iterations = outer;
        info->total_degree = total;
        info->converged = converged;
        info->max_residual = max_res;
    };
    auto out_of_budget = [&]() {
        report(0);
        return gingr_set_error(ctx, GINGR_ERR_NOT_CONVERGED,
                               "%s: residual %.3g above the tolerance %.3g after %d block products with L (the budget is %d)", who, max_res, tol,
                               total, budget);
    };
    double *Zl = s.Z.as<double>(), *Zr = Zl + m;
    for (;;) {
        if (total + 2 > budget) return out_of_budget();
        // ---- Rayleigh-Ritz: [X | L X], its Gram matrix, the eigen-decomposition of X^T L X, X := X V (ascending), L X again
        s.cheb(X, m, nullptr, Zr, 2 * m, Zl, 2 * m, LapStep{1.0, 0.0, 0.0});
        launch_gram(ctx, Zl, s.n3 / 3, 2 * m, nullptr, s.gws.as<double>(), s.G.as<double>());
        hipLaunchKernelGGL(lap_ritz_matrix_kernel, dim3((unsigned)ceil_div(active * active, 256)), dim3(256), 0, ctx->stream, s.G.as<double>(), m,
                           active, s.H.as<double>());
        GINGR_TRY(check_launch(ctx));
        GINGR_TRY(launch_jacobi_eig(ctx, s.H.as<double>(), m, active, s.evals.as<double>(), s.Vs.as<double>()));
        hipLaunchKernelGGL(lap_rotation_kernel, dim3((unsigned)ceil_div(m * m, 256)), dim3(256), 0, ctx->stream, s.Vs.as<double>(), m, active,
                           s.W.as<double>());
        s.apply(X, s.W.as<double>(), m, Y);
        std::swap(X, Y);
        s.cheb(X, m, nullptr, T, m, nullptr, 0, LapStep{1.0, 0.0, 0.0});
        total += 2;
        hipLaunchKernelGGL(lap_residual_chunk_kernel, dim3((unsigned)s.res_chunks), dim3(256), 0, ctx->stream, X, T, M, m, active,
                           s.evals.as<double>(), s.part.as<double>());
        hipLaunchKernelGGL(lap_residual_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, s.part.as<double>(), s.res_chunks, m, s.bound,
                           s.res.as<double>());
        GINGR_TRY(check_launch(ctx));
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), s.res.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(desc.data(), s.evals.p, (size_t)active * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        max_res = 0.0;
        for (int j = 0; j < active; ++j) {
            theta[(size_t)j] = desc[(size_t)(active - 1 - j)];
            if (!std::isfinite(theta[(size_t)j]) || !std::isfinite(res[(size_t)j])) {
                report(0);
                return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "%s: non-finite Ritz pair", who);
            }
            if (j < wanted) max_res = std::max(max_res, res[(size_t)j]);
        }
        if (lap_converged(res.data(), wanted, tol)) {
            const int t = lap_count_dropped(theta.data(), wanted);
            if (k + t > dim) {
                report(0);
                return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT,
                                       "%s: n_pairs = %d, but the Laplacian has only %lld eigenvalues above the cut-off", who, k,
                                       (long long)(dim - t));
            }
            if (k + t <= wanted) break;
            wanted = k + t;  // eigenvalues at or below the cut-off besides the components' null vectors: that many more pairs
            if (wanted > active - (active < dim ? 1 : 0)) {
                report(0);
                return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "%s: %d eigenvalues at or below the cut-off leave no room for %d pairs in a block of %d",
                                       who, t, k, active);
            }
            continue;
        }
        const int left = budget - total - 2;  // (the Rayleigh-Ritz step behind the filter takes two products)
        if (left < 1) return out_of_budget();
        // ---- the filter: Y_d = p_d(L) X by the scaled three-term recurrence, ping-pong between two buffers
        const LapFilter f = lap_filter_plan(theta[(size_t)active - 1], s.bound, left);
        double sigma = 0.0;
        double *prev = nullptr, *cur = X, *spare = Y;
        for (int step = 1; step <= f.degree; ++step) {
            const LapStep cs = lap_recurrence_step(f, step, &sigma);
            double *next = prev ? prev : spare;  // (T_next may overwrite T_prev: a row reads its own T_prev entries only)
            s.cheb(cur, m, prev, next, m, nullptr, 0, cs);
            prev = cur;
            cur = next;
        }
        total += f.degree;
        ++outer;
        s.deflate(cur);
        GINGR_TRY(s.cholesky_qr_pass(cur, T));
        double *other = cur == X ? Y : X;
        GINGR_TRY(s.cholesky_qr_pass(T, other));
        X = other;
        Y = cur;
    }
    const int t = wanted - k;  // leading pairs at or below the cut-off: dropped
    report(1);
    if (info) {
        info->n_dropped = g.n_components + t;
        info->cut_gap = t + k < active ? (theta[(size_t)(t + k)] - theta[(size_t)(t + k - 1)]) / theta[(size_t)(t + k - 1)]
                                       : std::numeric_limits<double>::infinity();
    }

    // ---- the model: variance scaling / mu_j on x, y and z; basis v_j on one coordinate each, sign fixed
    std::vector<double> var((size_t)3 * k), base((size_t)k), zero((size_t)3 * M, 0.0);
    for (int j = 0; j < k; ++j) {
        const double v = scaling / theta[(size_t)(t + j)];
        base[(size_t)j] = std::sqrt(v);
        for (int d = 0; d < 3; ++d) var[(size_t)3 * j + d] = v;
    }
    DevBuf dbase, dscale, dpos;
    HIP_TRY(ctx, dbase.alloc((size_t)k * sizeof(double)));
    HIP_TRY(ctx, dscale.alloc((size_t)k * sizeof(double)));
    HIP_TRY(ctx, hipMemcpy(dbase.p, base.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice));
    GINGR_TRY(upload(dpos, pos));
    hipLaunchKernelGGL(lap_sign_kernel, dim3((unsigned)k), dim3(256), 0, ctx->stream, X, M, m, t, s.orig.as<int32_t>(), dbase.as<double>(),
                       dscale.as<double>());
    GINGR_TRY(check_launch(ctx));
    auto fill = [&](gingr_model *nm) -> int {
        hipLaunchKernelGGL(lap_expand_kernel, dim3((unsigned)ceil_div(3 * M * nm->rp, 256)), dim3(256), 0, ctx->stream, X, m, t, k,
                           dscale.as<double>(), nm->perm, dpos.as<int32_t>(), M, (int)nm->rp, nm->Q0);
        return check_launch(ctx);
    };
    return model_create_impl(ctx, M, 3 * k, ref_xyz, zero.data(), var.data(), 0, M, fill, out);
}

}  // extern "C"
