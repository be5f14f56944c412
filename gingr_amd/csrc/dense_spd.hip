// The multi-workgroup blocked Cholesky of a dense SPD system (dense_spd.h): right-looking, 64-wide panels -- diagonal block in LDS
// (one workgroup, chol_block64_kernel), panel and trailing update as 64 x 64 MFMA tiles (v_mfma_f64_16x16x4) over the whole chip --
// with the border rows riding along: right-hand sides (the forward substitution is a by-product; dense_spd_solve3 adds the blocked
// backward substitution) or an identity, which comes back as L^-T (dense_spd_inverse).
#include "dense_spd.h"
#include "solve_blocks.h"

namespace {

constexpr int kNBc = DenseSpdWork::kBlock;  // Cholesky panel width

// Diagonal block of the blocked Cholesky: factor the 64 x 64 block k of the
// row-major matrix Aw in LDS with the building blocks of solve_blocks.h and invert the factor on the way -- the identity rides along as 64
// extra rows, which come back as (L^-1 e_c)^T = row c of L^-T.  Aw block <- L (upper part zeroed), Linv[k] <- L^-1 (64 x 64, dense).
__global__ __launch_bounds__(256) void chol_block64_kernel(double *__restrict__ Aw, int64_t ld, int k, double *__restrict__ Linv,
                                                           int32_t *__restrict__ flag) {
    extern __shared__ double lds_sm[];
    constexpr int n = 64, lda = 65;  // solve_ld(64)
    double *A = lds_sm, *rd = A + 2 * n * lda;
    __shared__ int bad;
    const int tid = threadIdx.x;
    double *blk = Aw + ((int64_t)k * n) * ld + (int64_t)k * n;
#ifdef GINGR_CHOL64_STAMPS
    GINGR_STAGE_CLOCK(7)
#endif
    {   // the sixteen entries of a thread requested together (one memory round trip; as a load-store loop this stage was 8.6k of
        // the kernel's 40k cycles: every iteration waited for its own load)
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q;
            v[q] = blk[(int64_t)(e >> 6) * ld + (e & 63)];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q, r = e >> 6, c = e & 63;
            A[r * lda + c] = v[q];
            A[(n + r) * lda + c] = r == c ? 1.0 : 0.0;
        }
    }
    if (tid == 0) bad = 0;
    __syncthreads();
#ifdef GINGR_CHOL64_STAMPS  // tools/ubench_chol_block64.hip only
    GINGR_STAGE_CLOCK(0)
#endif
    lds_cholesky<256, true>(A, lda, n, rd, &bad, n);
#ifdef GINGR_CHOL64_STAMPS
    GINGR_STAGE_CLOCK(1)
#endif
    double *li = Linv + (int64_t)k * n * n;
    for (int e = tid; e < n * n; e += 256) {
        const int r = e >> 6, c = e & 63;
        blk[(int64_t)r * ld + c] = c <= r ? A[r * lda + c] : 0.0;
        li[e] = c <= r ? A[(n + c) * lda + r] : 0.0;
    }
    if (tid == 0 && bad) *flag = GINGR_ERR_NOT_SPD;
#ifdef GINGR_CHOL64_STAMPS
    GINGR_STAGE_CLOCK(4)
    GINGR_STAGE_CLOCK(6)
#endif
}

// one 64 x 64 tile on the matrix pipe: D = (accumulate ? C : 0) + beta * A B^T with A = 64 rows of Ap, B = 64 rows of Bp, K = 64.
// Both operands are staged through LDS in two halves of 32 columns (coalesced 256-byte row segments in, conflict-free fragment
// reads out; a panel tile that overwrites its own A operand is safe because A is consumed from LDS before C is written).
// Fragment layout of v_mfma_f64_16x16x4: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds
// D[i = (l >> 4) + 4 reg][j = l & 15]; wave w owns the output rows 16 w .. 16 w + 15.
__device__ __forceinline__ void tile_abt(const double *Ap, int64_t lda, const double *Bp, int64_t ldb, double *Cp, int64_t ldc,
                                         bool accumulate, double beta) {
    __shared__ double As[kNBc][33], Bs[kNBc][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    v4f64 acc[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const double *pc = Cp + (int64_t)(16 * wave + l4) * ldc + 16 * tj + l15;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[tj][g] = accumulate ? pc[(int64_t)4 * g * ldc] : 0.0;
    }
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        double va[8], vb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, r = e >> 5, c = e & 31;
            va[u] = Ap[(int64_t)r * lda + 32 * half + c];
            vb[u] = Bp[(int64_t)r * ldb + 32 * half + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, r = e >> 5, c = e & 31;
            As[r][c] = beta * va[u];
            Bs[r][c] = vb[u];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double a = As[16 * wave + l15][4 * q + l4];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[16 * tj + l15][4 * q + l4], acc[tj], 0, 0, 0);
        }
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        double *pc = Cp + (int64_t)(16 * wave + l4) * ldc + 16 * tj + l15;
#pragma unroll
        for (int g = 0; g < 4; ++g) pc[(int64_t)4 * g * ldc] = acc[tj][g];
    }
}

// panel solve: L_ik = A_ik L_kk^-T for the row blocks i > k (the last one is the border with the right-hand sides)
// (inverse: the border is an identity block of nb block rows -- dense_spd_inverse -- whose block row b is still zero left of column b)
__global__ __launch_bounds__(256) void chol_panel_kernel(double *__restrict__ Aw, int64_t ld, int k, const double *__restrict__ Linv, int nb,
                                                         bool inverse) {
    const int64_t i = k + 1 + blockIdx.x;
    if (inverse && i >= nb && i - nb > k) return;
    double *aik = Aw + i * kNBc * ld + (int64_t)k * kNBc;
    tile_abt(aik, ld, Linv + (int64_t)k * kNBc * kNBc, kNBc, aik, ld, false, 1.0);
}

// trailing update: A_ij -= L_ik L_jk^T for k < j <= i (j a matrix block, i up to the border block)
__global__ __launch_bounds__(256) void chol_trailing_kernel(double *__restrict__ Aw, int64_t ld, int k, int nb, bool inverse) {
    const int64_t i = k + 1 + blockIdx.y, j = k + 1 + blockIdx.x;
    if (j > i || j >= nb) return;
    if (inverse && i >= nb && i - nb > k) return;
    tile_abt(Aw + i * kNBc * ld + (int64_t)k * kNBc, ld, Aw + j * kNBc * ld + (int64_t)k * kNBc, ld, Aw + i * kNBc * ld + j * kNBc, ld, true,
             -1.0);
}

// backward substitution L^T W = Z, step k (from the last panel to the first): every workgroup forms W_k = L_kk^-T Z_k from the border
// rows; workgroup j < k then applies Z_j -= L_kj^T W_k, workgroup k stores W_k (planes of stride Mp)
__global__ __launch_bounds__(256) void chol_backward_kernel(double *__restrict__ Aw, int64_t ld, int64_t Mp, int k,
                                                            const double *__restrict__ Linv, double *__restrict__ W) {
    __shared__ double Z[3][kNBc], Wk[3][kNBc];
    const int tid = threadIdx.x, c = tid & 63, d = tid >> 6;
    const int64_t kb = (int64_t)k * kNBc;
    if (d < 3) Z[d][c] = Aw[(Mp + d) * ld + kb + c];
    __syncthreads();
    if (d < 3) {
        const double *li = Linv + (int64_t)k * kNBc * kNBc;
        double v = 0.0;
#pragma unroll 16
        for (int p = 0; p < kNBc; ++p) v += li[p * kNBc + c] * Z[d][p];  // Linv is lower triangular: the entries p < c are zero
        Wk[d][c] = v;
    }
    __syncthreads();
    if (d >= 3) return;
    const int j = blockIdx.x;
    if (j == k) {
        W[(int64_t)d * Mp + kb + c] = Wk[d][c];
        return;
    }
    const int64_t jb = (int64_t)j * kNBc;
    double v = 0.0;
    const double *lkj = Aw + kb * ld + jb + c;
#pragma unroll 16
    for (int p = 0; p < kNBc; ++p) v += lkj[(int64_t)p * ld] * Wk[d][p];
    Aw[(Mp + d) * ld + jb + c] -= v;
}

}  // namespace

// factor the 64 x 64 diagonal block k of the row-major matrix Aw (leading dimension ld) in place and store its inverse in Linv[k];
// *flag = GINGR_ERR_NOT_SPD on a bad pivot
static void launch_chol_block64(gingr_ctx *ctx, double *Aw, int64_t ld, int k, double *Linv, int32_t *flag) {
    const size_t lds = lds_solve_doubles(64, 64) * sizeof(double);
    // (the attribute is per function AND per device, and the group's worker threads launch concurrently: set whenever needed)
    if (lds > 48 * 1024)
        set_dynamic_lds(&chol_block64_kernel, (size_t)(lds));
    hipLaunchKernelGGL(chol_block64_kernel, dim3(1), dim3(256), lds, ctx->stream, Aw, ld, k, Linv, flag);
}

// the factorisation both entry points share (dense_spd.h); inverse: the border is an identity of nb block rows
static void blocked_cholesky(gingr_ctx *ctx, double *Aw, int64_t Mp, double *Linv, int32_t *flag, bool inverse) {
    const int nb = (int)(Mp / kNBc);
    const int nrows = inverse ? 2 * nb : nb + 1;  // block rows: the matrix, then the border
    for (int k = 0; k < nb; ++k) {
        launch_chol_block64(ctx, Aw, Mp, k, Linv, flag);
        const int below = inverse ? nb + k + 1 : nrows;  // (inverse: border block rows past k are still zero)
        hipLaunchKernelGGL(chol_panel_kernel, dim3((unsigned)(below - k - 1)), dim3(256), 0, ctx->stream, Aw, Mp, k, Linv, nb, inverse);
        if (k + 1 < nb)
            hipLaunchKernelGGL(chol_trailing_kernel, dim3((unsigned)(nb - k - 1), (unsigned)(below - k - 1)), dim3(256), 0, ctx->stream, Aw, Mp,
                               k, nb, inverse);
    }
}

void dense_spd_solve3(gingr_ctx *ctx, double *Aw, int64_t Mp, double *Linv, double *W, int32_t *flag) {
    blocked_cholesky(ctx, Aw, Mp, Linv, flag, false);
    const int nb = (int)(Mp / kNBc);
    if (!W) return;  // (the factor alone: the lower triangle of Aw then holds L)
    for (int k = nb - 1; k >= 0; --k)
        hipLaunchKernelGGL(chol_backward_kernel, dim3((unsigned)(k + 1)), dim3(256), 0, ctx->stream, Aw, Mp, Mp, k, Linv, W);
}

namespace {
// C tile (a, b) = sum over the column blocks kb >= max(a, b) of X_a,kb X_b,kb^T, X = L^-T (upper triangular, row stride ld)
__global__ __launch_bounds__(256) void inverse_product_kernel(const double *__restrict__ X, int64_t ld, int nb, double *__restrict__ C) {
    const int a = blockIdx.y, b = blockIdx.x;
    double *c = C + (int64_t)a * kNBc * ld + (int64_t)b * kNBc;
    bool first = true;
    for (int kb = a > b ? a : b; kb < nb; ++kb) {
        tile_abt(X + (int64_t)a * kNBc * ld + (int64_t)kb * kNBc, ld, X + (int64_t)b * kNBc * ld + (int64_t)kb * kNBc, ld, c, ld, !first, 1.0);
        first = false;
        __syncthreads();
    }
}
}  // namespace

// The inverse of an SPD matrix on the matrix pipe.  Aw: (2 Mp) x Mp, Mp a multiple of 64 -- the lower triangle of A on top of an
// IDENTITY: the blocked Cholesky takes the identity along as border rows, which leaves L^-T there (the rows of a border X become
// X L^-T), and A^-1 = L^-T L^-1 is one product of that triangle with itself.  C: Mp x Mp, all of it written (exactly symmetric).
// *flag receives GINGR_ERR_NOT_SPD when a diagonal block fails.  Linv: (Mp / 64) blocks of 64 x 64.
// C == nullptr: the factor alone -- L^-T stays behind in the border rows (Aw + Mp * Mp, upper triangular, row stride Mp).
void dense_spd_inverse(gingr_ctx *ctx, double *Aw, int64_t Mp, double *Linv, double *C, int32_t *flag) {
    blocked_cholesky(ctx, Aw, Mp, Linv, flag, true);
    if (!C) return;
    const int nb = (int)(Mp / kNBc);
    hipLaunchKernelGGL(inverse_product_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, ctx->stream, Aw + Mp * Mp, Mp, nb, C);
}
