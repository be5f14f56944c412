// The accumulator tiles of a basis x factor product on float64 MFMA and their store, shared by basis_rotate_kernel (posterior_model.hip:
// one source basis) and basis_rotate2_kernel (augment_model.hip: two source bases into the same tiles).
#pragma once
#include "fitter.h"
#include "gp_device.h"

typedef double d4 __attribute__((ext_vector_type(4)));

// augment_model.hip: C [a->rp][b->rp] = Q_a^T Q_b on ctx->stream, slab partials added in a fixed order.  Of a and b it reads M, Q0, rp
// and a->perm, b->iperm (the vertex at row s of a sits at row b->iperm[a->perm[s]] of b); ws: nslabs a->rp b->rp doubles (cross_gram_plan)
void cross_gram_plan(int64_t M, int32_t rpa, int32_t rpb, int *npa, int *npb, int *nslabs, int64_t *verts_per_slab);
void launch_cross_gram(gingr_ctx *ctx, const gingr_model *a, const gingr_model *b, double *ws, double *C);

constexpr int kRotWaves = 8;       // waves per workgroup, each with 16 vertices of its own (no LDS, no barrier); two per SIMD keep the
                                   // 96 accumulator registers in VGPRs (marginal_cov_kernel, posterior_cov.hip)
constexpr int kRotVerts = 16;      // vertices per wave = rows of one MFMA tile
constexpr int kRotChunkTiles = 4;  // column tiles of the result a wave holds (3 x 4 accumulator tiles = 96 registers)

// The column chunk [n0, n0 + 16 NT) of Q0_rows T for the wave's 16 vertices.  Tile layout of cov_chunk (posterior_cov.hip):
//   D(16x16) += A(16x4) B(4x16): lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D: lane holds column
//   j = l & 15 of the rows i = (l >> 4) + 4 reg.
// Row tile d holds coordinate d of the 16 vertices (A row i = source basis row 3 src(v0 + i) + d, rs columns wide), so the three coordinates of a vertex
// sit in the same lane and register of the three tiles: the rotation is three FMAs per output, no exchange.  The 16 k of a step are
// dealt to the four MFMAs as k0 + 4 (l >> 4) + t: a lane's four A values are 32 contiguous bytes (one load), B follows the same
// permutation of k.
template <int NT>
__device__ __forceinline__ void rotate_clear(v4f64 (&acc)[3][NT]) {
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[d][j] = v4f64{0, 0, 0, 0};
}

// acc += Q0_rows T for one source: qrow = the lane's source row 3 src(v0 + cl) (rs columns wide), T [rs][rp]
template <int NT>
__device__ __forceinline__ void rotate_accumulate(v4f64 (&acc)[3][NT], const double *__restrict__ qrow, int rs, int rp, const double *__restrict__ T,
                                                  int n0, int kq, int cl) {
    const double *tcol = T + (int64_t)(4 * kq) * rp + n0 + cl;
    for (int k0 = 0; k0 < rs; k0 += 16) {
        d4 a[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = *reinterpret_cast<const d4 *>(qrow + (int64_t)d * rs + k0 + 4 * kq);
        double b[4][NT];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < NT; ++j) b[t][j] = tcol[(int64_t)(k0 + t) * rp + 16 * j];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[d][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[d][t], b[t][j], acc[d][j], 0, 0, 0);
    }
}

// R acc stored.  For one register g and tile (d, j) the 16 lanes of a row of lanes write 128 contiguous, 128-byte aligned bytes of result
// row 3 (v0 + kq + 4 g) + d (rp is a multiple of 16), the four rows of lanes four such rows: every store instruction fills whole
// cache lines, and the NT tiles of a chunk complete 128 NT contiguous bytes of each row.
template <int NT>
__device__ __forceinline__ void rotate_store(const v4f64 (&acc)[3][NT], int rp, int n0, int kq, int cl, const Rot3 &rot, double *__restrict__ out,
                                             int64_t vleft) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int i = kq + 4 * g;  // vertex of the wave this register belongs to
        if (i >= vleft) continue;
        double *orow = out + (int64_t)3 * i * rp + n0 + cl;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const double x = acc[0][j][g], y = acc[1][j][g], z = acc[2][j][g];
#pragma unroll
            for (int d = 0; d < 3; ++d)
                orow[(int64_t)d * rp + 16 * j] = __builtin_fma(rot.R[3 * d], x, __builtin_fma(rot.R[3 * d + 1], y, rot.R[3 * d + 2] * z));
        }
    }
}
