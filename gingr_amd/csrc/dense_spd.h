// The multi-workgroup blocked Cholesky of a dense SPD system (dense_spd.hip): the layout of its workspace, the kernel that writes the
// bordered system, the solve and the inverse.  Internal to libgingr_hip.so.
#pragma once

#include <cstdint>

struct gingr_ctx;

// One workspace of the blocked solve, in doubles from its start.  Aw is (Mp + border rows) x Mp row-major, Mp a multiple of 64: the
// lower triangle of the SPD matrix (identity on the padding) on top of the border --
//   kRhsRows    64 rows, the right-hand sides in the first of them (three at most: dense_spd_solve3);  then Linv, W (three planes of
//               stride Mp), the flag (two doubles: a second system behind this one stays 16-byte aligned)
//   kIdentity   Mp rows holding the identity, which the factorisation turns into L^-T (dense_spd_inverse);  then Linv, the flag.
//               `product`: C = A^-1 (Mp x Mp) sits between Aw and Linv, and the flag is the caller's own
// Linv: the inverses of the Mp / 64 diagonal blocks, 64 x 64 each.  Host arithmetic only: every size function and every launcher that
// carves such a workspace takes sizes and offsets from here (tests/test_dense_spd_layout_host.py).
struct DenseSpdWork {
    enum Border { kRhsRows, kIdentity };
    static constexpr int64_t kBlock = 64;  // Cholesky panel width
    int64_t Mp;
    Border border;
    bool product;

    // n: the order of the system before padding
    DenseSpdWork(int64_t n, Border b, bool inverse_product = false) : Mp((n + kBlock - 1) / kBlock * kBlock), border(b), product(inverse_product) {}
    static int64_t doubles(int64_t n, Border b, bool inverse_product = false) { return DenseSpdWork(n, b, inverse_product).doubles(); }

    int64_t rows() const { return Mp + (border == kRhsRows ? kBlock : Mp); }  // of Aw: the grid of spd_system_kernel
    int64_t aw_doubles() const { return rows() * Mp; }
    int64_t linv_doubles() const { return Mp / kBlock * kBlock * kBlock; }
    int64_t w_doubles() const { return border == kRhsRows ? 3 * Mp : 0; }
    int64_t flag_doubles() const { return border == kRhsRows ? 2 : (product ? 0 : 1); }

    int64_t aw() const { return 0; }
    int64_t lt() const { return Mp * Mp; }       // kIdentity: L^-T afterwards (upper triangular, row stride Mp)
    int64_t c() const { return aw_doubles(); }   // kIdentity with product
    int64_t linv() const { return aw_doubles() + (product ? Mp * Mp : 0); }
    int64_t w() const { return linv() + linv_doubles(); }
    int64_t flag() const { return w() + w_doubles(); }
    int64_t doubles() const { return flag() + flag_doubles(); }
};

// Aw ((Mp + 64) x Mp, lower triangle of an SPD matrix + up to three right-hand sides in the border rows Mp .. Mp + 2) -> W (three
// planes of stride Mp): blocked right-looking Cholesky, then the blocked backward substitution.  *flag receives GINGR_ERR_NOT_SPD
// when a diagonal block fails.  W == nullptr: the factor alone (the lower triangle of Aw then holds L).
void dense_spd_solve3(gingr_ctx *ctx, double *Aw, int64_t Mp, double *Linv, double *W, int32_t *flag);
// A^-1 of an SPD matrix: Aw = [lower triangle of A; identity] ((2 Mp) x Mp), C = Mp x Mp; C == nullptr stops after the factorisation,
// which leaves L^-T (A = L L^T) in place of the identity
void dense_spd_inverse(gingr_ctx *ctx, double *Aw, int64_t Mp, double *Linv, double *C, int32_t *flag);

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

// ---- the bordered system of an r x r matrix padded to Mp: one thread per element of Aw, grid (ceil(Mp / 256), DenseSpdWork::rows()).
// Elem(row, c): the entry of the SPD matrix for c <= row < r;  Border(brow, c, r): the entry of border row brow.  Clears *flag.
template <typename Elem, typename Border>
__global__ __launch_bounds__(256) void spd_system_kernel(int r, int64_t Mp, Elem elem, Border border, double *__restrict__ Aw,
                                                         int32_t *__restrict__ flag) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (c == 0 && row == 0) *flag = 0;
    if (c >= Mp) return;
    double v = 0.0;
    if (row >= Mp)
        v = border(row - Mp, c, r);
    else if (c <= row)
        v = (row < r && c < r) ? elem(row, c) : (row == c ? 1.0 : 0.0);
    Aw[row * Mp + c] = v;
}

struct SpdIdentityPlus {  // I + G (row stride n)
    const double *__restrict__ G;
    int n;
    __device__ double operator()(int64_t row, int64_t c) const { return G[row * n + c] + (row == c ? 1.0 : 0.0); }
};
struct SpdRhsRow {  // one right-hand side in border row 0
    const double *__restrict__ rhs;
    __device__ double operator()(int64_t brow, int64_t c, int r) const { return (brow == 0 && c < r) ? rhs[c] : 0.0; }
};
struct SpdIdentityBorder {
    __device__ double operator()(int64_t brow, int64_t c, int) const { return brow == c ? 1.0 : 0.0; }
};

template <typename Elem, typename Border>
inline void launch_spd_system(hipStream_t stream, int r, const DenseSpdWork &ws, Elem elem, Border border, double *Aw, int32_t *flag) {
    hipLaunchKernelGGL((spd_system_kernel<Elem, Border>), dim3((unsigned)((ws.Mp + 255) / 256), (unsigned)ws.rows()), dim3(256), 0, stream, r,
                       ws.Mp, elem, border, Aw, flag);
}
#endif
