// GPMM construction on the device: the low-rank model of
//     GPMMTriangleMesh3D(reference, relativeTolerance).Gaussian / GaussianMixture / AutomaticGaussian
//         (G/api/gpmm/GPMMHelper.scala:96-130)  and  automaticGPMMfromTemplate (G/api/registration/utils/GPMMHelper.scala:39-69)
// i.e.  LowRankGaussianProcess.approximateGPCholesky(reference, GaussianProcess(DiagonalKernel(k, 3)), relativeTolerance,
// NearestNeighborInterpolator)  (GPMM.construct, GPMMHelper.scala:39-55)  with  k = sum_i scaling_i exp(-|x-y|^2/sigma_i^2),
// built straight into a gingr_model: the 3M x r basis never crosses PCIe.
//
// scalismo's algorithm (restated in oracle/gingr_oracle.py: pivoted_cholesky_matrix_valued, approximate_eig): pivoted
// Cholesky over the 3M (point, coordinate) indices, stopped when the residual trace falls below relTol * trace, then the
// eigen-decomposition of L L^T through the SVD of L^T L.  For a DiagonalKernel the three coordinates never interact and
// ties are broken by position, so the generic pivot sequence is (P0,x),(P0,y),(P0,z),(P1,x),... with P0,P1,.. the pivot
// sequence of the SCALAR kernel; after n = 3j + e pivots the coordinates d < e own j+1 scalar columns and the others j,
// and the residual trace is (3-e) tr_s(j) + e tr_s(j+1).  So the device runs the scalar factorisation (M x k_s), finds
// n from the recorded scalar traces (gpmm_plan.h), eigen-decomposes the leading (j+1)x(j+1) and jxj blocks of L_s^T L_s (sym_eig.hip)
// and scatters  Q0 = U sqrt(lambda) = L_s V  into the three coordinate planes of the basis.
//
// The other kernels of GPMMTriangleMesh3D (GPMMHelper.scala:103-142) go through gingr_gpmm_build_diagonal: one scalar kernel per
// coordinate (Gaussian mixture with an optional x-mirrored copy, linear, lookup table).  Three equal kernels take the scalar route
// above; different kernels (GaussianSymmetry) run the generic factorisation over the 3M entries themselves (pc_*_kernel<Diagonal>).
// Exact ties between residuals follow scalismo's rule -- the first maximum in the permuted index order -- through a log of the
// swaps that is replayed for tied candidates (PosLog).
//
// gingr_gpmm_build_radial builds the same way from kernels the reference can only reach through a dense table: per coordinate a sum of
// radial terms (Gaussian, RationalQuadratic, InverseMultiquadric: KernelHelper.scala:53-73), each with an optional weight field over the
// points, sum_t w_t[i] w_t[j] scaling_t f_t(|x_i - x_j|^2) -- a kernel scaled by a function of position, scalismo's ChangePointKernel.
// Only the kernel value differs (radial_value, in pc_*_kernel<RadialScalar / RadialDiagonal>).
//
// Kernels here are one-off (model construction), not the per-iteration path; they are written for exactness of the pivot
// rule (unfused |x-y|^2, multiply-then-add dot products in ascending column order like the JVM) rather than for speed.
#include "gp.h"

#include "fastexp.h"
#include "gpmm_factor.h"
#include "gpmm_kernel_value.h"
#include "gpmm_plan.h"
#include "model_extend.h"

#include <algorithm>
#include <cmath>

namespace {

using gpmm_factor::Factor;
using gpmm_factor::FactorKind;
using gpmm_factor::TaperBasis;
using gpmm_factor::kMaxMix;
using gpmm_factor::KSpec;
using gpmm_factor::KSpec3;
using gpmm_factor::Mixture;

constexpr int kPcBlock = 256;

using gpmm_factor::mixture_value;
using gpmm_factor::radial_family_value;

// the kernel value between reference point c and pivot p (coordinates px, py, pz): gpmm_kernel_value.h, or the lookup table's entry
__device__ __forceinline__ double kspec_value(const KSpec &k, const Cloud &pts, int64_t c, int64_t p, double px, double py,
                                              double pz, const double *T) {
    if (k.kind == 2) return __dmul_rn(k.lookup[c * pts.n + p], k.scale);
    return gpmm_factor::kspec_value_xyz(k, pts.x[c], pts.y[c], pts.z[c], px, py, pz, T);
}

// k(x_c, x_p) = sum_t ((scaling_t f_t(nn)) w_t[c]) w_t[p], terms added left to right, the first assigned; a term without a field has no
// weight factors (a field of ones gives the same bits: x * 1.0 == x).  c == p is the diagonal: nn = 0, the Gaussian's f is exactly 1.
__device__ __forceinline__ double radial_value(const KSpec &k, const Cloud &pts, int64_t c, int64_t p, double px, double py, double pz,
                                               const double *T) {
    double nn = 0.0;
    if (c != p) {
        const double dx = pts.x[c] - px, dy = pts.y[c] - py, dz = pts.z[c] - pz;
        nn = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    }
    const gpmm_factor::RadialFields &rf = *k.radial;
    double v = 0.0;
    for (int i = 0; i < k.mix.n; ++i) {
        const int32_t family = rf.family[i];
        const double f = c == p && family == GINGR_RADIAL_GAUSSIAN ? 1.0 : radial_family_value(family, k.mix.c[i], nn, T);
        double e = __dmul_rn(k.mix.s[i], f);
        const double *w = rf.weight[i];
        if (w) e = __dmul_rn(__dmul_rn(e, w[c]), w[p]);
        v = i == 0 ? e : __dadd_rn(v, e);
    }
    return v;
}

struct Best {
    double v;
    int32_t i;
};

// scalismo's loop takes the FIRST maximal residual in its current PERMUTED index order: step s swaps the pivot into slot s and the
// element that sat there into the pivot's old slot.  With distinct residuals the order is irrelevant, but structured inputs tie
// exactly (a regular grid under a stationary kernel, mirror partners under the mirrored kernel, all entries at step 0), and a rank
// cut inside a group of tied pivots then depends on who went first.  The swaps are kept as a log -- step s: pivot piv[s], displaced
// element dis[s], the pivot's old slot old[s] -- and a tie is resolved by replaying it for the two candidates (O(steps), ties are
// rare).  `vp / vd / vo` is one more entry that is not in memory yet (the step a kernel is executing).
struct PosLog {
    const int32_t *piv, *dis, *old;
    int32_t n;           // entries in memory
    int32_t vp, vd, vo;  // virtual entry (vp < 0: none)
};

// Slot of element e after the logged swaps.  The replay -- "a pivot stays where it was put; a displaced element goes to the pivot's old
// slot" -- only depends on the step that pivoted e (at most one, and e never moves after it) and otherwise on the LAST step that displaced
// it, so the loop carries two selects and no branch: its reads do not depend on one another and run pipelined (as a literal replay with
// an early return every logged step was a dependent round trip, and a mirrored kernel's structural ties replay the log dozens of times
// per step: pc_step_kernel<Diagonal> (then <true>) 131 -> 113 us on average with the log in LDS, -> see profiles/r06_gpmm_build_ab_blocked_kernels.txt).
__device__ __forceinline__ int32_t log_position(const PosLog &lg, int32_t e) {
    int32_t sp = -1, sl = -1;
    for (int32_t s = 0; s < lg.n; ++s) {
        sp = lg.piv[s] == e ? s : sp;
        sl = lg.dis[s] == e ? s : sl;
    }
    if (sp >= 0) return sp;  // pivots stay where they were put (they never compete again)
    int32_t q = sl >= 0 ? lg.old[sl] : e;
    if (lg.vp >= 0) {
        if (lg.vp == e) return lg.n;
        if (lg.vd == e) q = lg.vo;
    }
    return q;
}

// the element in slot `slot` (>= lg.n) after the logged swaps: the one the last swap into that slot put there
__device__ __forceinline__ int32_t log_occupant(const PosLog &lg, int32_t slot) {
    int32_t sl = -1;
    for (int32_t s = 0; s < lg.n; ++s) sl = lg.old[s] == slot ? s : sl;
    return sl >= 0 ? lg.dis[sl] : slot;
}

__device__ __forceinline__ Best better(Best a, Best b, const PosLog &lg) {  // larger value; ties -> earlier slot; NaN never wins
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    if (b.v > a.v) return b;
    if (b.v == a.v && log_position(lg, b.i) < log_position(lg, a.i)) return b;
    return a;
}

// block-wide (max, argmax, sum) with a fixed tree: identical in every workgroup that reduces the same data
__device__ __forceinline__ void block_best_sum(Best &b, double &sum, Best *shb, double *shs, const PosLog &lg) {
    const int t = threadIdx.x;
    shb[t] = b;
    shs[t] = sum;
    __syncthreads();
    for (int off = kPcBlock / 2; off > 0; off >>= 1) {
        if (t < off) {
            shb[t] = better(shb[t], shb[t + off], lg);
            shs[t] += shs[t + off];
        }
        __syncthreads();
    }
    b = shb[0];
    sum = shs[0];
    __syncthreads();
}

// KIND = Scalar: one scalar kernel, entries = points.  KIND = Diagonal: the generic factorisation over the 3M (point, coordinate) entries
// of a DiagonalKernel(k_x, k_y, k_z) whose coordinates have DIFFERENT kernels (entry e = 3 point + coordinate; entries of
// different coordinates never interact: their column values are exact zeros).  KIND = Tapered: the same 3M entries under the full
// block kernel g(x_i, x_j) <Q[3i+a,:], Q[3j+b,:]> of gingr_model_localize (g = specs.k[0], one Gaussian of scaling 1; Q^T = basis.qt):
// every entry interacts with every other.  g(x, x) = 1, so an entry's own value is its row's dot product with itself, summed as the
// step kernel sums it (multiply, then add, ascending columns).  KIND = RadialScalar / RadialDiagonal: Scalar / Diagonal over radial terms
// with weight fields (radial_value); an entry whose weights are all zero has a zero diagonal, never wins a pivot and gets zeros.
template <FactorKind KIND>
__global__ __launch_bounds__(kPcBlock) void pc_init_kernel(Cloud pts, KSpec3 specs, TaperBasis basis, double *__restrict__ diag,
                                                           int32_t *__restrict__ pivoted, double *__restrict__ pmax,
                                                           int32_t *__restrict__ pidx, double *__restrict__ ptr,
                                                           int32_t *__restrict__ ctl) {
    __shared__ double T[GINGR_EXP_TABLE];
    __shared__ Best shb[kPcBlock];
    __shared__ double shs[kPcBlock];
    constexpr bool RAD = KIND == FactorKind::RadialScalar || KIND == FactorKind::RadialDiagonal;
    constexpr bool GEN = KIND != FactorKind::Scalar && KIND != FactorKind::RadialScalar, TAP = KIND == FactorKind::Tapered;
    fastexp_table_init(T);
    __syncthreads();
    const int64_t n = GEN ? 3 * pts.n : pts.n;
    const int64_t c = (int64_t)blockIdx.x * kPcBlock + threadIdx.x;
    Best b{0.0, -1};
    double tr = 0.0;
    if (c < n) {
        const int64_t pc = GEN ? c / 3 : c;
        const KSpec &spec = specs.k[GEN ? (int)(c - 3 * pc) : 0];
        double d0;
        if (RAD) {
            d0 = radial_value(spec, pts, pc, pc, 0.0, 0.0, 0.0, T);  // sum_t scaling_t f_t(0) w_t[c]^2
        } else if (TAP) {
            d0 = 0.0;
            for (int q = 0; q < basis.r; ++q) {
                const double v = basis.qt[(int64_t)q * n + c];
                d0 = __dadd_rn(d0, __dmul_rn(v, v));
            }
        } else if (spec.kind == 0 && spec.mirror == 0.0) {
            d0 = 0.0;
            for (int i = 0; i < spec.mix.n; ++i) d0 = i == 0 ? spec.mix.s[i] : d0 + spec.mix.s[i];  // k(x,x) = sum scaling_i * exp(0)
        } else {
            d0 = kspec_value(spec, pts, pc, pc, pts.x[pc], pts.y[pc], pts.z[pc], T);
        }
        diag[c] = d0;
        pivoted[c] = 0;
        b = Best{d0, (int32_t)c};
        tr = d0;
    }
    const PosLog none{nullptr, nullptr, nullptr, 0, -1, 0, 0};  // nothing swapped yet: ties -> lowest index
    block_best_sum(b, tr, shb, shs, none);
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = b.v;
        pidx[blockIdx.x] = b.i;
        ptr[blockIdx.x] = tr;
        if (blockIdx.x == 0) ctl[0] = ctl[1] = 0;
    }
}

// One pivot step.  Every workgroup first reduces the previous step's block partials (same data, same tree => same pivot
// everywhere, no grid synchronisation), then fills its rows of column k.
// KIND = Tapered: the kernel value is itself a dot product, of the entry's and the pivot's rows of the source basis.  basis.qt holds
// the basis transposed ([r][n], entry order) exactly as L holds the factor ([k][n]): both sums run with the lanes along the entries --
// every load of a wave is one contiguous line -- over a fixed ascending column order, against the pivot's row in LDS (Qp next to Lp).
// A step reads (r + k) n doubles; that traffic is its bound.
template <FactorKind KIND>
__global__ __launch_bounds__(kPcBlock) void pc_step_kernel(Cloud pts, KSpec3 specs, TaperBasis basis, int32_t k, int32_t kmax, double rel_tol,
                                                           int32_t nblocks, double *__restrict__ L /* [kmax][n] */,
                                                           double *__restrict__ diag, int32_t *__restrict__ pivoted,
                                                           const double *__restrict__ pmax_in,
                                                           const int32_t *__restrict__ pidx_in,
                                                           const double *__restrict__ ptr_in, double *__restrict__ pmax,
                                                           int32_t *__restrict__ pidx, double *__restrict__ ptr,
                                                           int32_t *__restrict__ ctl, double *__restrict__ trace,
                                                           int32_t *__restrict__ pivots, int32_t *__restrict__ sw_dis,
                                                           int32_t *__restrict__ sw_old) {
    __shared__ double T[GINGR_EXP_TABLE];
    __shared__ Best shb[kPcBlock];
    __shared__ double shs[kPcBlock];
    __shared__ double Lp[512];
    __shared__ int32_t s_piv[512], s_dis[512], s_old[512];
    __shared__ int32_t finished, sh_dis, sh_old;
    constexpr bool RAD = KIND == FactorKind::RadialScalar || KIND == FactorKind::RadialDiagonal;
    constexpr bool GEN = KIND != FactorKind::Scalar && KIND != FactorKind::RadialScalar, TAP = KIND == FactorKind::Tapered;
    __shared__ double Qp[TAP ? 512 : 1];  // the pivot's row of the basis (a model holds at most 512 columns)
    const int t = threadIdx.x;
    if (t == 0) finished = ctl[1];  // set by an earlier launch (or, harmlessly, by workgroup 0 of this one)
    __syncthreads();
    if (finished) return;
    fastexp_table_init(T);
    // The swaps of steps 0 .. k-1 (written by earlier launches), copied to LDS first: every workgroup replays the log twice per step
    // for this step's swap, and once per candidate for every exact tie (the y and z entries of a point under a mirrored kernel tie
    // structurally).  Read from global memory the replay was one dependent round trip per logged step -- 0.5 us per step of the
    // log for a single-kernel model, 0.8 us for a mirrored one: 365 ms of the 11 A/B builds of tools/experiments/gpmm_build_ab.py,
    // more than everything else of the set-up together.
    for (int r = t; r < k; r += kPcBlock) {
        s_piv[r] = pivots[r];
        s_dis[r] = sw_dis[r];
        s_old[r] = sw_old[r];
    }
    __syncthreads();
    PosLog lg{s_piv, s_dis, s_old, k, -1, 0, 0};
    Best g{0.0, -1};
    double gtr = 0.0;
    for (int b = t; b < nblocks; b += kPcBlock) {
        g = better(g, Best{pmax_in[b], pidx_in[b]}, lg);
        gtr += ptr_in[b];
    }
    block_best_sum(g, gtr, shb, shs, lg);
    const double tol = rel_tol * trace[0];  // trace[0] was written by step 0 (k == 0 uses gtr itself)
    const bool stop = k >= kmax || g.i < 0 || !(gtr >= (k == 0 ? rel_tol * gtr : tol)) || !(g.v > 0.0);
    if (t == 0 && !stop) {  // this step's swap: every workgroup derives it, workgroup 0 records it
        sh_old = log_position(lg, g.i);
        sh_dis = log_occupant(lg, k);
    }
    if (blockIdx.x == 0 && t == 0) {
        trace[k] = gtr;
        if (stop) {
            ctl[0] = k;
            ctl[1] = 1;
        } else {
            pivots[k] = g.i;
            sw_dis[k] = sh_dis;
            sw_old[k] = sh_old;
        }
    }
    if (stop) return;
    const int64_t M = pts.n, n = GEN ? 3 * M : M;
    const int64_t p = g.i;
    const int64_t pp = GEN ? p / 3 : p;
    const int pd = GEN ? (int)(p - 3 * pp) : 0;
    const KSpec &spec = specs.k[pd];
    const double lpk = sqrt(g.v);
    for (int r = t; r < k; r += kPcBlock) Lp[r] = L[(int64_t)r * n + p];
    if (TAP)
        for (int q = t; q < basis.r; q += kPcBlock) Qp[q] = basis.qt[(int64_t)q * n + p];
    __syncthreads();
    lg.vp = (int32_t)p, lg.vd = sh_dis, lg.vo = sh_old;  // the candidates of the NEXT step compete in the order after this swap
    const double px = pts.x[pp], py = pts.y[pp], pz = pts.z[pp];
    const int64_t c = (int64_t)blockIdx.x * kPcBlock + t;
    Best b{0.0, -1};
    double tr = 0.0;
    if (c < n) {
        const int64_t pc = GEN ? c / 3 : c;
        double l;
        if (c == p) {
            l = lpk;
            pivoted[c] = 1;
        } else if (pivoted[c]) {
            l = 0.0;
        } else if ((KIND == FactorKind::Diagonal || KIND == FactorKind::RadialDiagonal) && (int)(c - 3 * pc) != pd) {
            l = 0.0;  // another coordinate: exact zero, the residual is untouched
            b = Best{diag[c], (int32_t)c};
            tr = b.v;
        } else {
            double S = 0.0;
            for (int r = 0; r < k; ++r) S = __dadd_rn(S, __dmul_rn(L[(int64_t)r * n + c], Lp[r]));
            double kv = RAD ? radial_value(spec, pts, pc, pp, px, py, pz, T) : kspec_value(spec, pts, pc, pp, px, py, pz, T);
            if (TAP) {  // the taper times <Q[c,:], Q[p,:]>
                double A = 0.0;
                for (int q = 0; q < basis.r; ++q) A = __dadd_rn(A, __dmul_rn(basis.qt[(int64_t)q * n + c], Qp[q]));
                kv = __dmul_rn(kv, A);
            }
            l = (kv - S) / lpk;
            const double dc = __dadd_rn(diag[c], -__dmul_rn(l, l));
            diag[c] = dc;
            b = Best{dc, (int32_t)c};
            tr = dc;
        }
        L[(int64_t)k * n + c] = l;
    }
    block_best_sum(b, tr, shb, shs, lg);
    if (t == 0) {
        pmax[blockIdx.x] = b.v;
        pidx[blockIdx.x] = b.i;
        ptr[blockIdx.x] = tr;
    }
}

// G[a][b] = sum_c L[a][c] L[b][c]   (blocks on and above the diagonal computed, mirrored); grid (ceil(k / 4), ceil(k / 4)).
// A workgroup forms a 4 x 4 block of entries: per entry the arithmetic of the one-entry-per-workgroup kernel of rounds 1-5 (thread t
// adds the columns t, t + 256, ... by fma in ascending order, then the tree over the threads) -- the same bits -- with eight loads per
// sixteen multiply-adds instead of thirty-two (that kernel read 12 GB through the caches for the 171 columns of a rank-512 model at 50k points).
constexpr int kPcGramTile = 4;
__global__ __launch_bounds__(kPcBlock) void pc_gram_kernel(const double *__restrict__ L, int64_t M, int32_t k,
                                                           double *__restrict__ G) {
    __shared__ double shs[kPcGramTile * kPcGramTile][kPcBlock];
    const int a0 = blockIdx.x * kPcGramTile, b0 = blockIdx.y * kPcGramTile;
    if (a0 > b0) return;
    const double *la[kPcGramTile], *lb[kPcGramTile];
#pragma unroll
    for (int u = 0; u < kPcGramTile; ++u) {  // (columns past k: a clamped, valid column; the entries are not stored)
        la[u] = L + (int64_t)min(a0 + u, k - 1) * M;
        lb[u] = L + (int64_t)min(b0 + u, k - 1) * M;
    }
    double s[kPcGramTile][kPcGramTile];
#pragma unroll
    for (int u = 0; u < kPcGramTile; ++u)
#pragma unroll
        for (int v = 0; v < kPcGramTile; ++v) s[u][v] = 0.0;
    for (int64_t c = threadIdx.x; c < M; c += kPcBlock) {
        double va[kPcGramTile], vb[kPcGramTile];
#pragma unroll
        for (int u = 0; u < kPcGramTile; ++u) va[u] = la[u][c], vb[u] = lb[u][c];
#pragma unroll
        for (int u = 0; u < kPcGramTile; ++u)
#pragma unroll
            for (int v = 0; v < kPcGramTile; ++v) s[u][v] = __builtin_fma(va[u], vb[v], s[u][v]);
    }
#pragma unroll
    for (int u = 0; u < kPcGramTile; ++u)
#pragma unroll
        for (int v = 0; v < kPcGramTile; ++v) shs[u * kPcGramTile + v][threadIdx.x] = s[u][v];
    __syncthreads();
    for (int off = kPcBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int e = 0; e < kPcGramTile * kPcGramTile; ++e) shs[e][threadIdx.x] += shs[e][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x < kPcGramTile * kPcGramTile) {
        const int a = a0 + (int)threadIdx.x / kPcGramTile, b = b0 + (int)threadIdx.x % kPcGramTile;
        if (a < k && b < k && a <= b) {  // (below the diagonal of a diagonal block: the mirrored entry's own sum, the same number)
            G[(int64_t)a * k + b] = shs[threadIdx.x][0];
            G[(int64_t)b * k + a] = shs[threadIdx.x][0];
        }
    }
}

// B[i][c] = sum_r L[r][c] V[r][i]   (c over ALL points, i < n): column i of  U sqrt(lambda) = L V
// Only the leading `nout` columns are formed (a truncated model keeps the leading eigenvectors of a block); an entry's fma sequence
// does not depend on nout.
constexpr int kLvCols = 8;  // columns of B per thread: L is read nout / 8 times instead of nout times (the same fma sequence per entry)
__global__ __launch_bounds__(256) void lv_kernel(const double *__restrict__ L, int64_t M, int32_t n, int32_t nout,
                                                 const double *__restrict__ V, double *__restrict__ B) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * kLvCols;
    if (c >= M) return;
    int col[kLvCols];  // workgroup-uniform; columns past nout repeat the last one and are not stored
#pragma unroll
    for (int u = 0; u < kLvCols; ++u) col[u] = min(i0 + u, nout - 1);
    double acc[kLvCols];
#pragma unroll
    for (int u = 0; u < kLvCols; ++u) acc[u] = 0.0;
    for (int r = 0; r < n; ++r) {
        const double l = L[(int64_t)r * M + c];
        const double *v = V + (int64_t)r * n;
#pragma unroll
        for (int u = 0; u < kLvCols; ++u) acc[u] = __builtin_fma(l, v[col[u]], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < kLvCols; ++u)
        if (i0 + u < nout) B[(int64_t)(i0 + u) * M + c] = acc[u];
}

// Q0[(3s+d)*rp + q] = B_set(q)[idx(q)][row_begin + perm[s]] when coordinate(q) == d, else 0
__global__ __launch_bounds__(256) void gpmm_pack_kernel(const double *__restrict__ BA, const double *__restrict__ BB,
                                                        const double *__restrict__ BC, int64_t M_total, int64_t row_begin, int64_t M, int32_t r, int32_t rp,
                                                        const int32_t *__restrict__ perm, const int32_t *__restrict__ qdim,
                                                        const int32_t *__restrict__ qset, const int32_t *__restrict__ qidx,
                                                        double *__restrict__ Q0) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * M * rp) return;
    const int64_t row = idx / rp;
    const int32_t q = (int32_t)(idx - row * rp);
    const int64_t s = row / 3;
    const int d = (int)(row - 3 * s);
    double v = 0.0;
    if (q < r && qdim[q] == d) {
        const int64_t c = row_begin + (perm ? perm[s] : s);
        v = (qset[q] == 0 ? BA : (qset[q] == 1 ? BB : BC))[(int64_t)qidx[q] * M_total + c];
    }
    Q0[idx] = v;
}

// Q0[(3s+d)*rp + q] = B[q][3 (row_begin + perm[s]) + d]: the generic factor's columns are already (point, coordinate) interleaved
__global__ __launch_bounds__(256) void gpmm_pack_generic_kernel(const double *__restrict__ B, int64_t M_total, int64_t row_begin,
                                                                int64_t M, int32_t r, int32_t rp, const int32_t *__restrict__ perm,
                                                                double *__restrict__ Q0) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * M * rp) return;
    const int64_t row = idx / rp;
    const int32_t q = (int32_t)(idx - row * rp);
    const int64_t s = row / 3;
    const int d = (int)(row - 3 * s);
    Q0[idx] = q < r ? B[(int64_t)q * 3 * M_total + 3 * (row_begin + (perm ? perm[s] : s)) + d] : 0.0;
}

}  // namespace

// The pivoted Cholesky factorisation (gpmm_factor.h) over the kernels above
namespace gpmm_factor {

int Factor::init(gingr_ctx *c, const KSpec3 &k, const Cloud &p, bool gen, int32_t cap, bool radial) {
    if (radial) return init_kind(c, k, p, gen ? FactorKind::RadialDiagonal : FactorKind::RadialScalar, cap);
    return init_kind(c, k, p, gen ? FactorKind::Diagonal : FactorKind::Scalar, cap);
}

int Factor::init_tapered(gingr_ctx *c, const KSpec3 &taper, const Cloud &p, const TaperBasis &qb, int32_t cap, int timer_hook) {
    basis = qb, timer = timer_hook;
    return init_kind(c, taper, p, FactorKind::Tapered, cap);
}

int Factor::init_kind(gingr_ctx *c, const KSpec3 &k, const Cloud &p, FactorKind kind, int32_t cap) {
    const bool gen = kind != FactorKind::Scalar && kind != FactorKind::RadialScalar;
    ctx = c, specs = k, pts = p, n = gen ? 3 * p.n : p.n, kcap = cap;
    step_kernel = kind == FactorKind::Tapered          ? pc_step_kernel<FactorKind::Tapered>
                  : kind == FactorKind::Diagonal       ? pc_step_kernel<FactorKind::Diagonal>
                  : kind == FactorKind::RadialScalar   ? pc_step_kernel<FactorKind::RadialScalar>
                  : kind == FactorKind::RadialDiagonal ? pc_step_kernel<FactorKind::RadialDiagonal>
                                                       : pc_step_kernel<FactorKind::Scalar>;
    nb = (int)ceil_div(n, kPcBlock);
    HIP_TRY(ctx, Lb.alloc((size_t)kcap * n * sizeof(double)));
    HIP_TRY(ctx, diag.alloc((size_t)n * sizeof(double)));
    HIP_TRY(ctx, piv.alloc((size_t)n * sizeof(int32_t)));
    HIP_TRY(ctx, part.alloc((size_t)2 * nb * (2 * sizeof(double) + sizeof(int32_t)) + 64));
    HIP_TRY(ctx, ctl.alloc(2 * sizeof(int32_t)));
    HIP_TRY(ctx, trace.alloc((size_t)(kcap + 1) * sizeof(double)));
    HIP_TRY(ctx, pivots.alloc((size_t)(kcap + 1) * sizeof(int32_t)));
    HIP_TRY(ctx, swd.alloc((size_t)(kcap + 1) * sizeof(int32_t)));
    HIP_TRY(ctx, swo.alloc((size_t)(kcap + 1) * sizeof(int32_t)));
    pmaxv[0] = part.as<double>(), pmaxv[1] = part.as<double>() + nb;
    ptrv[0] = part.as<double>() + 2 * nb, ptrv[1] = part.as<double>() + 3 * nb;
    pidxv[0] = reinterpret_cast<int32_t *>(part.as<double>() + 4 * nb), pidxv[1] = pidxv[0] + nb;
    hipLaunchKernelGGL(kind == FactorKind::Tapered          ? pc_init_kernel<FactorKind::Tapered>
                       : kind == FactorKind::Diagonal       ? pc_init_kernel<FactorKind::Diagonal>
                       : kind == FactorKind::RadialScalar   ? pc_init_kernel<FactorKind::RadialScalar>
                       : kind == FactorKind::RadialDiagonal ? pc_init_kernel<FactorKind::RadialDiagonal>
                                                            : pc_init_kernel<FactorKind::Scalar>,
                       dim3(nb), dim3(kPcBlock), 0, ctx->stream, pts, specs, basis, diag.as<double>(), piv.as<int32_t>(), pmaxv[0], pidxv[0],
                       ptrv[0], ctl.as<int32_t>());
    return check_launch(ctx);
}

void Factor::launch(int32_t k, double rel_tol) {
    const int in = k & 1, o = in ^ 1;
    auto step = [&] {
        hipLaunchKernelGGL(step_kernel, dim3(nb), dim3(kPcBlock), 0, ctx->stream, pts, specs, basis, k, kcap, rel_tol, nb, Lb.as<double>(),
                           diag.as<double>(), piv.as<int32_t>(), pmaxv[in], pidxv[in], ptrv[in], pmaxv[o], pidxv[o], ptrv[o],
                           ctl.as<int32_t>(), trace.as<double>(), pivots.as<int32_t>(), swd.as<int32_t>(), swo.as<int32_t>());
    };
    if (timer < 0) return step();
    TimerScope ts(ctx, timer);
    step();
}

int Factor::run_to_tolerance(double rel_tol) {
    int32_t hctl[2] = {0, 0};
    for (int32_t k = 0; k <= kcap; ++k) {
        launch(k, rel_tol);
        if ((k & 15) == 15 || k == kcap) {  // look at the stop flag now and then instead of queueing no-op launches
            GINGR_TRY(check_launch(ctx));
            HIP_TRY(ctx, hipMemcpyAsync(hctl, ctl.p, sizeof(hctl), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (hctl[1]) break;
        }
    }
    if (!hctl[1]) return gingr_set_error(ctx, GINGR_ERR_STATE, "gpmm_build: pivoted Cholesky did not terminate");
    ks = hctl[0];
    htrace.resize((size_t)ks + 1);
    HIP_TRY(ctx, hipMemcpyAsync(htrace.data(), trace.p, htrace.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

// G = L^T L of the n columns, its eigenpairs, the caller's choice of the leading `keep`, U sqrt(lambda) = L V for those, the model
int generic_tail(gingr_ctx *ctx, Factor &fg, int64_t M, const double *ref, const double *mean, int64_t row_begin, int64_t row_end,
                 std::vector<double> &hev, const std::function<int(std::vector<double> &, int32_t *)> &choose, gingr_model **out,
                 const std::function<int(const double *, int32_t)> &keep_extension) {
    const int32_t n = fg.ks;
    DevBuf G, ev, V, B;
    HIP_TRY(ctx, G.alloc((size_t)n * n * sizeof(double)));
    HIP_TRY(ctx, ev.alloc((size_t)(n + 1) * sizeof(double)));
    HIP_TRY(ctx, V.alloc((size_t)(n * n + 1) * sizeof(double)));
    HIP_TRY(ctx, B.alloc((size_t)n * 3 * M * sizeof(double)));
    hipLaunchKernelGGL(pc_gram_kernel, dim3((unsigned)ceil_div(n, kPcGramTile), (unsigned)ceil_div(n, kPcGramTile)), dim3(kPcBlock), 0, ctx->stream, fg.Lb.as<double>(), 3 * M, n, G.as<double>());
    GINGR_TRY(launch_jacobi_eig(ctx, G.as<double>(), n, n, ev.as<double>(), V.as<double>()));
    hev.assign((size_t)n, 0.0);
    HIP_TRY(ctx, hipMemcpyAsync(hev.data(), ev.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int32_t keep = n;
    GINGR_TRY(choose(hev, &keep));
    hipLaunchKernelGGL(lv_kernel, dim3((unsigned)ceil_div(3 * M, 256), (unsigned)ceil_div(keep, kLvCols)), dim3(256), 0, ctx->stream, fg.Lb.as<double>(), 3 * M, n,
                       keep, V.as<double>(), B.as<double>());
    GINGR_TRY(check_launch(ctx));
    auto fill = [&](gingr_model *m) -> int {
        const int64_t total = 3 * m->M * m->rp;
        hipLaunchKernelGGL(gpmm_pack_generic_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, B.as<double>(),
                           M, m->row_begin, m->M, m->r, m->rp, m->perm, m->Q0);
        return check_launch(ctx);
    };
    if (keep_extension) GINGR_TRY(keep_extension(V.as<double>(), keep));
    return model_create_impl(ctx, M, keep, ref, mean, hev.data(), row_begin, row_end, fill, out);
}

}  // namespace gpmm_factor

namespace {

bool same_kernel(const gingr_scalar_kernel *a, const gingr_scalar_kernel *b) {
    if (a == b) return true;
    if (a->kind != b->kind) return false;
    if (a->kind == GINGR_KERNEL_GAUSSIAN_MIXTURE) {
        if (a->n_kernels != b->n_kernels || a->mirror != b->mirror) return false;
        for (int i = 0; i < a->n_kernels; ++i)
            if (a->sigmas[i] != b->sigmas[i] || a->scalings[i] != b->scalings[i]) return false;
        return true;
    }
    return a->scaling == b->scaling && a->lookup == b->lookup;
}

// The device form of one scalar kernel of the caller's, validated; the matrix of a lookup kernel (M x M) goes to the device in `lookup`.
int make_kspec(gingr_ctx *ctx, const gingr_scalar_kernel *k, int64_t M, DevBuf &lookup, KSpec &sp) {
    memset(&sp, 0, sizeof(sp));
    sp.kind = k->kind;
    if (k->kind == GINGR_KERNEL_GAUSSIAN_MIXTURE) {
        if (k->n_kernels < 1 || k->n_kernels > kMaxMix || !k->sigmas || !k->scalings)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: need M >= 1 and 1..%d kernels", kMaxMix);
        if (!(k->mirror == 0.0 || k->mirror == 1.0 || k->mirror == -1.0))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: mirror must be 0, +1 or -1");
        sp.mix.n = k->n_kernels;
        sp.mirror = k->mirror;
        for (int i = 0; i < k->n_kernels; ++i) {
            if (!(k->sigmas[i] > 0.0) || !(k->scalings[i] > 0.0) || !std::isfinite(k->sigmas[i]) || !std::isfinite(k->scalings[i]))
                return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: sigma and scaling must be positive");
            sp.mix.c[i] = -(double)GINGR_EXP_TABLE * 1.4426950408889634074 / (k->sigmas[i] * k->sigmas[i]);
            sp.mix.s[i] = k->scalings[i];
        }
    } else if (k->kind == GINGR_KERNEL_DOT || k->kind == GINGR_KERNEL_LOOKUP) {
        if (!(k->scaling > 0.0) || !std::isfinite(k->scaling))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: scaling must be positive");
        sp.scale = k->scaling;
        if (k->kind == GINGR_KERNEL_LOOKUP) {
            if (!k->lookup) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: lookup kernel without a matrix");
            HIP_TRY(ctx, lookup.alloc((size_t)M * M * sizeof(double)));
            HIP_TRY(ctx, hipMemcpyAsync(lookup.p, k->lookup, (size_t)M * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            sp.lookup = lookup.as<double>();
        }
    } else {
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: unknown kernel kind %d", (int)k->kind);
    }
    return GINGR_OK;
}

// What an entry asks for, validated, with the reference and the kernels on the device
struct Build {
    gingr_ctx *ctx;
    int64_t M;  // points of the whole model
    const double *ref;
    double rel_tol;
    bool ex, to_tolerance;
    int32_t max_rank, keep_rank;  // factor columns at most; columns of the model (ex)
    int64_t row_begin, row_end;
    gingr_gpmm_info *info;
    gingr_model **out;
    Cloud pts;
    KSpec3 specs;
    bool radial;  // the kernels are sums of radial terms, with or without weight fields (gingr_gpmm_build_radial)
    int32_t family[3][kMaxMix];  // radial: the families of every coordinate's terms (host copy of RadialFields::family)
    bool weighted;               // radial: some term carries a weight field
};

// the caller's gingr_gpmm_info from the plan's values, and the entry's answer to a refusal
int report(const Build &b, gpmm_plan::Refusal refusal, const gpmm_plan::Info &pi) {
    if (b.info) *b.info = gingr_gpmm_info{pi.columns, pi.rank, pi.tolerance_reached, pi.residual_fraction, pi.kept_variance_fraction};
    if (refusal == gpmm_plan::Refusal::CeilingBeforeTolerance)
        return gingr_set_error(b.ctx, GINGR_ERR_BAD_ARGUMENT,
                               "gpmm_build: the ceiling of %d factor columns (GINGR_GPMM_MAX_COLUMNS) was reached at a residual fraction of %.6g, "
                               "above the relative tolerance %.6g",
                               GINGR_GPMM_MAX_COLUMNS, pi.residual_fraction, b.rel_tol);
    if (refusal == gpmm_plan::Refusal::AboveRankLimit)
        return gingr_set_error(b.ctx, GINGR_ERR_BAD_ARGUMENT,
                               "gpmm_build: the factorisation has %d columns (columns = %d), a model holds at most 512: pass keep_rank <= 512",
                               (int)pi.columns, (int)pi.columns);
    return GINGR_OK;
}

// the zero-mean model of `rank` columns whose basis `fill` writes
int create_model(const Build &b, int32_t rank, const double *variance, const std::function<int(gingr_model *)> &fill) {
    const std::vector<double> zero_mean((size_t)3 * b.M, 0.0);
    return model_create_impl(b.ctx, b.M, rank, b.ref, zero_mean.data(), variance, b.row_begin, b.row_end, fill, b.out);
}

// Why a model of this build carries no kernel extension (model_extend.h); null: it carries one
const char *extension_fault(const Build &b) {
    if (b.row_begin != 0 || b.row_end != b.M) return "it is a row shard";
    for (const KSpec &k : b.specs.k)
        if (k.kind == GINGR_KERNEL_LOOKUP)
            return "its kernel is a lookup table over the reference points (InverseLaplacian), which has no value off the reference";
    if (b.radial && b.weighted)
        return "its radial terms carry weight fields (ScaledGaussian, ChangePoint), and a field is not defined off the reference";
    return nullptr;
}

// the extension of a model of `rank` columns with the build's kernels by value; the caller adds the pivots and what forms C
std::shared_ptr<KernelExtension> new_extension(const Build &b, bool shared, int32_t rank) {
    auto x = std::make_shared<KernelExtension>();
    x->shared = shared, x->r = rank, x->rp = (int32_t)round_up(rank, 16);
    for (int d = 0; d < 3; ++d) {
        x->kernel[d].spec = b.specs.k[d];
        x->kernel[d].spec.lookup = nullptr;  // (the build's device table of families dies with the build: family[] replaces it)
        memcpy(x->kernel[d].family, b.family[d], sizeof(b.family[d]));
    }
    return x;
}

// Coordinates with different kernels: scalismo's generic factorisation itself, over the 3M (point, coordinate) entries -- argmax of the
// residual diagonal in the permuted entry order, stop at relTol * trace -- then the eigen-decomposition of L^T L and
// U sqrt(lambda) = L V, exactly as for any matrix-valued kernel.
int build_generic(const Build &b) {
    gingr_ctx *ctx = b.ctx;
    const int64_t M = b.M;
    Factor fg;
    const int32_t gcap = (int32_t)std::min<int64_t>(std::min<int64_t>(3 * M, b.max_rank), 512);  // (the pivot step's swap log: 512 entries)
    GINGR_TRY(fg.init(ctx, b.specs, b.pts, true, gcap, b.radial));
    GINGR_TRY(fg.run_to_tolerance(b.rel_tol));
    const int32_t n = fg.ks;
    if (n < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: empty model (tolerance too large)");
    const double fraction = fg.htrace[(size_t)n] / fg.htrace[0];
    const bool reached = gpmm_plan::below_tolerance(fg.htrace[(size_t)n], fg.htrace[0], b.rel_tol) || (int64_t)n == 3 * M;
    gpmm_plan::Info pi;
    if (b.ex && !reached && n == gcap && gcap < b.max_rank) {
        (void)report(b, gpmm_plan::Refusal::None, gpmm_plan::Info{n, 0, 0, fraction, 1.0});
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT,
                               "gpmm_build: coordinate-wise different kernels: at most 512 factor columns (residual fraction %.6g after 512)", fraction);
    }
    if (gpmm_plan::unfinished(b.to_tolerance, n, reached, fraction, pi) != gpmm_plan::Refusal::None)
        return report(b, gpmm_plan::Refusal::CeilingBeforeTolerance, pi);
    std::vector<double> hev;
    const std::vector<double> zero_mean((size_t)3 * M, 0.0);
    auto choose = [&](std::vector<double> &lam, int32_t *keep) -> int {
        for (auto &v : lam) v = v > 0.0 ? v : 0.0;
        return report(b, gpmm_plan::conclude(b.ex, b.keep_rank, n, reached, fraction, lam, *keep, pi), pi);
    };
    // what the kernel extension needs, while the factor is alive: a pivot is a (point, coordinate) entry of its own coordinate's list
    const char *fault = extension_fault(b);
    std::shared_ptr<KernelExtension> x;
    auto keep_extension = [&](const double *V, int32_t keep) -> int {
        if (fault) return GINGR_OK;
        x = new_extension(b, false, keep);
        const double *const Vs[3] = {V, nullptr, nullptr};
        const int32_t vn[3] = {n, 0, 0};
        return kernel_extension_keep(ctx, fg, n, true, Vs, vn, *x);
    };
    GINGR_TRY(gpmm_factor::generic_tail(ctx, fg, M, b.ref, zero_mean.data(), b.row_begin, b.row_end, hev, choose, b.out, keep_extension));
    (*b.out)->ext = x;
    if (fault) (*b.out)->ext_missing = fault;
    return GINGR_OK;
}

// One kernel for all coordinates: the scalar factorisation (M x k_s), the generic column count from its traces (gpmm_plan.h:
// count_columns), the eigen-decompositions of the leading blocks of L_s^T L_s -- one per distinct column count among the coordinates,
// side by side -- and Q0 = L_s V scattered into the three coordinate planes in the order of the merged spectrum.
int build_scalar(const Build &b) {
    gingr_ctx *ctx = b.ctx;
    const int64_t M = b.M;
    Factor fac;
    const int32_t kmax = (int32_t)std::min<int64_t>(M, (b.max_rank + 2) / 3);  // scalar columns that can ever be needed
    GINGR_TRY(fac.init(ctx, b.specs, b.pts, false, kmax, b.radial));
    GINGR_TRY(fac.run_to_tolerance(b.rel_tol));
    if (fac.ks < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: empty model (tolerance too large)");
    const gpmm_plan::Columns c = gpmm_plan::count_columns(fac.htrace.data(), fac.ks, b.max_rank, b.rel_tol, M);
    gpmm_plan::Info pi;
    if (gpmm_plan::unfinished(b.to_tolerance, c.n, c.reached, c.fraction, pi) != gpmm_plan::Refusal::None)
        return report(b, gpmm_plan::Refusal::CeilingBeforeTolerance, pi);
    if (c.n < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: empty model (tolerance too large)");

    // the Gram matrix of the scalar columns in use; a block is its leading block_n[b] x block_n[b] part
    int block_of[3];
    int32_t block_n[3];
    const int nblocks = gpmm_plan::group_blocks(c.cnt, block_of, block_n);
    const int32_t kkmax = *std::max_element(block_n, block_n + 3);
    DevBuf G, ev[3], V[3], B[3];
    HIP_TRY(ctx, G.alloc((size_t)kkmax * kkmax * sizeof(double)));
    hipLaunchKernelGGL(pc_gram_kernel, dim3((unsigned)ceil_div(kkmax, kPcGramTile), (unsigned)ceil_div(kkmax, kPcGramTile)), dim3(kPcBlock), 0, ctx->stream, fac.Lb.as<double>(), M, kkmax,
                       G.as<double>());
    std::vector<double> hev[3];
    {
        const double *Gs[3];
        double *es[3], *vs[3];
        int32_t lds[3];
        for (int q = 0; q < nblocks; ++q) {
            const int32_t nq = block_n[q];
            HIP_TRY(ctx, ev[q].alloc((size_t)(nq + 1) * sizeof(double)));
            HIP_TRY(ctx, V[q].alloc((size_t)(nq * nq + 1) * sizeof(double)));
            HIP_TRY(ctx, B[q].alloc(((size_t)nq * M + 1) * sizeof(double)));
            Gs[q] = G.as<double>(), lds[q] = kkmax, es[q] = ev[q].as<double>(), vs[q] = V[q].as<double>();
            hev[q].resize((size_t)nq);
        }
        GINGR_TRY(sym_eig(ctx, nblocks, Gs, lds, block_n, es, vs, b.ex));  // the blocks side by side
    }
    for (int q = 0; q < nblocks; ++q)
        HIP_TRY(ctx, hipMemcpyAsync(hev[q].data(), ev[q].p, hev[q].size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    const gpmm_plan::Merged m = gpmm_plan::merge_spectra(hev, c.cnt, block_of);
    int32_t rank = c.n;
    const gpmm_plan::Refusal refusal = gpmm_plan::conclude(b.ex, b.keep_rank, c.n, c.reached, c.fraction, m.variance, rank, pi);
    GINGR_TRY(report(b, refusal, pi));
    // U sqrt(lambda) = L V for the eigenvectors the model keeps: the leading ones of every block
    int32_t need[3];
    gpmm_plan::eigvecs_needed(m, rank, need);
    for (int q = 0; q < nblocks; ++q)
        if (need[q] > 0)
            hipLaunchKernelGGL(lv_kernel, dim3((unsigned)ceil_div(M, 256), (unsigned)ceil_div(need[q], kLvCols)), dim3(256), 0, ctx->stream,
                               fac.Lb.as<double>(), M, block_n[q], need[q], V[q].as<double>(), B[q].as<double>());
    GINGR_TRY(check_launch(ctx));
    std::vector<int32_t> qmap;  // [3][rank]: coordinate, block, index of the kept columns
    for (const std::vector<int32_t> *v : {&m.qdim, &m.qblock, &m.qidx}) qmap.insert(qmap.end(), v->begin(), v->begin() + rank);
    DevBuf dq;
    HIP_TRY(ctx, dq.alloc(qmap.size() * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpy(dq.p, qmap.data(), qmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));

    auto fill = [&](gingr_model *mdl) -> int {
        const int64_t total = 3 * mdl->M * mdl->rp;
        hipLaunchKernelGGL(gpmm_pack_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, B[0].as<double>(),
                           B[1].as<double>(), B[2].as<double>(), M, mdl->row_begin, mdl->M, mdl->r, mdl->rp, mdl->perm, dq.as<int32_t>(),
                           dq.as<int32_t>() + rank, dq.as<int32_t>() + 2 * rank, mdl->Q0);
        return check_launch(ctx);
    };
    // what the kernel extension needs, while the factor is alive and ahead of the synchronisations of the model's construction: the
    // three pivot lists are prefixes of the scalar pivot sequence
    const char *fault = extension_fault(b);
    std::shared_ptr<KernelExtension> x;
    if (!fault) {
        x = new_extension(b, true, rank);
        for (int d = 0; d < 3; ++d) x->cnt[d] = c.cnt[d], x->block_of[d] = block_of[d];
        x->qdim.assign(m.qdim.begin(), m.qdim.begin() + rank);
        x->qidx.assign(m.qidx.begin(), m.qidx.begin() + rank);
        const double *const Vs[3] = {V[0].as<double>(), V[1].as<double>(), V[2].as<double>()};
        GINGR_TRY(kernel_extension_keep(ctx, fac, kkmax, false, Vs, block_n, *x));
    }
    GINGR_TRY(create_model(b, rank, m.variance.data(), fill));
    (*b.out)->ext = x;
    if (fault) (*b.out)->ext_missing = fault;
    return GINGR_OK;
}

}  // namespace

// What every entry checks before it looks at its kernels, and the Build that follows from it.
// `ex` false (gingr_gpmm_build_diagonal): max_columns is its max_rank, silently clamped to the model's rank limit, no truncation.
// `ex` true (gingr_gpmm_build_diagonal_ex, gingr_gpmm_build_radial): max_columns <= 0 runs to the tolerance under the library's
// ceiling, nothing is ever shortened silently, keep_rank leading eigenpairs of the merged spectrum are kept.
static int start_build(gingr_ctx *ctx, int64_t M, const double *ref, bool kernels, double relative_tolerance, bool ex, int32_t max_columns,
                       int32_t keep_rank, int64_t row_begin, int64_t row_end, gingr_gpmm_info *info, gingr_model **out, Build &b) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    if (ex && max_columns > GINGR_GPMM_MAX_COLUMNS)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: max_columns = %d is above the ceiling of %d factor columns",
                               (int)max_columns, GINGR_GPMM_MAX_COLUMNS);
    const bool to_tolerance = ex && max_columns <= 0;
    if (M < 1 || !ref || !kernels) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: need M >= 1, a reference and three kernels");
    if (!(relative_tolerance >= 0.0) || !(relative_tolerance < 1.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: relative tolerance must be in [0, 1)");
    int32_t max_rank = max_columns;  // factor columns at most
    if (ex) {
        if (to_tolerance) max_rank = GINGR_GPMM_MAX_COLUMNS;
    } else if (max_rank <= 0 || max_rank > 512) {
        max_rank = 512;  // the model's rank limit (gingr_model_upload)
    }
    if ((int64_t)max_rank > 3 * M) max_rank = (int32_t)(3 * M);
    b = Build{ctx, M, ref, relative_tolerance, ex, to_tolerance, max_rank, keep_rank, row_begin, row_end <= 0 ? M : row_end, info, out, Cloud{}, KSpec3{}, false};
    return GINGR_OK;
}

// the reference to the device, then the route: one scalar factorisation, or the generic one when the coordinates' kernels differ
static int run_build(Build &b, bool generic) {
    gingr_ctx *ctx = b.ctx;
    const int64_t M = b.M;
    DevBuf aos, soa;
    HIP_TRY(ctx, aos.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, soa.alloc((size_t)3 * M * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(aos.p, b.ref, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos.as<double>(), M, soa.as<double>());
    const double *s = soa.as<double>();
    b.pts = Cloud{s, s + M, s + 2 * M, M};
    return generic ? build_generic(b) : build_scalar(b);
}

static int gpmm_build_impl(gingr_ctx *ctx, int64_t M, const double *ref, const gingr_scalar_kernel *kx, const gingr_scalar_kernel *ky,
                           const gingr_scalar_kernel *kz, double relative_tolerance, bool ex, int32_t max_columns, int32_t keep_rank,
                           int64_t row_begin, int64_t row_end, gingr_gpmm_info *info, gingr_model **out) {
    Build b;
    GINGR_TRY(start_build(ctx, M, ref, kx && ky && kz, relative_tolerance, ex, max_columns, keep_rank, row_begin, row_end, info, out, b));

    // the kernels, one device form per distinct one
    const gingr_scalar_kernel *kd[3] = {kx, ky, kz};
    int set_of[3], first[3];
    const int nsets = gpmm_plan::group3([&](int e, int d) { return same_kernel(kd[e], kd[d]); }, gpmm_plan::none, set_of, first);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf lookups[3];
    KSpec specs[3];
    for (int q = 0; q < nsets; ++q) GINGR_TRY(make_kspec(ctx, kd[first[q]], M, lookups[q], specs[q]));
    for (int d = 0; d < 3; ++d) b.specs.k[d] = specs[set_of[d]];
    return run_build(b, nsets > 1);
}

// ---- gingr_gpmm_build_radial: radial terms with weight fields
namespace {

bool same_field(const double *a, const double *b, int64_t M) {
    return a == b || (a && b && memcmp(a, b, (size_t)M * sizeof(double)) == 0);  // by pointer, then by content
}

bool same_radial(const gingr_radial_kernel *a, const gingr_radial_kernel *b, int64_t M) {
    if (a == b) return true;
    if (a->n_terms != b->n_terms) return false;
    for (int t = 0; t < a->n_terms; ++t) {
        const gingr_radial_term &x = a->terms[t], &y = b->terms[t];
        if (x.family != y.family || x.parameter != y.parameter || x.scaling != y.scaling || !same_field(x.weight, y.weight, M)) return false;
    }
    return true;
}

// one kernel of the caller's, checked: every refusal names the coordinate's kernel and the term
int check_radial(gingr_ctx *ctx, const gingr_radial_kernel *k, char coord, int64_t M) {
    if (k->n_terms < 1 || k->n_terms > kMaxMix || !k->terms)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build_radial: kernel %c: n_terms = %d, need 1..%d terms", coord, (int)k->n_terms,
                               kMaxMix);
    for (int t = 0; t < k->n_terms; ++t) {
        const gingr_radial_term &term = k->terms[t];
        if (term.family != GINGR_RADIAL_GAUSSIAN && term.family != GINGR_RADIAL_RATIONAL_QUADRATIC &&
            term.family != GINGR_RADIAL_INVERSE_MULTIQUADRIC)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build_radial: kernel %c term %d: unknown family %d", coord, t, (int)term.family);
        if (!(term.parameter > 0.0) || !std::isfinite(term.parameter))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build_radial: kernel %c term %d: the parameter must be finite and positive", coord, t);
        if (!(term.scaling > 0.0) || !std::isfinite(term.scaling))
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build_radial: kernel %c term %d: the scaling must be finite and positive", coord, t);
        if (term.weight)
            for (int64_t i = 0; i < M; ++i)
                if (!std::isfinite(term.weight[i]))
                    return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build_radial: kernel %c term %d: weight %lld is not finite", coord, t,
                                           (long long)i);
    }
    // k(x_i, x_i) = sum_t scaling_t f_t(0) w_t[i]^2 as the device sums it: positive somewhere, or there is nothing to factor
    for (int64_t i = 0; i < M; ++i) {
        double d = 0.0;
        for (int t = 0; t < k->n_terms; ++t) {
            const gingr_radial_term &term = k->terms[t];
            const double f0 = term.family == GINGR_RADIAL_INVERSE_MULTIQUADRIC ? 1.0 / std::sqrt(term.parameter * term.parameter) : 1.0;
            double e = term.scaling * f0;
            if (term.weight) e = e * term.weight[i] * term.weight[i];
            d = t == 0 ? e : d + e;
        }
        if (d > 0.0) return GINGR_OK;
    }
    return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT,
                           "gpmm_build_radial: kernel %c: the diagonal is zero at every point (the weights of terms 0..%d vanish everywhere)", coord,
                           (int)k->n_terms - 1);
}

}  // namespace

extern "C" {

int gingr_gpmm_build_diagonal(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_scalar_kernel *kx,
                              const gingr_scalar_kernel *ky, const gingr_scalar_kernel *kz, double relative_tolerance,
                              int32_t max_rank, int64_t row_begin, int64_t row_end, gingr_model **out) {
    return gpmm_build_impl(ctx, M_total, ref, kx, ky, kz, relative_tolerance, false, max_rank, 0, row_begin, row_end, nullptr, out);
}

int gingr_gpmm_build_diagonal_ex(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_scalar_kernel *kx,
                                 const gingr_scalar_kernel *ky, const gingr_scalar_kernel *kz, double relative_tolerance,
                                 int32_t max_columns, int32_t keep_rank, int64_t row_begin, int64_t row_end, gingr_gpmm_info *info,
                                 gingr_model **out) {
    return gpmm_build_impl(ctx, M_total, ref, kx, ky, kz, relative_tolerance, true, max_columns, keep_rank, row_begin, row_end, info, out);
}

int gingr_gpmm_build_radial(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_radial_kernel *kx,
                            const gingr_radial_kernel *ky, const gingr_radial_kernel *kz, double relative_tolerance, int32_t max_columns,
                            int32_t keep_rank, int64_t row_begin, int64_t row_end, gingr_gpmm_info *info, gingr_model **out) {
    Build b;
    GINGR_TRY(start_build(ctx, M_total, ref, kx && ky && kz, relative_tolerance, true, max_columns, keep_rank, row_begin, row_end, info, out, b));
    b.radial = true;
    const int64_t M = M_total;
    const gingr_radial_kernel *kd[3] = {kx, ky, kz};
    int set_of[3], first[3];
    for (int d = 0; d < 3; ++d)  // (checked before they are compared: the comparison reads the terms)
        if (d == 0 || (kd[d] != kd[0] && kd[d] != kd[d - 1])) GINGR_TRY(check_radial(ctx, kd[d], "xyz"[d], M));
    const int nsets = gpmm_plan::group3([&](int e, int d) { return same_radial(kd[e], kd[d], M); }, gpmm_plan::none, set_of, first);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the device form of every distinct kernel; every distinct field (by pointer) is uploaded once
    const double *host_field[3 * kMaxMix];
    DevBuf dev_field[3 * kMaxMix], dev_terms;
    int nfields = 0;
    gpmm_factor::RadialFields hterms[3];
    memset(hterms, 0, sizeof(hterms));
    HIP_TRY(ctx, dev_terms.alloc(sizeof(hterms)));
    KSpec specs[3];
    for (int q = 0; q < nsets; ++q) {
        const gingr_radial_kernel *k = kd[first[q]];
        KSpec &sp = specs[q];
        memset(&sp, 0, sizeof(sp));
        sp.kind = gpmm_factor::kKernelRadial;
        sp.mix.n = k->n_terms;
        sp.radial = dev_terms.as<gpmm_factor::RadialFields>() + q;
        for (int t = 0; t < k->n_terms; ++t) {
            const gingr_radial_term &term = k->terms[t];
            const double p2 = term.parameter * term.parameter;
            sp.mix.c[t] = term.family == GINGR_RADIAL_GAUSSIAN ? -(double)GINGR_EXP_TABLE * 1.4426950408889634074 / p2 : p2;
            sp.mix.s[t] = term.scaling;
            hterms[q].family[t] = term.family;
            if (!term.weight) continue;
            b.weighted = true;
            int f = 0;
            while (f < nfields && host_field[f] != term.weight) ++f;
            if (f == nfields) {
                host_field[nfields++] = term.weight;
                HIP_TRY(ctx, dev_field[f].alloc((size_t)M * sizeof(double)));
                HIP_TRY(ctx, hipMemcpyAsync(dev_field[f].p, term.weight, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            }
            hterms[q].weight[t] = dev_field[f].as<double>();
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(dev_terms.p, hterms, sizeof(hterms), hipMemcpyHostToDevice, ctx->stream));
    for (int d = 0; d < 3; ++d) {
        b.specs.k[d] = specs[set_of[d]];
        memcpy(b.family[d], hterms[set_of[d]].family, sizeof(b.family[d]));
    }
    return run_build(b, nsets > 1);
}

int gingr_gpmm_build_gaussian(gingr_ctx *ctx, int64_t M_total, const double *ref, int32_t n_kernels, const double *sigmas,
                              const double *scalings, double relative_tolerance, int32_t max_rank, int64_t row_begin,
                              int64_t row_end, gingr_model **out) {
    if (!ctx || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (M_total < 1 || !ref || n_kernels < 1 || n_kernels > kMaxMix || !sigmas || !scalings)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gpmm_build: need M >= 1 and 1..%d kernels", kMaxMix);
    gingr_scalar_kernel k;
    memset(&k, 0, sizeof(k));
    k.kind = GINGR_KERNEL_GAUSSIAN_MIXTURE, k.n_kernels = n_kernels, k.sigmas = sigmas, k.scalings = scalings;
    return gingr_gpmm_build_diagonal(ctx, M_total, ref, &k, &k, &k, relative_tolerance, max_rank, row_begin, row_end, out);
}

}  // extern "C"
