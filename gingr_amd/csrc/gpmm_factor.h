// The pivoted Cholesky factorisation of a scalar kernel over a point cloud on the device (gpmm.hip), for the translation units that
// consume its factor: the GPMM construction itself and the low-rank non-rigid CPD (classic_cpd.hip).  Internal to libgingr_hip.so.
#pragma once

#include "common.h"
#include "fastexp.h"

#include <functional>
#include <vector>

namespace gpmm_factor {

constexpr int kMaxMix = 8;

struct Mixture {
    int32_t n;
    double c[kMaxMix];  // -2048 log2(e) / sigma^2
    double s[kMaxMix];  // scaling
};

// One scalar kernel of a DiagonalKernel(k_x, k_y, k_z) (GPMMHelper.scala:96-142, KernelHelper.scala:25-84):
//   kind 0  sum_i scaling_i exp(-|x-y|^2/sigma_i^2)  [+ mirror * the same kernel at (Mx, y), M = diag(-1,1,1): the x-mirrored
//           kernel of KernelHelper.symmetrizeKernel -- xMirroredKernel3D evaluates kernel(Point(-x0, x1, x2), y)]
//   kind 1  scale * (x . y)          DotProductKernel.k returns x.dot(y) whatever kernel / gamma it wraps (KernelHelper.scala:43-51)
//   kind 2  scale * m[i][j]          LookupKernel on the reference points themselves (closest reference point of a reference
//                                     point = the point), m = pinv(graph Laplacian) (LaplacianHelper.scala:27-41)
//   kind 3  sum_t w_t[i] w_t[j] scaling_t f_t(|x-y|^2)   (gingr_gpmm_build_radial; only the Radial* factor kinds evaluate it): radial
//           terms with an optional weight field each over the points of the full reference.  mix.n terms, mix.s[t] = scaling_t,
//           mix.c[t] = the Gaussian's exponent factor as for kind 0, or beta^2 (KernelHelper.scala:53-73: val beta2 = beta * beta)
struct RadialFields {
    int32_t family[kMaxMix];        // GINGR_RADIAL_*
    const double *weight[kMaxMix];  // device, [M_total], or null: no field
};

struct KSpec {
    int32_t kind;
    Mixture mix;
    double mirror;
    double scale;
    union {
        const double *lookup;        // kind 2: device, M x M row-major
        const RadialFields *radial;  // kind 3: device
    };
};

constexpr int32_t kKernelRadial = 3;

struct KSpec3 {
    KSpec k[3];
};

// one Gaussian term scaling * exp(-|x-y|^2 / sigma^2) for all three coordinates
inline KSpec3 gaussian_specs(double sigma, double scaling) {
    KSpec3 s;
    memset(&s, 0, sizeof(s));
    for (KSpec &k : s.k) {
        k.kind = GINGR_KERNEL_GAUSSIAN_MIXTURE;
        k.mix.n = 1;
        k.mix.c[0] = -(double)GINGR_EXP_TABLE * 1.4426950408889634074 / (sigma * sigma);
        k.mix.s[0] = scaling;
    }
    return s;
}

// The basis a tapered kernel takes its entries from (gingr_model_localize): Qt [r][n], row q = column q of the source's
// Q = U sqrt(lambda) over the n = 3M (point, coordinate) entries in the caller's order.  qt == nullptr: none (every other build).
struct TaperBasis {
    const double *qt;
    int32_t r;
};

// What the pivoted Cholesky factors: one scalar kernel over the points; a DiagonalKernel with different kernels per coordinate over the
// 3M (point, coordinate) entries; or the full 3 x 3 block kernel g(x_i, x_j) (Q Q^T)[(i,a),(j,b)] over the same entries, g = specs.k[0].
// RadialScalar / RadialDiagonal: the first two over kernels of kind 3 -- instantiations of their own, so that the three above neither load
// a field nor branch on a family.
enum class FactorKind { Scalar = 0, Diagonal = 1, Tapered = 2, RadialScalar = 3, RadialDiagonal = 4 };

// pc_step_kernel<kind> of gpmm.hip
using StepKernel = void (*)(Cloud, KSpec3, TaperBasis, int32_t, int32_t, double, int32_t, double *, double *, int32_t *, const double *,
                            const int32_t *, const double *, double *, int32_t *, double *, int32_t *, double *, int32_t *, int32_t *,
                            int32_t *);

// The pivoted Cholesky factorisation on the device: over the M points for one scalar kernel, or (gen) over the 3M (point,
// coordinate) entries of a DiagonalKernel whose coordinates have different kernels, or (init_tapered) of a tapered basis kernel.
struct Factor {
    gingr_ctx *ctx = nullptr;
    KSpec3 specs{};
    Cloud pts{};
    TaperBasis basis{nullptr, 0};
    int timer = -1;    // timing hook of the pivot step (-1: none)
    StepKernel step_kernel = nullptr;
    int64_t n = 0;     // entries
    int nb = 0;
    int32_t kcap = 0;  // columns the buffers can hold
    int32_t ks = 0;    // columns computed
    DevBuf Lb, diag, piv, part, ctl, trace, pivots, swd, swo;  // Lb: [kcap][n], column r of the factor in row r
    std::vector<double> htrace;                                // residual trace after 0 .. ks columns
    double *pmaxv[2]{}, *ptrv[2]{};
    int32_t *pidxv[2]{};

    int init(gingr_ctx *c, const KSpec3 &k, const Cloud &p, bool gen, int32_t cap, bool radial = false);
    // the tapered kernel of `taper` (one Gaussian, all three coordinates) and the basis qb over the 3 p.n entries
    int init_tapered(gingr_ctx *c, const KSpec3 &taper, const Cloud &p, const TaperBasis &qb, int32_t cap, int timer_hook);
    int init_kind(gingr_ctx *c, const KSpec3 &k, const Cloud &p, FactorKind kind, int32_t cap);  // what the two above share
    void launch(int32_t k, double rel_tol);
    // the whole factorisation under the device's stopping rule (residual trace below rel_tol * trace, capacity, exhaustion)
    int run_to_tolerance(double rel_tol);
};

// The tail of a generic build (gpmm.hip), shared by the GPMM of coordinate-wise different kernels and gingr_model_localize: from the
// fg.ks columns of a factor over the 3M entries, G = L^T L and its eigenpairs (descending, as the solver leaves them, in lam); `choose`
// clamps or refuses them and names the leading columns to keep (or returns an error code, which ends the build); then the model of
// U sqrt(lambda) = L V for those columns on ref with `mean` ([3M] interleaved).  `keep` (optional) sees the eigenvectors
// V (device, fg.ks x fg.ks, V[row fg.ks + column]) and the number of kept columns right before the model is made, while the factor is
// alive and ahead of the synchronisations of the model's construction; its failure ends the build.
int generic_tail(gingr_ctx *ctx, Factor &fg, int64_t M, const double *ref, const double *mean, int64_t row_begin, int64_t row_end,
                 std::vector<double> &lam, const std::function<int(std::vector<double> &, int32_t *)> &choose, gingr_model **out,
                 const std::function<int(const double *, int32_t)> &keep_extension = nullptr);

}  // namespace gpmm_factor
