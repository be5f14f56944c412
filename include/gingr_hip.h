/*
 * gingr_hip.h -- C ABI of libgingr_hip.so, the MI355X (gfx950) implementation of GiNGR's
 * per-iteration update (reference: unibas-gravis/GiNGR, gingr/api/GingrAlgorithm.update).
 *
 * This header is the drop-in boundary: plain C, pointers and sizes only, no C++/torch/JVM types.
 * A JVM host binds it through the JNI shim in jvm/ (see INTEGRATION.md); the Python host layer
 * gingr_amd/ binds it with ctypes.  G/ = src/main/scala/gingr/ of the reference.
 *
 * Conventions
 *  - every function returns a gingr_status (0 = ok); gingr_last_error(ctx) has the text.
 *  - host point arrays are interleaved x,y,z float64 ("x1x,x1y,x1z,x2x,..."), the layout of
 *    G/api/registration/utils/PointSequenceConverter.scala:54-59.
 *  - the caller owns every host buffer; the library never keeps a host pointer after the call returns.
 *  - a gingr_ctx binds ONE device and ONE stream and is not thread-safe; distinct contexts are independent
 *    (one per MH chain / per GPU), mirroring the reference's "one algorithm instance per chain"
 *    (G/api/GingrAlgorithm.scala:69-70 retryCounter is an unsynchronised var).
 *  - functions whose name ends in _async only enqueue work on the context's stream.
 */
#ifndef GINGR_HIP_H
#define GINGR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gingr_ctx gingr_ctx;
typedef struct gingr_model gingr_model;
typedef struct gingr_fitter gingr_fitter;

typedef enum gingr_status {
    GINGR_OK = 0,
    GINGR_ERR_BAD_ARGUMENT = 1,
    GINGR_ERR_HIP = 2,          /* a HIP runtime call failed */
    GINGR_ERR_NONFINITE = 3,    /* a result is NaN/Inf (reference: exception inside Try => ModelFlexibilityError) */
    GINGR_ERR_NOT_SPD = 4,      /* Cholesky pivot <= 0 in the posterior solve (same mapping) */
    GINGR_ERR_NO_DEVICE = 5,
    GINGR_ERR_STATE = 6,        /* call order violated (e.g. update before target upload) */
    GINGR_ERR_NOT_CONVERGED = 7 /* an iterative solve reached its iteration cap (gingr_nicp_step) */
} gingr_status;

/* G/api/GlobalTranformationType.scala:20-24 */
typedef enum gingr_global_transform {
    GINGR_NO_TRANSFORMS = 0,
    GINGR_RIGID_TRANSFORMS = 1,
    GINGR_SIMILARITY_TRANSFORMS = 2
} gingr_global_transform;

/* G/api/FittingStatuses.scala:22 */
typedef enum gingr_fitting_status {
    GINGR_FIT_NONE = 0,
    GINGR_FIT_CONVERGED = 1,
    GINGR_FIT_MAX_ITERATION = 2,
    GINGR_FIT_MODEL_FLEXIBILITY_ERROR = 3
} gingr_fitting_status;

/* ------------------------------------------------------------------ context */

int gingr_device_count(void);
int gingr_ctx_create(int device, gingr_ctx **out);
void gingr_ctx_destroy(gingr_ctx *ctx);
const char *gingr_last_error(const gingr_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the context's own. NULL restores it. */
int gingr_ctx_set_stream(gingr_ctx *ctx, void *hip_stream);
void *gingr_ctx_get_stream(gingr_ctx *ctx);
int gingr_ctx_synchronize(gingr_ctx *ctx);
const char *gingr_build_info(void);
/* Run-time options of a context.  All of them select between code paths with IDENTICAL results (the tests compare them bit for bit);
 * they exist for those tests and for same-box timing comparisons, not for tuning -- nothing in the library reads the environment.
 *   GINGR_OPT_CULL       1 (default) / 0: exact-zero tile culling of the CPD passes and exact pruning of the closest-point scans
 *   GINGR_OPT_FINE_CULL  -1 (default: by the regime the device reports) / 0 / 1: quarter-tile culling variant of the CPD passes
 *   GINGR_OPT_NN_GRID    1 (default) / 0: the ICP closest point searches the target's uniform grid first / tile scan only;
 *                        2: as 1, and the stateless gingr_nn searches a grid too (built per call; from a cold start its
 *                        default forms -- all pairs up to 2^26 of them, the box-pruned scan above -- are faster)
 *   GINGR_OPT_TRI_GRID   0 / 1 (default) / 2: the surface ICP's closest surface point searches a grid of the (fixed) target triangles
 *                        first, warm-started from the previous iteration, and the tile scan only answers what the grid cannot certify:
 *                        never / from 16 384 target triangles on / always.  2 also bins the MOVING template's triangles on the device
 *                        in front of every self-intersection test (round 5; same decisions, measured slower than the tile scan at 41k x 82k)
 *   GINGR_OPT_SPLIT_EXCHANGE  0 (default) / 1: row-sharded CPD through the library's own RCCL exchange (gingr_fitter_update_*_rccl_async):
 *                        the column-sum pass runs in two halves of the target tiles and the all-reduce of the first half is enqueued on a
 *                        second stream of the context (event-ordered, same communicator) while the second half computes, so that only
 *                        the second half's all-reduce is exposed.  Costs two short launches instead of one (the emulated per-rank time
 *                        rises by a few microseconds); whether it pays depends on the all-reduce latency of the node.
 *                        Same sums up to the order of the chunk partials (<= 1e-12 on the state).
 *   GINGR_OPT_GRAM_DOWNDATE  -1 (default: from 16 384 local rows on) / 1 / 0: ICP with a surface correspondence gives every accepted pair
 *                        the weight 1 / sigma2 and every rejected one 0 (ICP.scala:50,90-92), so its weighted Gram matrix is the model's
 *                        one-off moment Q^T Q minus the rows of the rejected vertices, scaled: one pass over the rejected rows (0.2 % of
 *                        them at 41k) instead of one over the basis / 0: the pass over the basis.  Same matrix up to the rounding of the
 *                        subtraction (<= 1e-12).  -1 also decides again on the DEVICE in every iteration: with more than one zero-weight
 *                        vertex in eight (open targets, partial overlap) the pass over the basis runs, exactly as with 0 (round 6; a
 *                        fixed rule -- the choice never depends on timing); 1 forces the downdate whatever the rejected fraction is.
 *                        Results are therefore NOT bit-stable across the 16 384-row threshold, across the one-in-eight rule or across
 *                        this option: the two forms round differently, and the exact `intersection point != vertex` comparison of the
 *                        self-intersection test (ClosestPointRegistrator.scala:67) can turn a last-bit difference into a different
 *                        accept / reject decision in the next iteration.
 *   GINGR_OPT_DECIMATE_BATCH  16 (default), 1 .. 60: gingr_mesh_decimate enqueues this many steps of its cube-size bisection before it reads
 *                        the control block back; the steps behind the deciding one return at once.  1 = one read-back per step.
 *   GINGR_OPT_SEPARABLE  -1 (default) / 0: a model whose basis columns each live on one coordinate (every model built from a diagonal
 *                        kernel; gingr_model_separable) keeps a compact copy of its basis, and a single-shard CPD or isotropic-pairs
 *                        update without landmarks or a sampled proposal forms the weighted Gram matrix, solves the posterior and
 *                        writes the fit as three scalar-valued problems over it / 0: the dense passes.  Same results up to the
 *                        summation order.
 * No reference counterpart (the reference has one code path per operation). */
typedef enum gingr_ctx_option {
    GINGR_OPT_CULL = 0,
    GINGR_OPT_FINE_CULL = 1,
    GINGR_OPT_NN_GRID = 2,
    GINGR_OPT_TRI_GRID = 3,
    GINGR_OPT_SPLIT_EXCHANGE = 4,
    GINGR_OPT_GRAM_DOWNDATE = 5,
    GINGR_OPT_DECIMATE_BATCH = 6,
    GINGR_OPT_SEPARABLE = 7
} gingr_ctx_option;
int gingr_ctx_set_option(gingr_ctx *ctx, int32_t option, int32_t value);
int gingr_ctx_get_option(gingr_ctx *ctx, int32_t option, int32_t *value);

/* --------------------------------------------- stateless all-pairs operators
 * Each call uploads its inputs, runs on the device, downloads and synchronises.
 */

/*
 * CPD soft-assignment statistics of ONE affinity evaluation, P never materialised.
 * Replaces CpdRegistrationState.P (G/api/registration/config/CPD.scala:54-75), the row/column sums of
 * CPDCorrespondence.estimate (:36) and updateSigma2 (:133-147).
 *   fit[3M], target[3N], sigma2, w  ->  den[N] (= colsum K + c), P1[M], PX[3M], Pt1[N],
 *   scalars[6] = { Np, xPx, trPXY, yPy, sigma2_next, c }.   Any output pointer may be NULL.
 */
int gingr_cpd_stats(gingr_ctx *ctx, int64_t M, const double *fit, int64_t N, const double *target, double sigma2,
                    double w, double *den, double *P1, double *PX, double *Pt1, double *scalars);

/* sigma2_0 = sum_ij ||x_j - y_i||^2 / (3 M N)      (CPD.scala:81-90) */
int gingr_cpd_initial_sigma2(gingr_ctx *ctx, int64_t M, const double *ref, int64_t N, const double *target,
                             double *sigma2_out);

/*
 * Exact brute-force nearest neighbour, lowest index wins ties.
 * Replaces ClosestPointUnstructuredPointsDomain3D.closestPointCorrespondence
 * (G/api/registration/utils/ClosestPointRegistrator.scala:133-148) / scalismo findClosestPoint.
 *   query[3M], target[3N] -> idx[M] (int32), d2[M] (squared distance), *mean_distance (mean of sqrt(d2)).
 */
int gingr_nn(gingr_ctx *ctx, int64_t M, const double *query, int64_t N, const double *target, int32_t *idx,
             double *d2, double *mean_distance);

/*
 * Gaussian-kernel covariance block out[i*nb + j] = scaling * exp(-||a_i - b_j||^2 / sigma^2)
 * (G/api/gpmm/GPMMHelper.scala:99-102: GaussianKernel(sigma) * scaling; the (x) I3 of DiagonalKernel is implicit;
 *  with sigma = sqrt(2) beta, scaling = 1 it is CPDFactory.initializeKernelMatrixG,
 *  G/other/algorithms/cpd/CPDFactory.scala:54-66).
 */
int gingr_gauss_block(gingr_ctx *ctx, int64_t na, const double *A, int64_t nb, const double *B, double sigma,
                      double scaling, double *out);

/* ------------------------------------------------------------------- model
 * A point distribution model resident on the device: scalismo PointDistributionModel (reference, mean, basisMatrix,
 * variance) as held by GeneralRegistrationState.model (G/api/GeneralRegistrationState.scala:29).
 *   ref[3M], mean[3M] (mean DISPLACEMENT), basis[3M*r] COLUMN-major (3M rows) exactly as Breeze stores
 *   basisMatrix, variance[r].
 * Row sharding (multi-GPU): the model holds points [row_begin, row_end) of M_total; pass 0, M for one GPU.
 * Host arrays are always the FULL model; only the shard is uploaded.
 */
int gingr_model_upload(gingr_ctx *ctx, int64_t M_total, int32_t rank, const double *ref, const double *mean,
                       const double *basis_colmajor, const double *variance, int64_t row_begin, int64_t row_end,
                       gingr_model **out);
void gingr_model_destroy(gingr_model *model);
/* Row-sharded models only: after upload every shard holds its partial one-off moments of the basis (Q^T Q and the
 * per-coordinate cross moments; float64, count elements at dev_ptr); the host all-reduces (sum) them across shards once,
 * then calls gingr_model_finalize, which factors Q^T Q / 1e-5 + I for the coefficient projections.
 * Single-shard uploads are finalized by gingr_model_upload. */
int gingr_model_gram_exchange(gingr_model *model, void **dev_ptr, int64_t *count);
int gingr_model_finalize(gingr_ctx *ctx, gingr_model *model);
/* ---- GPMM construction on the device ----------------------------------------------------------
 * Replaces GPMMTriangleMesh3D(reference, relativeTolerance).Gaussian / .GaussianMixture / .AutomaticGaussian
 * (G/api/gpmm/GPMMHelper.scala:96-130) and automaticGPMMfromTemplate (G/api/registration/utils/GPMMHelper.scala:39-69):
 * zero-mean GP with DiagonalKernel(sum_i scaling_i * GaussianKernel(sigma_i), 3), low-rank approximation by scalismo's
 * pivoted Cholesky (stopped at relative_tolerance * trace, or at max_rank columns; max_rank <= 0 means the model limit
 * 512) and the eigen-decomposition of its factor (LowRankGaussianProcess.approximateGPCholesky, GPMM.construct :39-55).
 * The basis is produced in HBM; the result is a finished (single shard) or to-be-finalized (row shard) gingr_model exactly
 * as from gingr_model_upload.  ref = interleaved xyz of the FULL reference; row_end <= 0 means M_total. */
int gingr_gpmm_build_gaussian(gingr_ctx *ctx, int64_t M_total, const double *ref, int32_t n_kernels, const double *sigmas,
                              const double *scalings, double relative_tolerance, int32_t max_rank, int64_t row_begin,
                              int64_t row_end, gingr_model **out);
/* The other kernels of GPMMTriangleMesh3D (G/api/gpmm/GPMMHelper.scala:96-142) and gingr.simple.SimpleTriangleModels3D.create
 * (G/simple/SimpleModels.scala:52-75): a DiagonalKernel with one scalar kernel per coordinate,
 *   GINGR_KERNEL_GAUSSIAN_MIXTURE  sum_i scalings[i] exp(-|x-y|^2 / sigmas[i]^2), plus mirror * the same kernel evaluated at
 *                                  (diag(-1,1,1) x, y) when mirror = +-1 -- KernelHelper.symmetrizeKernel (KernelHelper.scala:25-38):
 *                                  GaussianSymmetry = (mirror -1 for x, +1 for y and z)
 *   GINGR_KERNEL_DOT               scaling * (x . y) -- DotProductKernel.k returns x.dot(y) whatever kernel / gamma it wraps
 *                                  (KernelHelper.scala:40-51): GaussianDot(sigma, scaling), InverseLaplacianDot(scaling, gamma)
 *   GINGR_KERNEL_LOOKUP            scaling * lookup[i * M_total + j] -- LookupKernel(reference, m) on the reference points
 *                                  (KernelHelper.scala:76-84), m = pinv(graph Laplacian) for InverseLaplacian (host array)
 * Three equal kernels run one scalar pivoted Cholesky (the coordinates swap in triplets); different kernels run scalismo's
 * generic factorisation over the 3M (point, coordinate) entries.  Exact ties follow scalismo's rule (first maximum in the
 * permuted index order).  kx / ky / kz may be the same pointer.
 * gingr_gpmm_build_gaussian(..) == gingr_gpmm_build_diagonal with the same mixture (mirror 0) three times. */
#define GINGR_KERNEL_GAUSSIAN_MIXTURE 0
#define GINGR_KERNEL_DOT 1
#define GINGR_KERNEL_LOOKUP 2
typedef struct gingr_scalar_kernel {
    int32_t kind;
    int32_t n_kernels;       /* mixture */
    const double *sigmas;    /* mixture, host */
    const double *scalings;  /* mixture, host */
    double mirror;           /* mixture: 0, +1 or -1 */
    double scaling;          /* dot / lookup */
    const double *lookup;    /* lookup: host, M_total x M_total row-major */
} gingr_scalar_kernel;
int gingr_gpmm_build_diagonal(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_scalar_kernel *kx,
                              const gingr_scalar_kernel *ky, const gingr_scalar_kernel *kz, double relative_tolerance,
                              int32_t max_rank, int64_t row_begin, int64_t row_end, gingr_model **out);
/* NOTE on max_rank of the two entries above: it is clamped to 512 (the rank limit of a model) SILENTLY -- a factorisation that
 * has not met relative_tolerance after 512 columns comes back as a 512-column model with GINGR_OK.  The entry below never does that.
 *
 * gingr_gpmm_build_diagonal_ex: the same construction with the factor allowed to be longer than the model, as the reference's
 * pivoted Cholesky (no rank limit, G/api/gpmm/GPMMHelper.scala:39-52) followed by PointDistributionModel.truncate(k).
 *   max_columns > 0   the caller's stop: at most that many factor columns; stopping there is no error (tolerance_reached = 0).
 *                     Above GINGR_GPMM_MAX_COLUMNS: GINGR_ERR_BAD_ARGUMENT.
 *   max_columns <= 0  to tolerance: the factorisation runs until relative_tolerance is met.  If the library's ceiling of
 *                     GINGR_GPMM_MAX_COLUMNS columns (or 3 M_total) comes first: GINGR_ERR_BAD_ARGUMENT, the text names the
 *                     ceiling and the residual fraction.
 *   keep_rank > 0     the model keeps the keep_rank leading eigenpairs of the merged, descending spectrum (equal eigenvalues in
 *                     the order of the untruncated model); keep_rank <= 0 or >= columns keeps everything.
 * A model above rank 512 is GINGR_ERR_BAD_ARGUMENT (the text names `columns`; ask again with keep_rank <= 512), never a shorter
 * model; *out stays NULL.  info (may be NULL) is filled whenever the factorisation itself finished, also on these errors.
 * Coordinates with different kernels (GaussianSymmetry) stay within 512 factor columns: needing more is GINGR_ERR_BAD_ARGUMENT.
 * With max_columns <= 512 and keep_rank <= 0 the model is bit-identical to gingr_gpmm_build_diagonal's with max_rank = max_columns. */
#define GINGR_GPMM_MAX_COLUMNS 1536
typedef struct gingr_gpmm_info {
    int32_t columns;               /* factor columns the pivoted Cholesky produced (= the model's rank before truncation) */
    int32_t rank;                  /* rank of the returned model */
    int32_t tolerance_reached;     /* 1: residual trace < relative_tolerance * trace when the factorisation stopped */
    double residual_fraction;      /* residual trace / trace at the stop */
    double kept_variance_fraction; /* sum of kept eigenvalues / sum of all `columns` eigenvalues (1 without truncation) */
} gingr_gpmm_info;
int gingr_gpmm_build_diagonal_ex(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_scalar_kernel *kx,
                                 const gingr_scalar_kernel *ky, const gingr_scalar_kernel *kz, double relative_tolerance,
                                 int32_t max_columns, int32_t keep_rank, int64_t row_begin, int64_t row_end, gingr_gpmm_info *info,
                                 gingr_model **out);
/* Spatially varying and non-Gaussian kernels: one scalar kernel per coordinate of the form
 *     k(x_i, x_j) = sum_t  w_t[i] w_t[j] scaling_t f_t(|x_i - x_j|^2)          1 <= n_terms <= 8
 * with a radial family per term,
 *   GINGR_RADIAL_GAUSSIAN              exp(-nn / parameter^2)          (parameter = sigma; the arithmetic of the mixture above)
 *   GINGR_RADIAL_RATIONAL_QUADRATIC    1 - nn / (nn + parameter^2)     (RationalQuadratic(beta), KernelHelper.scala:64-73)
 *   GINGR_RADIAL_INVERSE_MULTIQUADRIC  1 / sqrt(nn + parameter^2)      (InverseMultiquadric(beta), KernelHelper.scala:53-61)
 * and an optional weight field per term over the M_total points of the full reference (host, any real values; NULL: none).  The sum
 * is D_t K_t D_t over the terms, positive semi-definite for any weights: a kernel scaled by a function of position, and with two
 * terms weighted by s and 1 - s scalismo's ChangePointKernel.  One term's value is ((scaling * f) * w[i]) * w[j], terms are added
 * left to right; a field of ones gives the bits of no field, and Gaussian terms without fields give the bits of
 * gingr_gpmm_build_diagonal_ex with the same mixture.  A point whose weights are all zero never becomes a pivot and its basis rows
 * are exact zeros: it stays on the reference.
 * max_columns, keep_rank, info, the row shard and every stop and error are those of gingr_gpmm_build_diagonal_ex.  kx / ky / kz may
 * be the same pointer; kernels that are equal term by term (fields by pointer, then by content) run one scalar factorisation,
 * different ones the generic factorisation over the 3 M_total entries (at most 512 factor columns).  Every distinct field goes to the
 * device once.  GINGR_ERR_BAD_ARGUMENT with a message that names the term, *out == NULL: n_terms outside 1..8, an unknown family, a
 * parameter or scaling that is not finite and positive, a weight that is not finite, a kernel whose diagonal is zero at every point. */
#define GINGR_RADIAL_GAUSSIAN 0
#define GINGR_RADIAL_RATIONAL_QUADRATIC 1
#define GINGR_RADIAL_INVERSE_MULTIQUADRIC 2
typedef struct gingr_radial_term {
    int32_t family;
    double parameter;     /* sigma or beta */
    double scaling;
    const double *weight; /* host, M_total, or NULL */
} gingr_radial_term;
typedef struct gingr_radial_kernel {
    int32_t n_terms;
    const gingr_radial_term *terms;
} gingr_radial_kernel;
int gingr_gpmm_build_radial(gingr_ctx *ctx, int64_t M_total, const double *ref, const gingr_radial_kernel *kx,
                            const gingr_radial_kernel *ky, const gingr_radial_kernel *kz, double relative_tolerance,
                            int32_t max_columns, int32_t keep_rank, int64_t row_begin, int64_t row_end, gingr_gpmm_info *info,
                            gingr_model **out);
/* PointDistributionModel.truncate(k): a new, finalized, independent model of the k leading basis functions of a complete
 * (single-shard, finalized) model of this context, built or uploaded; 1 <= k <= rank, else GINGR_ERR_BAD_ARGUMENT.  A row
 * shard is refused: build the shards with keep_rank, or truncate the complete model. */
int gingr_model_truncate(gingr_ctx *ctx, const gingr_model *src, int32_t k, gingr_model **out);
/* ---- Kernel extension: a model built from a kernel, at points off its reference.
 * The pivoted Cholesky of a GPMM build reproduces the kernel exactly on its pivot rows, so every basis function of the model is a fixed
 * combination of kernel functions centred at the pivots:  Q(x)[d, :] = sum_j k_d(x, p_dj) C_d[j, :],  L_P^T C_d = V_d  (L_P: the factor's
 * rows at coordinate d's pivots, V_d: the kept eigenvectors).  At the model's own vertices this gives back the model's rows, elsewhere
 * the Nystroem extension of scalismo's continuous LowRankGaussianProcess.  Far from every pivot the extended model has no variance (the
 * deformation goes to zero): that is the extension's nature.
 * A complete model carries the extension when it was built by gingr_gpmm_build_gaussian / _diagonal / _diagonal_ex / _radial from
 * Gaussian mixtures (with or without mirror), the dot-product kernel or radial terms WITHOUT weight fields; so does what
 * gingr_model_truncate and gingr_model_extend make of such a model.  Lookup kernels, radial terms with weight fields, row shards and
 * every other model (uploaded, interpolated, posterior, PCA, augmented, localized, spectral) carry none: the entries below that need
 * one answer GINGR_ERR_STATE, and the message names the reason.  C is formed at the first use (one back substitution on the device).
 *
 * gingr_model_kernel_extension: available = 0 / 1 (no error for a model without one); counts (nullable): pivots per coordinate;
 * shared_kernel (nullable): 1 when the three coordinates share one kernel and their pivot lists are prefixes of one sequence.  A query:
 * nothing is computed, except for a model whose coordinates have different kernels and whose extension has not been used yet -- its
 * pivots are counted per coordinate by forming the extension, which can fail with GINGR_ERR_HIP. */
int gingr_model_kernel_extension(const gingr_model *model, int32_t *available, int32_t counts[3], int32_t *shared_kernel);
/* The pivots of coordinate d (0..2) in pivot order: their ids (pivot_ids [counts[d]], nullable) into the reference of the model the
 * extension was BUILT on -- this model's own reference, unless it was made by gingr_model_extend, which shares its source's extension
 * and has other points: read the ids of such a model against its source's reference --, and C_d row-major [counts[d]][rank] (coeff,
 * nullable). */
int gingr_model_get_kernel_extension(gingr_ctx *ctx, const gingr_model *model, int32_t d, int32_t *pivot_ids, double *coeff);
/* A new, finalized, independent single-shard model on the M_new >= 1 points new_ref_xyz [3 M_new]: zero mean, the source's variances
 * bit for bit, basis rows Q(x) evaluated on the device (float64 MFMA) straight into the new model; it carries the source's extension
 * (the same pivots and C), so it extends again to the same rows.  A point's row depends on the point alone, not on the other points
 * of the call.  Non-finite points: GINGR_ERR_NONFINITE. */
int gingr_model_extend(gingr_ctx *ctx, const gingr_model *src, int64_t M_new, const double *new_ref_xyz, gingr_model **out);
/* out_p = s (R (x_p + u(x_p) - c) + c + t),  u(x)[d] = sum_j k_d(x, p_dj) (C_d alpha)[j]: the model's deformation field for the
 * coefficients alpha [rank] at the P >= 1 host points points_xyz [3 P] under the pose convention of gingr_model_instance; out_xyz [3 P]
 * (may be points_xyz).  No basis of the P points is formed; the points stream through the device in slabs, P is limited by host memory
 * alone.  Non-finite points or coefficients: GINGR_ERR_NONFINITE, and out_xyz is left untouched. */
int gingr_model_warp_points(gingr_ctx *ctx, const gingr_model *model, const double *alpha, const double euler[3], const double center[3],
                            const double translation[3], double scale, int64_t P, const double *points_xyz, double *out_xyz);
/* PointSetHelper.maximumPointDistance / minimumPointDistance (GPMMHelper.scala:75-87; the O(n^2) scans behind
 * AutomaticGaussian and automaticGPMMfromTemplate): largest pairwise distance, smallest distance to the nearest OTHER point. */
int gingr_pointset_distance_extrema(gingr_ctx *ctx, const double *xyz, int64_t n, double *max_distance, double *min_distance);
/* Copy the local rows of a model back to the host in gingr_model_upload's layout (any pointer may be NULL):
 * ref / mean [3 M_local], basis column-major [3 M_local x rank] (unit columns: Q0 / sqrt(variance)), variance [rank]. */
int gingr_model_download(gingr_ctx *ctx, const gingr_model *model, double *ref, double *mean, double *basis_colmajor,
                         double *variance);
int64_t gingr_model_num_points(const gingr_model *model); /* local rows */
int32_t gingr_model_rank(const gingr_model *model);
/* Whether every basis column of the (finalised) model is supported on one coordinate only -- decided on the device from the local basis,
 * entries of +-0.0 counting as absent -- the number of columns per coordinate (class_counts, nullable; zeros when not separable), and
 * whether the model keeps the compact basis the separable passes read (compact, nullable; GINGR_OPT_SEPARABLE). */
int gingr_model_separable(const gingr_model *model, int32_t *separable, int32_t class_counts[3], int32_t *compact);

/* PointDistributionModel.instance(alpha) posed and scaled:  s * (R (ref + mean + U sqrt(lam) alpha - c) + c + t)
 * (G/api/ModelFittingParameters.scala:130-143).  out_xyz[3*M_local]. */
int gingr_model_instance(gingr_ctx *ctx, const gingr_model *model, const double *alpha, const double euler[3],
                         const double center[3], const double translation[3], double scale, double *out_xyz);

/* PointDistributionModel.transform(rigid).coefficients(mesh): GP regression at all points with noise 1e-5 I3
 * (G/api/GingrAlgorithm.scala:212-216,234-237).  mesh_xyz[3*M_local] -> alpha[r].  Single shard only. */
int gingr_model_coefficients(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                             const double translation[3], const double *mesh_xyz, double *alpha);

/* PointDistributionModel.transform(rigid).posterior(obs).mean  (G/api/GingrAlgorithm.scala:297-301).
 * Observations: every local point i with weight[i] > 0 is observed at obs_xyz[3i..] with covariance I3/weight[i];
 * n_lm landmark observations (point id, target point, full 3x3 covariance, row-major) are appended and their point ids
 * must carry weight 0.  Outputs: mean_xyz[3*M_local] (posterior mean mesh), coeffs[r] (regression coefficients). */
int gingr_model_posterior_mean(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                               const double translation[3], const double *obs_xyz, const double *weight,
                               int32_t n_lm, const int32_t *lm_pid, const double *lm_xyz, const double *lm_cov,
                               double *mean_xyz, double *coeffs);

/* ------------------------------------------------------------------ fitter
 * Device-resident registration state = the numeric content of GeneralRegistrationState
 * (alpha, Euler angles, centre, translation, scale, sigma2, fit, iteration, status) plus target and
 * configuration; one update = GingrAlgorithm.update followed by GingrGeneratorWrapper.propose's fit refresh
 * (G/api/GingrAlgorithm.scala:192-254; G/api/sampling/generators/GingrGeneratorWrapper.scala:28-39).
 */
typedef struct gingr_state_scalars {
    double euler[3];        /* phi, theta, psi  (EulerAngles, G/api/ModelFittingParameters.scala:35-37) */
    double center[3];       /* rotation centre */
    double translation[3];
    double scale;
    double sigma2;
    int32_t iteration;
    int32_t status;         /* gingr_fitting_status */
} gingr_state_scalars;

typedef struct gingr_cpd_params {   /* CpdConfiguration, CPD.scala:105-115 */
    double w;
    double lambda;
} gingr_cpd_params;

typedef struct gingr_icp_params {   /* IcpConfiguration, ICP.scala:54-66 (PointcloudClosestPoint flavour) */
    double initial_sigma;
    double end_sigma;
    int32_t max_iterations;
} gingr_icp_params;

int gingr_fitter_create(gingr_ctx *ctx, const gingr_model *model, gingr_fitter **out);
void gingr_fitter_destroy(gingr_fitter *f);
/* target cloud, replicated on every shard */
int gingr_fitter_set_target(gingr_fitter *f, int64_t N, const double *target_xyz);
/* landmark observations (GeneralRegistrationState.landmarkCorrespondences, GeneralRegistrationState.scala:43-62);
 * pids are GLOBAL point ids; cov row-major 3x3 per landmark.  n_lm = 0 clears. */
int gingr_fitter_set_landmarks(gingr_fitter *f, int32_t n_lm, const int32_t *lm_pid, const double *lm_xyz,
                               const double *lm_cov);
int gingr_fitter_set_options(gingr_fitter *f, int32_t global_transform, double step_length);
/* The stopping rule of a run, applied on the device (GingrAlgorithm.run's dropWhile, G/api/GingrAlgorithm.scala:142-153, with the
 * CPD rule |sigma2 - last sigma2| < threshold, G/api/registration/config/CPD.scala:108-110): with threshold >= 0 an update that
 * moves sigma2 by less than threshold marks the device state as stopped, and every later update enqueued on it leaves it as it is
 * -- exactly like a failed fit -- so a host can enqueue all updates of a run in ONE call and read the state it stopped at.
 * threshold < 0 (the default): no rule.  The call also clears the mark; so does gingr_fitter_set_state.
 * gingr_fitter_stop_rule_hit: the mark as of the last gingr_fitter_get_state (no transfer of its own). */
int gingr_fitter_set_stop_threshold(gingr_fitter *f, double threshold);
int gingr_fitter_stop_rule_hit(gingr_fitter *f, int32_t *hit);
/* Whether the last update committed, as of the last gingr_fitter_get_state (no transfer of its own): 0, or the error code
 * (GINGR_ERR_NOT_SPD / GINGR_ERR_NONFINITE) of the failure the Try rules of `update` turned into "state unchanged" or
 * ModelFlexibilityError.  A host that applies an updateSigma2 of its own applies it to committed updates only
 * (G/api/GingrAlgorithm.scala:238-247). */
int gingr_fitter_last_update_error(gingr_fitter *f, int32_t *code);
/* state in: alpha[r] + scalars; the fit is recomputed on the device (modelInstanceShapePoseScale). */
int gingr_fitter_set_state(gingr_fitter *f, const double *alpha, const gingr_state_scalars *s);
/* state out (synchronises): alpha[r], scalars, fit_xyz[3*M_local]; any pointer may be NULL. */
int gingr_fitter_get_state(gingr_fitter *f, double *alpha, gingr_state_scalars *s, double *fit_xyz);
/* diagnostics of the LAST update (synchronises): P1[M_local], PX[3*M_local] (CPD) or nn idx (ICP), coeffs. */
int gingr_fitter_get_cpd_stats(gingr_fitter *f, double *P1, double *PX, double *den, double *scalars6);
int gingr_fitter_get_icp_idx(gingr_fitter *f, int32_t *idx, double *d2);

/* n_iterations updates back to back on the stream, no host synchronisation in between (single shard). */
int gingr_fitter_update_cpd_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t n_iterations);
int gingr_fitter_update_icp_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations);

/* ---- ICP with the surface correspondence -----------------------------------------------------------
 * The reference's DEFAULT ICP method: ICPCorrespondence.estimate with TriangularClosestPoint (ICP.scala:36-52,63) ->
 * ClosestPointTriangleMesh3D.closestPointCorrespondence (ClosestPointRegistrator.scala:75-100): closest point on the target
 * SURFACE, rejected (weight 0) when the nearest target vertex is a boundary vertex, when the vertex normals are opposite, or
 * when the line through the template vertex along the closest-point vector meets the template itself first.
 * gingr_fitter_set_meshes: triangle lists (vertex ids of the model reference resp. of the target set by
 * gingr_fitter_set_target, 3 ids per triangle); call it after gingr_fitter_set_target.  On a row shard the model triangles are those
 * of the WHOLE template (ids of the full model) and the update runs through the sharded entry points further down.
 * The self-intersection test restates scalismo's getIntersectionPoints as a Moeller-Trumbore line/triangle test
 * (semantics unpinned without the scalismo source). */
int gingr_fitter_set_meshes(gingr_fitter *f, int64_t n_model_triangles, const int32_t *model_triangles,
                            int64_t n_target_triangles, const int32_t *target_triangles);
/* 0 = TriangularClosestPoint (default), 1 = AlongNormalClosestPoint (ClosestPointRegistrator.scala:102-131: the target point
 * hit first by the line through the template vertex along its vertex normal; no hit = rejected) */
int gingr_fitter_set_surface_method(gingr_fitter *f, int32_t method);
/* reverseCorrespondenceDirection (ICP.scala:46-48, ClosestPointRegistrator.scala:34-49): the correspondence is computed from the
 * target to the template and inverted; holds for all three ICP flavours until reset (call after gingr_fitter_set_target and, for
 * the surface flavours, gingr_fitter_set_meshes).  gingr_fitter_get_reversed_correspondence: per TARGET vertex the template vertex
 * it was assigned to and its weight in {0, 1} (last phase 0). */
int gingr_fitter_set_correspondence_direction(gingr_fitter *f, int32_t reversed);
int gingr_fitter_get_reversed_correspondence(gingr_fitter *f, int32_t *model_vertex_id, double *w);
int gingr_fitter_update_icp_surface_async(gingr_fitter *f, const gingr_icp_params *params, int32_t n_iterations);
int gingr_fitter_icp_surface_phase_async(gingr_fitter *f, const gingr_icp_params *params, int32_t phase);
/* probabilistic proposal / log transition density with the surface correspondence (see the _sample / _logpdf entry points below) */
int gingr_fitter_update_icp_surface_sample_async(gingr_fitter *f, const gingr_icp_params *params, const double *z);
int gingr_fitter_posterior_logpdf_icp_surface(gingr_fitter *f, const gingr_icp_params *params, const double *mesh_xyz,
                                              double *logpdf);
/* correspondences of the last surface phase 0: closest surface point [3 M] and weight in {0, 1} [M] per model vertex */
int gingr_fitter_get_surface_correspondence(gingr_fitter *f, double *cp_xyz, double *w);

/* ---- surface distance statistics ("the same query inside IndependentPointDistanceEvaluator") ----
 * d_i = |p_i - closestPointOnSurface(p_i)| reduced on the device: out = {sum d, max d, number of points counted,
 * sum of log N(d; 0, sdev)} (the last is 0 when sdev == 0; breeze Gaussian(0, sdev).logPdf).
 * gingr_fitter_surface_distance_stats works on the fitter's CURRENT state (meshes from gingr_fitter_set_meshes):
 *   direction 0: the first n_points vertices of the current fit (0 = all; `points` must be NULL) against the target surface
 *                = IndependentPointDistanceEvaluator.distModelToTarget
 *                  (G/api/sampling/evaluators/IndependentPointDistanceEvaluator.scala:54-60; with numberOfPointsForComparison
 *                  the reference walks the decimated instance's point ids 0..n'-1 over the full sample, :49-50);
 *   direction 1: `points` [3 n_points] (NULL = every target vertex) against the surface of the current fit
 *                = distTargetToModel (:62-67).
 * boundary_aware != 0 skips the points whose surface point lies nearest to a boundary vertex of the mesh
 * (G/api/helper/RegistrationComparison.scala:63-73, avgDistanceBoundaryAware).
 * gingr_mesh_distance_stats is the same reduction for any point list against any triangle mesh (host arrays):
 * MeshMetrics.avgDistance = out[0] / out[2], RegistrationComparison.maxDistance (:24-35) = out[1], Hausdorff = the larger of
 * the two directed maxima.  Both calls synchronise. */
int gingr_fitter_surface_distance_stats(gingr_fitter *f, int32_t direction, int64_t n_points, const double *points,
                                        int32_t boundary_aware, double sdev, double out[4]);
int gingr_mesh_distance_stats(gingr_ctx *ctx, int64_t n_points, const double *points, int64_t n_vertices, const double *vertices,
                              int64_t n_triangles, const int32_t *triangles, int32_t boundary_aware, double sdev, double out[4]);


/* Closest point of a triangle mesh to every query point (scalismo mesh.operations.closestPointOnSurface, the query behind
 * ClosestPointTriangleMesh3D, ClosestPointRegistrator.scala:75-100, and TriangleMeshInterpolator3D): cp_xyz[3n], squared
 * distance d2[n], the triangle tri_id[n] it lies in (lowest triangle number on exact ties) and the barycentric weights bary[3n] of
 * that triangle's three corners at the closest point (vertex -> (1,0,0), edge -> (1-q, q, 0)).  Any output may be NULL. */
int gingr_mesh_closest_points(gingr_ctx *ctx, int64_t n_points, const double *points, int64_t n_vertices, const double *vertices,
                              int64_t n_triangles, const int32_t *triangles, double *cp_xyz, double *d2, int32_t *tri_id,
                              double *bary);
/* Mesh decimation by vertex clustering (the step behind SimpleRegistrator.scala:84-106, IndependentPointDistanceEvaluator.scala:44-50
 * and examples/DemoHelper/DemoDatasetLoader.scala:34; scalismo's own mesh.operations.decimate is not restated): the bounding box is
 * cut into cubes, every occupied cube keeps its vertex closest to the mean of the cube's vertices (lowest index on ties), the
 * triangles are re-indexed, and the collapsed and the repeated ones (same corner set: the first stays) are dropped.  The cube size is
 * bisected so that the number of kept vertices is the closest reachable to n_target from above.  The definition is
 * gingr_amd/simple.py: cluster_decimate, and the result is that function's, bit for bit.
 * kept_ids[*n_kept] (capacity n_vertices): original vertex indices, ascending.  out_triangles[3 * *n_out_triangles] (capacity
 * 3 n_triangles) index into kept_ids and keep their original order.  triangles == NULL: a point cloud (n_triangles,
 * n_out_triangles and out_triangles are ignored).  n_target >= n_vertices is the identity: all ids, the triangles untouched.
 * *cube_size = the chosen cube edge, 0 when nothing was decimated.  n_target < 1, n_vertices < 1 or > INT32_MAX, a triangle id out
 * of range and a non-finite coordinate are GINGR_ERR_BAD_ARGUMENT.  Host arrays in and out; the call synchronises. */
int gingr_mesh_decimate(gingr_ctx *ctx, int64_t n_vertices, const double *vertices, int64_t n_triangles, const int32_t *triangles,
                        int64_t n_target, int64_t *n_kept, int32_t *kept_ids, int64_t *n_out_triangles, int32_t *out_triangles,
                        double *cube_size);
/* model.newReference(newReference, interpolator) (scalismo PointDistributionModel; used as
 * SimpleRegistrator.scala:89-90 with NearestNeighborInterpolator and as examples/DemoHelper/DemoDatasetLoader.scala:58-62 with
 * TriangleMeshInterpolator3D): mean and every basis function of the new point i are the fixed combination
 * sum_k weights[3i+k] * (value at source point vertex_ids[3i+k]); eigenvalues and rank are unchanged, nothing is
 * re-orthonormalised.  Nearest neighbour: ids (nn, nn, nn), weights (1, 0, 0); triangle mesh: the corners of the triangle from
 * gingr_mesh_closest_points and its barycentric weights.  The basis is gathered in HBM from the source model (a complete model
 * of the same context); the result is a model like any other (row shard [row_begin, row_end) of M_new; row_end <= 0 = M_new). */
int gingr_model_new_reference(gingr_ctx *ctx, const gingr_model *src, int64_t M_new, const double *new_ref,
                              const int32_t *vertex_ids, const double *weights, int64_t row_begin, int64_t row_end,
                              gingr_model **out);

/* ---- probabilistic proposal (single shard) ------------------------------------------------
 * update(current, probabilistic = true): the shape proposal is posterior.sample() instead of posterior.mean
 * (G/api/GingrAlgorithm.scala:211).  z[r] are standard-normal draws from the HOST's random generator (the JVM's
 * scalismo.utils.Random there, numpy here); the sample is a + L^-T z with L L^T = I + Q^T L Q, which has exactly the
 * distribution of scalismo's SVD-parameterised posterior sample.  One iteration per call. */
int gingr_fitter_update_cpd_sample_async(gingr_fitter *f, const gingr_cpd_params *p, const double *z);
int gingr_fitter_update_icp_sample_async(gingr_fitter *f, const gingr_icp_params *p, const double *z);
/* posterior(of the fitter's CURRENT state).gp.logpdf(posterior.coefficients(mesh)): the quantity
 * GeneratorWrapperStochastic.logTransitionProbability evaluates (G/api/sampling/generators/GeneratorWrapperStochastic.scala:42-63).
 * mesh_xyz[3*M]; the state is not modified.  rank <= 512.  A failed posterior gives GINGR_ERR_NOT_SPD / _NONFINITE
 * (the reference returns -infinity in that case).  Like the reference's Memoize(computePosterior, 10)
 * (G/api/GingrAlgorithm.scala:68) the fitter remembers which state the correspondences / Gram / right-hand side in its buffers
 * belong to: when gingr_fitter_set_state writes exactly that state again (same coefficients, pose, sigma2, flavour and
 * parameters), the update and these queries reuse them instead of recomputing (single shard; invisible in the results). */
int gingr_fitter_posterior_logpdf_cpd(gingr_fitter *f, const gingr_cpd_params *p, const double *mesh_xyz, double *logpdf);
int gingr_fitter_posterior_logpdf_icp(gingr_fitter *f, const gingr_icp_params *p, const double *mesh_xyz, double *logpdf);

/* ---- per-vertex covariance maps, exact (no sampling) -----------------------------------------------------------------
 * For a right factor W (r x r, row-major; NULL = identity) the 3 x 3 block of vertex i is
 *     C_i = R (Q0_i W)(Q0_i W)^T R^T,   Q0 = U sqrt(lambda),   R = Rotation(euler),
 * positive semi-definite by construction.  W = I is the prior marginal U_i diag(lambda) U_i^T (the map behind the reference's
 * VisualizeGPMMCorrelation); W = L^-T with L L^T = I + G gives a posterior's posterior.gp.cov(pid, pid).
 * gingr_model_marginal_covariance: cov6_out[6 M_local] = {xx, xy, xz, yy, yz, zz} per local point, in the caller's point order.
 * gingr_model_cross_covariance: cov9_out[9 M_local] = R (Q0_i W)(Q0_pid W)^T R^T, full 3 x 3 row-major, for one GLOBAL point id;
 * the block at i = pid is the marginal.  A row shard that does not own pid returns GINGR_ERR_STATE.  Both calls synchronise. */
int gingr_model_marginal_covariance(gingr_ctx *ctx, const gingr_model *model, const double *factor, const double euler[3],
                                    double *cov6_out);
int gingr_model_cross_covariance(gingr_ctx *ctx, const gingr_model *model, const double *factor, const double euler[3], int64_t pid,
                                 double *cov9_out);
/* The same map for the posterior of the fitter's CURRENT state -- what DemoPosteriorVisualizationFemur estimates from thousands of
 * Metropolis-Hastings samples: correspondences, Gram matrix (landmarks included) and the Cholesky factor of I + G of the state,
 * then one pass over the basis with the state's rotation.  cov6_out[6 M].  The posterior is that of model.transform(rigid)
 * (G/api/GingrAlgorithm.scala:297-301): the state's scale is NOT applied.  Single shard only; synchronises; a failed factorisation
 * gives GINGR_ERR_NOT_SPD.  State, retry counter and posterior memo are left as gingr_fitter_posterior_logpdf_* leaves them. */
int gingr_fitter_posterior_covariance_cpd(gingr_fitter *f, const gingr_cpd_params *p, double *cov6_out);
int gingr_fitter_posterior_covariance_icp(gingr_fitter *f, const gingr_icp_params *p, double *cov6_out);
int gingr_fitter_posterior_covariance_icp_surface(gingr_fitter *f, const gingr_icp_params *p, double *cov6_out);

/* ---- the posterior as a model ------------------------------------------------------------------------------------------
 * model.transform(rigid).posterior(obs) as a PointDistributionModel of its own (G/api/GingrAlgorithm.scala:281-302, computePosterior;
 * scalismo DiscreteLowRankGaussianProcess.regression: U_p = U innerU, lambda_p = innerD2 of SVD(D Minv D)): a new, finalized,
 * independent model of the same rank on the same context -- reference R (ref - c) + c + t, mean displacement R (mean + Q0 a), basis
 * U_p sqrt(lambda_p) = R (Q0 L^-T V) with L L^T = I + G and L^-1 diag(lambda) L^-T = V diag(lambda_p) V^T, lambda_p descending.  The
 * basis never leaves the device (one pass over it); reference and mean pass through the host once, they fix the new row order.  No
 * scale.  The observation arguments of gingr_model_posterior mean exactly what they mean in gingr_model_posterior_mean.  Single
 * shard only (GINGR_ERR_STATE otherwise); synchronises; a failed factorisation gives GINGR_ERR_NOT_SPD, a non-finite mean or
 * variance GINGR_ERR_NONFINITE, and *out is NULL then. */
int gingr_model_posterior(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                          const double translation[3], const double *obs_xyz, const double *weight, int32_t n_lm,
                          const int32_t *lm_pid, const double *lm_xyz, const double *lm_cov, gingr_model **out);
/* The same for the posterior of the fitter's CURRENT state (what computePosterior returns for it): correspondences and Gram matrix
 * as gingr_fitter_posterior_covariance_* builds them.  State, retry counter and posterior memo are left as that query leaves them. */
int gingr_fitter_posterior_model_cpd(gingr_fitter *f, const gingr_cpd_params *p, gingr_model **out);
int gingr_fitter_posterior_model_icp(gingr_fitter *f, const gingr_icp_params *p, gingr_model **out);
int gingr_fitter_posterior_model_icp_surface(gingr_fitter *f, const gingr_icp_params *p, gingr_model **out);

/* ---- correspondences given by the caller: the "pairs" flavour (flavour 3) --------------------------------------------------
 * GiNGR's plugin surface is getCorrespondence: State => CorrespondencePairs, getUncertainty: (PointId, State) =>
 * MultivariateNormalDistribution and updateSigma2 (G/api/GingrAlgorithm.scala:65-74,256-258; registration/config/Template.scala is
 * the skeleton).  With this flavour the host supplies the first two as lists and the device runs everything `update` does around
 * them: the posterior, both coefficient projections, step length, global transform, the Try failure rules and the retry counter,
 * the fit refresh, the sampled proposal, the transition density, the covariance maps and the posterior as a model.
 *
 * gingr_fitter_set_pairs: K >= 0 isotropic pairs (pid[k], xyz[3k..3k+2], var[k]), host arrays.  Pids are GLOBAL ids in the
 * caller's point order, in any order, repeated or not, covering any subset of the vertices.  They are consolidated ONCE, here,
 * into one observation per vertex -- k isotropic observations of one point are one observation of their precision-weighted mean:
 *     weight_i = sum_k 1 / var_k,     obs_i = (sum_k x_k / var_k) / weight_i      (both sums in ascending pair position),
 * weight_i = 0 (and obs_i = 0) for a vertex without pairs -- by a stable radix sort of the device rows (only the bits a row can
 * have) and one gather thread per local vertex.  A row shard is given the WHOLE list and keeps the pairs of its own rows.  The
 * working memory belongs to the fitter and is reused while K does not grow.  K = 0 clears the list.
 * gingr_fitter_set_pairs_cov: a second, independent list with a full 3 x 3 covariance per pair (row-major).  It is summed into G
 * and the right-hand side by the landmark pass, in ONE launch over "covariance pairs first, then the landmarks"; that pass costs
 * O(K r^2) -- it is meant for tens to hundreds of pairs, NOT for one pair per vertex: that is gingr_fitter_set_pairs_cov_dense.
 * gingr_fitter_set_pairs_cov_dense: a third, independent list with a full 3 x 3 covariance per pair (row-major, world frame), for
 * covariances at mesh scale -- one pair per vertex, point-to-plane ICP.  The contract of gingr_fitter_set_pairs (global pids in any
 * order, repeated or not, any subset; host arrays; K <= 1 << 24; a row shard is given the WHOLE list; working memory of the fitter's,
 * reused while K does not grow; K = 0 clears the list).  The pairs are consolidated ONCE, here, on the device -- the same stable
 * radix sort, one gather thread per local vertex -- into one observation per vertex:
 *     Lambda_i = sum_k Sigma_k^-1 (six doubles: xx, xy, xz, yy, yz, zz),   xbar_i = Lambda_i^-1 sum_k Sigma_k^-1 x_k
 * (both sums in ascending pair position; a vertex with exactly one pair keeps that pair's point bit for bit; without pairs
 * Lambda_i = 0 and xbar_i = 0).  Every update then adds, with the state's R, c, t and m_i = ref_i - c + mean_i,
 *     G += sum_i Q_i^T W_i Q_i,   rhs += sum_i Q_i^T W_i v_i,     W_i = R^T Lambda_i R,   v_i = R^T (xbar_i - c - t) - m_i
 * by a float64-MFMA pass over the basis (row slabs, partials combined in a fixed order, no atomics: two runs give the same bits),
 * behind the isotropic pass and in front of the landmark pass, before the exchange segment is handed out.  The three lists are
 * independent: a vertex may be in all of them and their contributions add.  With the dense list empty nothing of it is launched.
 * Covered: gingr_fitter_update_pairs_async, _pairs_phase_async, _update_pairs_sample_async, _posterior_logpdf_pairs,
 * _posterior_covariance_pairs, _posterior_model_pairs, and gingr_fitter_update_sharded_async / _posterior_logpdf_sharded with flavour 3.
 * NOT covered, as the flavour itself: gingr_fitter_mh_step, the gingr_group_* and RCCL entry points.
 * gingr_fitter_get_pair_precisions (synchronises): the consolidated planes of the dense list, obs_xyz[3 M_local] / prec6[6 M_local]
 * (six doubles per vertex) in the caller's point order; either may be NULL.
 * A vertex that a landmark overrides (gingr_fitter_set_landmarks) loses its isotropic, its covariance and its dense covariance pairs
 * (GingrAlgorithm.scala:288-296); the three calls and gingr_fitter_set_landmarks may come in any order.
 * All three calls synchronise and forget the posterior memo (the same state with other pairs is another posterior).  A pid outside
 * [0, M_total) is GINGR_ERR_BAD_ARGUMENT (nothing is changed).  VALUES are not validated; they follow the Try rules of `update`, as
 * the ICP flavours' do: a non-finite point, variance or covariance fails the posterior on the device (state unchanged at
 * iteration 0, ModelFlexibilityError later, a retry when sampled); var = +inf is weight 0, a dropped pair.
 * gingr_fitter_get_pair_observations (synchronises): the consolidated planes, obs_xyz[3 M_local] / weight[M_local] in the caller's
 * point order; either may be NULL.
 *
 * gingr_fitter_update_pairs_async: n_iterations updates + fit refresh with the pairs as they stand.  sigma2 is LEFT AS IT IS, the
 * trait's default updateSigma2 (GingrAlgorithm.scala:256-258); a host with a rule of its own applies it between updates with
 * gingr_fitter_set_sigma2: asynchronous, writes sigma2 of the device state only (no fit recomputation), forgets the memo.
 * _sample / _logpdf / _covariance / _model: the contracts of their _icp siblings, memo reuse included (exactly the same state set
 * again, pairs and landmarks untouched in between).  Without pairs and landmarks G = 0 and rhs = 0: the posterior mean is the
 * prior mean and the update proceeds; with landmarks only it is a landmark registration.  The general weighted Gram pass and the
 * Cholesky solve are always taken: the uniform-weight shortcuts of the ICP flavours do not apply.  A target must be set
 * (gingr_fitter_set_target sizes the exchange buffers), though this flavour never reads it.
 * gingr_fitter_update_sharded_async / gingr_fitter_posterior_logpdf_sharded accept flavour = 3 (cp and ip unused): no segment-0
 * exchange.  NOT covered: gingr_fitter_mh_step (the correspondences come from the host, a step cannot be fused; call by call works),
 * the gingr_group_* and RCCL entry points. */
int gingr_fitter_set_pairs(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *var);
int gingr_fitter_set_pairs_cov(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *cov);
int gingr_fitter_set_pairs_cov_dense(gingr_fitter *f, int64_t K, const int32_t *pid, const double *xyz, const double *cov);
int gingr_fitter_get_pair_observations(gingr_fitter *f, double *obs_xyz, double *weight);
int gingr_fitter_get_pair_precisions(gingr_fitter *f, double *obs_xyz, double *prec6);
int gingr_fitter_set_sigma2(gingr_fitter *f, double sigma2);
int gingr_fitter_update_pairs_async(gingr_fitter *f, int32_t n_iterations);
int gingr_fitter_pairs_phase_async(gingr_fitter *f, int32_t phase);
int gingr_fitter_update_pairs_sample_async(gingr_fitter *f, const double *z);
int gingr_fitter_posterior_logpdf_pairs(gingr_fitter *f, const double *mesh_xyz, double *logpdf);
int gingr_fitter_posterior_covariance_pairs(gingr_fitter *f, double *cov6_out);
int gingr_fitter_posterior_model_pairs(gingr_fitter *f, gingr_model **out);

/* ---- point-to-plane ICP on the surfaces, its correspondence made on the device ---------------------------------------------
 * The pairs flavour with the dense list filled by the fitter itself: per model vertex the closest point of the target SURFACE and a
 * covariance that is tight along the target's face normal and loose across it.  With r = tangent_over_normal, v_n = sigma2 of the
 * device state, v_t = r sigma2 and n_i the unit normal of the target triangle the closest point of vertex i lies on (as
 * gingr_fitter_set_meshes stored it: (b - a) x (c - a), normalised), every vertex gets
 *     Lambda_i = (1 / v_t) I + (1 / v_n - 1 / v_t) n_i n_i^T   (six doubles: xx, xy, xz, yy, yz, zz),     xbar_i = closest point,
 * the closed-form inverse of Sigma_i = v_t I + (v_n - v_t) n_i n_i^T -- nothing is inverted numerically, xbar_i is the scan's point bit
 * for bit, and r = 1 gives (1 / sigma2) I exactly: point-to-point ICP against the surface.  A stored normal that is zero or non-finite
 * (a degenerate target triangle) gives (1 / v_t) I.  reject = 1 applies the three rejection rules of the surface flavour (boundary
 * vertex, opposing normals, self-intersection: gingr_fitter_update_icp_surface_async); a rejected vertex has Lambda_i = 0, xbar_i = 0,
 * "no observation".  reject = 0 observes every vertex.  A vertex that a landmark overrides loses its plane, as every dense pair does.
 *
 * gingr_fitter_set_pairs_plane_async: the forward TriangularClosestPoint correspondence of the CURRENT device state's fit against the
 * target -- the launches of the surface flavour, warm starts and triangle grid included -- then one kernel, one thread per local
 * vertex, that writes the planes above.  Asynchronous on the context's stream: no transfer, no synchronisation.  The result BECOMES
 * the dense list: it replaces what gingr_fitter_set_pairs_cov_dense put there, a later gingr_fitter_set_pairs_cov_dense replaces it in
 * turn, K = 0 there clears it.  The isotropic list, the covariance list and the landmarks stay independent and keep adding, as
 * documented for the dense list.  Forgets the posterior memo.  Afterwards gingr_fitter_get_surface_correspondence returns the closest
 * points and the 0/1 weights that were used (all 1 with reject = 0), gingr_fitter_get_pair_precisions the planes; every entry point
 * listed as covered under the dense list reads them -- the sampled update, the transition density, the covariance maps and the
 * posterior model of a point-to-plane state are the _pairs queries behind this call.
 * gingr_fitter_update_plane_async: n_iterations times { the call above; one update as gingr_fitter_update_pairs_async(f, 1) runs it;
 * ICP's schedule  sigma2 <- max(sigma2 - (initial_sigma - end_sigma) / max_iterations, end_sigma)  on the device }.  The schedule
 * is applied only to an update that committed, exactly where the ICP flavours apply it; a failed or stopped state is left as it is
 * and the stop rule (gingr_fitter_set_stop_threshold) compares sigma2 before and after the schedule, as it does for ICP.
 * Asynchronous, nothing is synchronised between iterations; two runs give the same bits, and n iterations in one call give the bits
 * of n calls of one.
 * Refused with nothing changed -- GINGR_ERR_STATE: no target or state set; no meshes set; a row shard (single shard only); surface
 * method 1 or the reversed direction set.  GINGR_ERR_BAD_ARGUMENT: null params; tangent_over_normal < 1 or non-finite; reject not 0
 * or 1; n_iterations < 1; schedule null or max_iterations < 1.
 * NOT covered, as the pairs flavour itself: gingr_fitter_mh_step, the gingr_group_* and RCCL entry points. */
typedef struct gingr_plane_params {
    double tangent_over_normal;  /* >= 1, finite; 1 = isotropic: point-to-point against the surface */
    int32_t reject;              /* 0: every vertex observed; 1: the three rejection rules of the surface flavour */
} gingr_plane_params;
int gingr_fitter_set_pairs_plane_async(gingr_fitter *f, const gingr_plane_params *p);
int gingr_fitter_update_plane_async(gingr_fitter *f, const gingr_plane_params *p, const gingr_icp_params *schedule,
                                    int32_t n_iterations);

/* ---- k nearest neighbours of a cloud within itself, and the normals of those neighbourhoods (cloud_knn.hip) -----------------
 * gingr_cloud_knn: for every point j of xyz [N][3] the k points of the cloud with the smallest (d2, index), d2 = dx*dx + dy*dy + dz*dz
 * of x_i - x_j with separately rounded products and sums (the bits of that expression in float64 on a CPU), ties to the lowest index.
 * idx [N][k] / d2 [N][k] (nullable): row j sorted ascending by (d2, index).  The point itself is a candidate: the first entry is j, or
 * a lower-indexed duplicate of it.  3 <= k <= 64 and k <= N (N <= 2^27), else GINGR_ERR_BAD_ARGUMENT; a non-finite coordinate is
 * GINGR_ERR_NONFINITE and nothing is computed.  A uniform grid over the cloud is built on the device per call; a query the grid cannot
 * certify (a far outlier, a crowded row of cells) is answered by a scan of the whole cloud -- the same lists either way.  info
 * (nullable): the grid's cell size and dimensions and the number of queries that took the scan.  Two calls give the same bits.
 * Synchronises.
 * gingr_cloud_normals: a normal per point from its k-neighbourhood -- THIS PACKAGE'S DEFINITION, not a toolkit's.  With the list of
 * gingr_cloud_knn in its order: q_i = x_i - x_j (taken first: the result does not depend on where the cloud lies, up to rounding),
 * m = sum q_i / k, C = sum (q_i - m)(q_i - m)^T / k in float64 in list order, lam0 <= lam1 <= lam2 its eigenvalues.  normals [N][3]:
 * the unit eigenvector of lam0; the ZERO vector when lam1 - lam0 <= 2^-26 lam2 (coincident points, a line, an isotropic blob: the
 * direction has no correct digit).  Sign: the component of largest magnitude is positive, the lowest axis on ties; with a viewpoint v
 * [3] (nullable) the normal is turned so that n . (v - x_j) >= 0.  variation [N] (nullable): lam0 / (lam0 + lam1 + lam2), Pauly's surface
 * variation, 0 on a plane and 0 when the trace is 0.  Arguments, errors and info as gingr_cloud_knn; a non-finite viewpoint is
 * GINGR_ERR_NONFINITE.  Synchronises. */
typedef struct gingr_cloud_knn_info {
    double cell_size;  /* edge of a grid cell */
    int32_t grid[3];   /* cells per axis */
    int32_t flagged;   /* queries the grid did not certify: answered by the scan of the whole cloud */
} gingr_cloud_knn_info;
int gingr_cloud_knn(gingr_ctx *ctx, int64_t N, const double *xyz, int32_t k, int32_t *idx, double *d2, gingr_cloud_knn_info *info);
int gingr_cloud_normals(gingr_ctx *ctx, int64_t N, const double *xyz, int32_t k, const double *viewpoint, double *normals, double *variation,
                        gingr_cloud_knn_info *info);

/* ---- point-to-plane ICP against a point cloud: a normal per target point instead of target triangles ------------------------
 * The planes of gingr_fitter_set_pairs_plane_async with the nearest target POINT in place of the closest surface point and that
 * point's stored normal in place of the face normal: xbar_i = the nearest target point of vertex i bit for bit (the forward search of
 * gingr_fitter_update_icp_async, grid and warm start as they stand), Lambda_i = (1 / v_t) I + (1 / v_n - 1 / v_t) n n^T by the same
 * arithmetic, a zero normal gives (1 / v_t) I, tangent_over_normal = 1 gives (1 / sigma2) I exactly: point-to-point ICP against the
 * cloud.  max_distance > 0: a vertex whose squared distance to its nearest target point exceeds max_distance * max_distance is not
 * observed (Lambda_i = 0, xbar_i = 0).  No meshes are needed.
 * Target normals, [N][3] in the order of the target set last; a new gingr_fitter_set_target drops them.
 *   gingr_fitter_set_target_normals       the caller's (a scanner's own): each is normalised on upload -- one whose squared length is
 *                                         within 2^-48 of 1 is taken as it is, zero stays zero; non-finite: GINGR_ERR_NONFINITE
 *   gingr_fitter_estimate_target_normals  gingr_cloud_normals (k, viewpoint, info) on the target as it lies on the device: no download,
 *                                         no upload, the same bits
 *   gingr_fitter_get_target_normals       what the fitter holds (GINGR_ERR_STATE without normals)
 * gingr_fitter_set_pairs_plane_cloud_async / gingr_fitter_update_plane_cloud_async: as the two surface entry points above -- the result
 * becomes the dense list, the loop applies ICP's schedule on the device, n iterations in one call give the bits of n calls of one, a
 * landmark overrides a vertex.  gingr_fitter_get_icp_idx reports the matches that were used, gingr_fitter_get_pair_precisions the planes;
 * the sampled update, transition density, posterior covariance and posterior model are the _pairs queries.
 * Refused with nothing changed -- GINGR_ERR_STATE: no target or state set; no target normals; a row shard (single shard, forward
 * direction only).  GINGR_ERR_BAD_ARGUMENT: null params; tangent_over_normal < 1 or non-finite; max_distance NaN; n_iterations < 1;
 * schedule null or max_iterations < 1. */
typedef struct gingr_plane_cloud_params {
    double tangent_over_normal;  /* >= 1, finite; 1 = point-to-point against the cloud */
    double max_distance;         /* <= 0: no rejection; else a vertex farther than this from its nearest target point is not observed */
} gingr_plane_cloud_params;
int gingr_fitter_set_target_normals(gingr_fitter *f, const double *normals);
int gingr_fitter_estimate_target_normals(gingr_fitter *f, int32_t k, const double *viewpoint, gingr_cloud_knn_info *info);
int gingr_fitter_get_target_normals(gingr_fitter *f, double *normals);
int gingr_fitter_set_pairs_plane_cloud_async(gingr_fitter *f, const gingr_plane_cloud_params *p);
int gingr_fitter_update_plane_cloud_async(gingr_fitter *f, const gingr_plane_cloud_params *p, const gingr_icp_params *schedule,
                                          int32_t n_iterations);

/* ---- robust point-to-plane ICP: M-estimator weights as a variance per vertex, the scale from a median on the device ----------
 * THIS PACKAGE'S DEFINITION.  For every vertex i the correspondence observed (after `reject` on the surface route, after max_distance on
 * the cloud route), with d_i = fit vertex - observed point, n_i the unit normal of its plane and r = tangent_over_normal:
 *   residual   s_i = e_n^2 + max(|d_i|^2 - e_n^2, 0) / r,  e_n = n_i . d_i   -- sigma2 d_i^T Lambda_i d_i, the squared distance in the
 *              metric of the observation; r = 1: |d_i|^2 exactly; a zero or non-finite normal: |d_i|^2 / r, as the planes treat it
 *   scale      c = scale (scale_mode 0), or c = scale * 1.4826 * sqrt(s_(k)) (scale_mode 1; scale is the tuning constant): s_(k) the k-th
 *              smallest s_i of the n observed vertices, k = (n - 1) / 2 -- the lower median, an element of the data, found exactly by a
 *              radix selection over the bit patterns (robust_select.hip).  Then c = max(c, min_scale).  n = 0 or c = 0: u_i = 1
 *   inflation  Cauchy u = 1 + s / c^2;  Huber u = max(1, sqrt(s) / c);  Tukey: s >= c^2 removes the vertex (Lambda_i = 0, xbar_i = 0),
 *              else u = 1 / (1 - s / c^2)^2.  The vertex's plane is the one above at v_n = sigma2 u_i.
 * A vertex Tukey removes still counts in the median: the scale never depends on the weights.  The usual 95 % tunings with the median
 * scale: Cauchy 2.385, Huber 1.345, Tukey 4.685.
 * gingr_fitter_set_plane_robust: a persistent setting of the fitter; NULL or loss 0 turns it off (the default).  While it is on, the
 * four plane entry points -- gingr_fitter_set_pairs_plane_async, gingr_fitter_update_plane_async, gingr_fitter_set_pairs_plane_cloud_async,
 * gingr_fitter_update_plane_cloud_async -- run, behind the correspondence, a residual kernel, the selection (a handful of short
 * launches, kernel boundaries the only synchronisation) and the robust variant of their plane kernel; still no transfer and no
 * synchronisation, two runs give the same bits and n iterations in one call give the bits of n calls of one.  While it is off nothing
 * of this is launched and every result keeps its bits.  Forgets the posterior memo.  Refused with nothing changed --
 * GINGR_ERR_BAD_ARGUMENT: loss outside 0..3, scale_mode outside 0..1, scale or min_scale non-finite, scale <= 0, min_scale < 0;
 * GINGR_ERR_STATE: a row shard.
 * gingr_fitter_get_plane_robust (every pointer nullable): s [M] and u [M] in the caller's point order (u = 0: not observed, s = 0
 * there), *selected = s_(k) (0 for n = 0), *c, *n_observed, of the last robust refresh.  Synchronises.  GINGR_ERR_STATE before the
 * first robust refresh under the current setting.
 * The sampled update, the transition density, the posterior covariance and the posterior model stay the pairs flavour's and take the
 * robust planes as they are.  NOT covered: gingr_fitter_mh_step, the gingr_group_* and RCCL entry points, the JVM binding.
 * gingr_order_statistic: the selection as a stateless operator -- *out = the k-th smallest (0-based) of values [n], host arrays, the
 * element itself bit for bit (-0 counts as +0).  +inf is a value like any other.  A negative or NaN value: GINGR_ERR_NONFINITE;
 * n < 1, n >= 2^31 or k outside [0, n): GINGR_ERR_BAD_ARGUMENT.  Two calls give the same bits.  Synchronises. */
typedef struct gingr_robust_params {
    int32_t loss;        /* 0 none, 1 Cauchy, 2 Huber, 3 Tukey */
    int32_t scale_mode;  /* 0: fixed, scale = c > 0;  1: median, scale = the tuning constant > 0 */
    double scale;
    double min_scale;    /* >= 0: a floor under c */
} gingr_robust_params;
int gingr_fitter_set_plane_robust(gingr_fitter *f, const gingr_robust_params *p);
int gingr_fitter_get_plane_robust(gingr_fitter *f, double *s, double *u, double *selected, double *c, int64_t *n_observed);
int gingr_order_statistic(gingr_ctx *ctx, int64_t n, const double *values, int64_t k, double *out);

/* ---- a PCA model from shapes in correspondence ----------------------------------------------------------------------------
 * What DataCollection.gpa(...) followed by PointDistributionModel.createUsingPCA(...) gives a scalismo user, built on the device: a
 * new, finalized, single-shard model on this context.  ref_xyz [3 M]: the reference; shapes_xyz [n_shapes][3 M]: the shapes, point
 * for point on the reference's vertices, 2 <= n_shapes <= 512.
 * alignment: 0 none; 1 every shape rigidly onto the reference (Kabsch: centroids, 3 x 3 cross-covariance, SVD, last singular vector
 * flipped for a negative determinant, no scale); 2 generalised Procrustes -- from target = reference, sweeps of "align every shape to
 * the target, target := mean of the aligned shapes", at most gpa_max_iterations of them (<= 0: 3), ended early when the RMS distance
 * per point between successive targets falls below gpa_tolerance (1e-5 is the customary value).  The model's reference is the final
 * target in mode 2 and ref_xyz otherwise.
 * Model: mean displacement = mean shape - reference; with Xc = [X_i - mean] / sqrt(n - 1) and Xc^T Xc = V diag(lambda) V^T, the leading
 * k components with lambda_j > relative_tolerance lambda_1 are kept, k <= min(n - 1, max_rank or 512): variance lambda[:k], basis
 * U sqrt(lambda) = Xc V[:, :k].  relative_tolerance: 1e-10 is this library's customary value; the cutoff constant of scalismo's own
 * createUsingPCA is not pinned by anything in reach.
 * info (nullable) reports the rank, the Procrustes sweeps run and the last target change, and the total / kept variance (sums of
 * eigenvalues).  Two calls with the same input give the same bits.  Synchronises.  GINGR_ERR_BAD_ARGUMENT: n_shapes outside 2..512,
 * M < 1, alignment outside 0..2, all shapes identical (rank 0); GINGR_ERR_NONFINITE: non-finite input; *out is NULL then. */
typedef struct {
    int32_t rank;
    int32_t gpa_sweeps;
    double gpa_last_change;
    double total_variance;
    double kept_variance;
} gingr_pca_info;
int gingr_model_from_shapes(gingr_ctx *ctx, int64_t M, int32_t n_shapes, const double *ref_xyz, const double *shapes_xyz,
                            int32_t alignment, int32_t gpa_max_iterations, double gpa_tolerance, double relative_tolerance,
                            int32_t max_rank, gingr_model **out, gingr_pca_info *info);

/* ---- a model augmented with a second one ----------------------------------------------------------------------------------
 * What PointDistributionModel.augmentModel(pcaModel, biasModel) gives a scalismo user, with both bases staying on the device: a new,
 * finalized, independent model on the same reference with mean displacement mean_a + mean_b and covariance Q_a Q_a^T + Q_b Q_b^T
 * (Q = U sqrt(lambda)), re-diagonalised.  The sum of the means and the cutoff below are this library's definition; nothing in reach
 * pins scalismo's own.  a, b: complete (single-shard, finalized) models of this context on references that are equal coordinate for
 * coordinate, ra + rb <= 512 columns together (truncate first otherwise); b may be a itself.
 * With G = [Q_a | Q_b]^T [Q_a | Q_b] = V diag(lambda) V^T (lambda descending; the diagonal blocks are the models' resident moments, used
 * as stored, the cross block Q_a^T Q_b is one pass over the two bases) the leading k eigenvalues with lambda_j > relative_tolerance
 * lambda_1 and > 0 are kept, k <= max_rank when max_rank > 0 and k <= 512: variance lambda[:k], basis U sqrt(lambda) =
 * Q_a V[:ra, :k] + Q_b V[ra:, :k], rows in the order of ref + mean_a + mean_b.  relative_tolerance: 1e-10 is this library's customary value.
 * Only reference and mean pass through the host.  a and b are not changed.  Two calls with the same input give the same bits.
 * Synchronises.  GINGR_ERR_BAD_ARGUMENT (the text names the cause): a null argument, a model of another context, a row shard or a
 * model that is not finalized, different point counts, references that differ (the text names the first differing point), more than
 * 512 columns, a negative tolerance or max_rank, no eigenvalue above the cutoff (rank 0); GINGR_ERR_NONFINITE: a non-finite Gram
 * matrix or eigenvalue; *out is NULL then and the context stays usable. */
typedef struct gingr_augment_info {
    int32_t columns;        /* ra + rb */
    int32_t rank;           /* rank of the returned model */
    double total_variance;  /* sum of all eigenvalues = trace S_a + trace S_b */
    double kept_variance;
} gingr_augment_info;
int gingr_model_augment(gingr_ctx *ctx, const gingr_model *a, const gingr_model *b, double relative_tolerance,
                        int32_t max_rank, gingr_model **out, gingr_augment_info *info /* may be NULL */);

/* ---- a model localized: its covariance tapered by a Gaussian of the distance on the reference --------------------------------------
 * The localized statistical shape model of Luethi et al. (Gaussian Process Morphable Models): with Q = U sqrt(lambda) of the source
 * (3M x r, rows 3i + d) and x_1 .. x_M its reference,
 *     K[(i,a),(j,b)] = g(x_i, x_j) sum_k Q[3i+a, k] Q[3j+b, k],    g(x, y) = exp(-|x - y|^2 / sigma^2)
 * -- every vertex keeps its own variance (g(x, x) = 1), correlations survive nearby and are removed far away; the rank rises from r to
 * hundreds.  g is taken over the reference (not reference + mean) and is the GPMM builder's Gaussian of scaling 1, bit for bit.  K is
 * positive semi-definite (Schur product) with trace K = trace Q Q^T.  K ~ L L^T by the builder's pivoted Cholesky over the 3M (point,
 * coordinate) entries (its pivot, tie and stop rules) until the residual trace is below relative_tolerance trace K, or 512 columns
 * are computed (the generic factor's ceiling), or no positive residual is left; reaching the ceiling first is not an error, info says
 * so.  Then L^T L = V diag(lambda') V^T, basis L V; the leading components with lambda'_j > 1e-12 lambda'_1 and > 0 are kept, at most
 * max_rank (0: 512) and at most 512.  The 1e-12 is the noise floor of the Gram route, not a modelling knob: relative_tolerance and
 * max_rank are.  The result is a new, independent, finalized model on the same reference with the same mean; the source is not
 * changed.  Only reference and mean pass through the host.  Float64, a complete (single-shard) model.  Every sum has a fixed order: two
 * calls with the same input give the same bits.  Synchronises.
 * GINGR_ERR_BAD_ARGUMENT (the text contains "model_localize" and names the cause): a null argument, a model of another context, a row
 * shard or a model that is not finalized, sigma not positive and finite, relative_tolerance outside [0, 1) or NaN, a negative
 * max_rank, rank 0 after the cutoff; GINGR_ERR_NONFINITE: a non-finite trace or eigenvalue.  On any error *out is NULL, *info is
 * zeroed and the context stays usable. */
typedef struct gingr_localize_info {
    int32_t columns;            /* factor columns computed */
    int32_t rank;               /* rank of the returned model */
    int32_t tolerance_reached;  /* 0: stopped at the 512-column ceiling above the tolerance */
    double residual_fraction;   /* residual trace / trace K after the last column */
    double total_variance;      /* trace K */
    double kept_variance;       /* sum of the kept eigenvalues */
} gingr_localize_info;
int gingr_model_localize(gingr_ctx *ctx, const gingr_model *model, double sigma, double relative_tolerance,
                         int32_t max_rank, gingr_model **out, gingr_localize_info *info /* may be NULL */);

/* ---- model metrics: many instances, many projections, many samples against many shapes ------------------------------------------
 * What the shape-model literature (and scalismo's ModelMetrics) measures a model by, batched on the device.  What is not scalismo's is
 * this library's definition: nothing in reach pins scalismo's own, and scalismo measures against the closest surface point, whereas
 * every distance of these three entries is vertex to corresponding vertex (the closest-surface-point measure: the next section).  model: a complete (single-shard), finalized model of this context -- a row
 * shard or a model that is not finalized is GINGR_ERR_STATE.  Shapes are host arrays of 3 M doubles each, one after the other,
 * interleaved xyz in the caller's point order (the layout of gingr_model_from_shapes).  ranks: n_ranks <= 16 strictly increasing values
 * 1 <= k <= rank.  Bad counts or ranks and null arguments are GINGR_ERR_BAD_ARGUMENT (the text names the cause); a non-finite
 * coordinate or coefficient is GINGR_ERR_NONFINITE (the text names the shape or vector) and nothing is computed.  Single precision
 * nowhere; every sum in a fixed order, no float atomics: two calls with the same input give the same bits.  All three synchronise.
 *
 * gingr_model_instances: out_xyz [n][3 M] = ref + mean + Q0 alpha_i for the n >= 1 coefficient vectors alphas [n][rank], no pose: one
 *   pass over the basis on the matrix pipe per block of 512 vectors.
 * gingr_model_generalization: for the 1 <= n <= 512 shapes and every k in ranks, avg [n_ranks][n] the mean and max [n_ranks][n] the
 *   largest vertex distance between the shape and its projection onto the k leading components; coeffs (may be NULL)
 *   [n_ranks][n][rank] the projection's coefficients, zero from entry k on.  The projection is the existing rule: what
 *   gingr_model_truncate(k), gingr_model_coefficients and gingr_model_instance return at the identity pose -- the regression with
 *   noise 1e-5, alpha_k = (S_k / 1e-5 + I)^-1 Q_k^T (x - ref - mean) / 1e-5 with Q_k the k leading columns of U sqrt(lambda) and
 *   S_k = Q_k^T Q_k.  A shape that is an instance of the model therefore comes back at a distance of the order of that ridge's bias,
 *   not 0.  GINGR_ERR_NOT_SPD: S / 1e-5 + I could not be factored.
 * gingr_model_specificity: the sample (i, k) is the instance of alphas [n_samples][rank] row i with the entries from k on set to
 *   zero; min_avg [n_ranks][n_samples] is its smallest mean vertex distance to one of the 1 <= n_train <= 512 training shapes and
 *   argmin [n_ranks][n_samples] that shape's index, the lowest index on an exact tie.  The coefficients are the caller's: the library
 *   draws nothing.  n_samples >= 1, in blocks of 512. */
int gingr_model_instances(gingr_ctx *ctx, const gingr_model *model, int64_t n, const double *alphas, double *out_xyz);
int gingr_model_generalization(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, int32_t n_ranks,
                               const int32_t *ranks, double *coeffs /* may be NULL */, double *avg, double *max);
int gingr_model_specificity(gingr_ctx *ctx, const gingr_model *model, int32_t n_train, const double *train_xyz, int64_t n_samples,
                            const double *alphas, int32_t n_ranks, const int32_t *ranks, double *min_avg, int32_t *argmin);

/* ---- surface-distance model metrics: many point sets against the surfaces of many meshes of one triangulation ---------------------
 * The measure scalismo's ModelMetrics and the shape-model literature use (MeshMetrics.avgDistance) beside the vertex-to-vertex one above.
 * Definition (this library's: scalismo's source is not in reach, so the DIRECTION is ours): the surface distance of a model-side mesh A
 * -- a projection or a sample -- to a data shape B with the same triangles is, for every vertex p of A, d(p) = |p -
 * closestPointOnSurface_B(p)|; avg is the mean over the M vertices, max the largest d(p).  Model side -> data surface: what
 * gingr_mesh_distance_stats(A, B, triangles) gives as out[0] / out[2] and out[1].  No boundary-aware variant, no likelihood term.
 * All three are float64, synchronise, sum in a fixed order without float atomics: two calls with the same input give the same bits.
 *
 * gingr_mesh_set_distances: n_sets query sets of n_points points each (sets_xyz [n_sets][3 n_points]) against n_meshes meshes of
 *   n_vertices vertices each (meshes_xyz [n_meshes][3 n_vertices]) that share `triangles` [3 n_triangles]; host arrays, interleaved xyz.
 *   pairing 0: every set against every mesh, avg and max are [n_sets][n_meshes]; pairing 1: set c against mesh c % n_meshes, avg and max
 *   are [n_sets].  corresponding != 0 needs n_points == n_vertices and declares that point k of a set lies near vertex k of the mesh:
 *   a HINT that seeds the search of point k with a triangle at vertex k and never changes a bit of a result; with 0 the search starts
 *   cold.  Points need not be near anything.  A vertex of no triangle is legal (its point starts cold), and so are degenerate triangles,
 *   as in gingr_mesh_closest_points.  The squared distance behind every d(p) has the bits gingr_mesh_closest_points returns, max the bits
 *   of gingr_mesh_distance_stats' out[1]; avg differs from out[0] / out[2] by the order of the sum alone.
 *   Route: the k-d order of the first mesh's vertices and triangle centroids serves every mesh (correct for any meshes: every mesh has
 *   its own tile boxes, the pruning only gets looser when the meshes differ much); every mesh is resident at once, the sets pass in
 *   blocks of 512.
 * gingr_model_generalization_surface / gingr_model_specificity_surface: the arguments, limits (512 shapes, 16 ranks, samples in blocks
 *   of 512), coefficient rule, tie rule (lowest index) and error codes of gingr_model_generalization / gingr_model_specificity, with the
 *   shapes' shared `triangles` (vertex ids in the caller's point order); only the distance differs: projection (i, k) against the surface
 *   of shape i, sample (s, k) against the surface of every training shape.  coeffs has the bits of gingr_model_generalization's.
 * Errors: GINGR_ERR_BAD_ARGUMENT (the text names the cause) for a null argument, a count < 1, a vertex id of a triangle out of range,
 *   corresponding with n_points != n_vertices, a pairing other than 0 or 1, more than 2^26 triangles, and a working set (every mesh, a
 *   block of sets) that does not fit the device's free memory -- the text names the size; GINGR_ERR_NONFINITE (the text names the set,
 *   mesh, shape or vector) for a non-finite coordinate, nothing is computed; GINGR_ERR_STATE for a row shard or a model that is not
 *   finalized.  Nothing is written and the context stays usable after each of them. */
int gingr_mesh_set_distances(gingr_ctx *ctx, int64_t n_points, int64_t n_sets, const double *sets_xyz, int64_t n_vertices, int64_t n_meshes,
                             const double *meshes_xyz, int64_t n_triangles, const int32_t *triangles, int32_t pairing, int32_t corresponding,
                             double *avg, double *max);
int gingr_model_generalization_surface(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, int64_t n_triangles,
                                       const int32_t *triangles, int32_t n_ranks, const int32_t *ranks, double *coeffs /* may be NULL */,
                                       double *avg, double *max);
int gingr_model_specificity_surface(gingr_ctx *ctx, const gingr_model *model, int32_t n_train, const double *train_xyz, int64_t n_triangles,
                                    const int32_t *triangles, int64_t n_samples, const double *alphas, int32_t n_ranks, const int32_t *ranks,
                                    double *min_avg, int32_t *argmin);

/* ---- leave-one-out generalization of a PCA shape model --------------------------------------------------------------------------
 * The measurement the literature defines generalization by (scalismo: Crossvalidation.leaveOneOutCrossvalidation with the
 * generalization measure): for every shape i the model of the other n - 1 shapes, shape i projected onto it.  shapes_xyz: n_shapes
 * host arrays of 3 M doubles, the layout of gingr_model_from_shapes, 3 <= n_shapes <= 512, taken as already aligned; ranks: n_ranks <= 16
 * strictly increasing values 1 <= k <= n_shapes - 2.  No reference enters.
 * Definition, for every i: the fold model is what gingr_model_from_shapes(alignment 0, relative_tolerance, max_rank 0) builds from the
 * other shapes -- mean of the n - 1, covariance divisor n - 2, the components with lambda_j > relative_tolerance lambda_1 and > 0 kept,
 * fold_rank [n_shapes] of them (<= n_shapes - 2); the projection of shape i onto k components is that of gingr_model_generalization (the
 * regression with noise 1e-5) with k' = min(k, fold_rank[i]); avg [n_ranks][n_shapes] is the mean and max [n_ranks][n_shapes] the largest
 * vertex-to-corresponding-vertex distance between shape i and that projection.  A fold whose other shapes are all identical -- its total
 * variance lies within the rounding of the Gram entries it is formed from -- is no error: fold_rank[i] = 0, the projection is the
 * fold's mean.
 * Route: nothing of mesh size is repeated per fold.  The shapes centred on the mean of all n and their Gram matrix are formed once;
 * every fold's Gram matrix is a rank-two correction of it, decomposed (with the mean-eigenvalue shift of gingr_model_from_shapes) side
 * by side with the other folds, one workgroup each, up to n_shapes = 193; from 194 on the folds go through the block kernel three at a
 * time (correct; no speed is promised there).  Every fold's error field is a combination of the centred shapes with weights worked
 * out in n-space, formed on float64 MFMA and measured without being stored.  Float64 throughout, every sum in a fixed order, no float
 * atomics: two calls with the same input give the same bits.  Synchronises.
 * GINGR_ERR_BAD_ARGUMENT (the text contains "pca_leave_one_out" and names the cause): a null argument, n_shapes outside 3..512, M < 1,
 * n_ranks outside 1..16, a rank outside 1..n_shapes - 2 or not above its predecessor, relative_tolerance outside [0, 1) or NaN, all
 * shapes identical; GINGR_ERR_NONFINITE: a non-finite coordinate (the text names the shape) or eigenvalue.  Nothing is written then
 * and the context stays usable. */
int gingr_pca_leave_one_out(gingr_ctx *ctx, int64_t M, int32_t n_shapes, const double *shapes_xyz, double relative_tolerance,
                            int32_t n_ranks, const int32_t *ranks, double *avg, double *max, int32_t *fold_rank);

/* ---- the inverse-Laplacian model from the sparse Laplacian's own eigenpairs -------------------------------------------------
 * The model of DiagonalKernel(LookupKernel(pinv(L)) * scaling) (GPMMHelper.scala:132-136, InvLapKernel) without the n x n
 * pseudo-inverse: a new, finalized, single-shard model on this context.  Everything is host memory: ref_xyz [3 M] the reference,
 * cells [3 n_cells] its triangles.
 * Definition.  L = D - A, A the adjacency of the unique undirected edges of the triangulation (LaplacianHelper.laplacianMatrix; a
 * cell that names a vertex twice adds no loop).  (mu_j, v_j): its eigenpairs, |v_j| = 1, mu ascending, those with mu <= 1e-5 dropped
 * (the cut-off of MatrixHelper.pinv, MatrixHelper.scala:21-26: one null vector per connected component, isolated vertices included);
 * j = 0 .. k - 1 over what is left, k = n_pairs.  The model has rank 3 k, mean 0 and the reference as given; for d in {x, y, z}
 * variance[3 j + d] = scaling / mu_j and basis[(i, d), 3 j + d] = v_j[i], every other entry exactly 0.  The sign of v_j makes its
 * component of largest magnitude positive (the lowest vertex index on a tie).  These are the leading 3 k components of the reference's
 * model built to a tight tolerance.  A cut inside a cluster of equal eigenvalues is allowed: the vectors are then some orthonormal
 * vectors of that eigenspace, and info->cut_gap says so.
 * Solve: Chebyshev-filtered subspace iteration on the device (lap_spectral.hip), stopped when |L v - mu v| <= tolerance * Lambda for
 * every wanted pair, Lambda = 2 * (largest vertex degree); tolerance <= 0: 1e-10.  max_degree: the budget of products of L with the
 * block, <= 0: the default (4 000).  A solve that does not reach the tolerance within the budget returns GINGR_ERR_NOT_CONVERGED and
 * no model -- never a less accurate one.  Two calls with the same input give the same bits.  Synchronises.
 * GINGR_ERR_BAD_ARGUMENT (gingr_last_error names the cause): n_pairs outside 1 .. 170 (3 k <= 512), n_pairs larger than the number of
 * eigenvalues above the cut-off, n_cells < 1, a cell index outside [0, M), scaling not positive; GINGR_ERR_NONFINITE: a non-finite
 * coordinate.  *out is NULL then; info (nullable) is filled in as far as the call came. */
typedef struct gingr_laplacian_info {
    int32_t n_components;     /* connected components of the edge graph (an isolated vertex is one) */
    int32_t n_dropped;        /* eigenvalues <= 1e-5: the components' null vectors and whatever else lies below the cut-off */
    int32_t block_columns;    /* columns of the iteration block (wanted + guard, padded to a multiple of 16) */
    int32_t outer_iterations; /* filter + orthonormalisation + Rayleigh-Ritz steps */
    int32_t total_degree;     /* products of L with the block */
    int32_t converged;        /* 1: every wanted residual is within the tolerance */
    double max_residual;      /* largest |L v - mu v| / Lambda of the wanted pairs at the end */
    double cut_gap;           /* (mu_{k+1} - mu_k) / mu_k from the first guard column's Ritz value; +inf when no eigenvalue is left */
} gingr_laplacian_info;
int gingr_model_from_laplacian(gingr_ctx *ctx, int64_t M, const double *ref_xyz, int64_t n_cells, const int32_t *cells, double scaling,
                               int32_t n_pairs, double tolerance, int32_t max_degree, gingr_laplacian_info *info /* may be NULL */,
                               gingr_model **out);

/* The retry counter of the probabilistic proposal (G/api/GingrAlgorithm.scala:69-70,196-202,210: `retryCounter`, a private var
 * of the algorithm INSTANCE): a sampled proposal whose posterior cannot be computed returns the state unchanged up to 10 times in
 * a row before the state is marked ModelFlexibilityError; every successful posterior gives one retry back (at most 10).  The
 * fitter is the device-side stand-in of one algorithm instance, so the counter lives with it (it survives gingr_fitter_set_state).
 * set_to >= 0 writes the counter, set_to < 0 only reads; value_out (nullable) receives the value.  Synchronises. */
int gingr_fitter_retry_counter(gingr_fitter *f, int32_t set_to, int32_t *value_out);

/* ---- row-sharded update, host-driven exchange (multi-GPU) -----------------------------------------------------
 * One iteration = phases 0..GINGR_NUM_PHASES-1.  After phase p < GINGR_NUM_SEGMENTS the host all-reduces (sum, float64)
 * exchange segment p across shards (RCCL over xGMI via torch.distributed, or nothing for one shard), then runs phase p+1.
 * The exchange buffer is device memory owned by the library; gingr_fitter_exchange gives its address and the
 * [offset, count) of every segment in float64 elements.
 * Stream contract: phase kernels are enqueued on the context's stream (gingr_ctx_set_stream / gingr_ctx_get_stream).  A host that
 * runs its collective on another stream must order the two itself: wait for the context's stream before the all-reduce and for
 * the collective before the next phase (gingr_amd/sharded.py does exactly that when the streams differ).  The in-library
 * alternative that needs no host collective at all is the device group below (gingr_group_*).
 *   phase 0 -> segment 0: den partial column sums [N]           (the CPD column-sum exchange; unused for ICP)
 *   phase 1 -> segment 1: weighted Gram [rp*rp] + rhs [rp] + sigma2 sums [8]
 *   phase 2: replicated r x r algebra (posterior solve, projections and Umeyama from the model's one-off moments),
 *            state commit, new fit of the local rows -- nothing to exchange.
 */
#define GINGR_NUM_PHASES 3
#define GINGR_NUM_SEGMENTS 2
/* Row-sharded SURFACE ICP only (round 4): the rejection tests against the template itself need the whole posed template, so an
 * iteration starts with one more step -- phase GINGR_PHASE_GATHER writes this shard's rows of the fit into the full-fit buffer
 * ([3][M_total] planes, original point order, zeros elsewhere; gingr_fitter_fullfit_exchange gives its address), the host
 * all-reduces (sum) it across the shards = an all-gather, then phases 0, 1, 2 as above.  In the one-call protocols below it is
 * exchange segment GINGR_SEGMENT_FULLFIT of the callback. */
#define GINGR_PHASE_GATHER 3
#define GINGR_SEGMENT_FULLFIT 2
/* Reversed correspondence direction on row shards (round 5; G/api/registration/utils/ClosestPointRegistrator.scala:34-49): the queries
 * of that direction are the vertices of the (replicated) target, so they partition by index range -- every shard scans its range
 * against the gathered template and leaves, per vertex of the WHOLE template, the sum of its accepted target points and their
 * number ([4][M_total] = sum x, sum y, sum z, count; gingr_fitter_reversal_exchange gives the address).  Between phases 0 and 1 the
 * host all-reduces (sum) that buffer = exchange segment GINGR_SEGMENT_REVSUM of the callback; phase 1 then takes the shard's rows. */
#define GINGR_SEGMENT_REVSUM 3
int gingr_fitter_exchange(gingr_fitter *f, void **dev_ptr, int64_t offsets[GINGR_NUM_SEGMENTS],
                          int64_t counts[GINGR_NUM_SEGMENTS]);
int gingr_fitter_cpd_phase_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t phase);
int gingr_fitter_icp_phase_async(gingr_fitter *f, const gingr_icp_params *p, int32_t phase);
/* The same protocol as ONE call per n iterations: the library runs the phases and calls `reduce(user, segment, device_ptr, count)`
 * wherever a segment has to be summed across the shards; the callback enqueues an in-place float64 sum all-reduce of those
 * `count` elements, ordered after everything already on the context's stream and before whatever is enqueued on it afterwards
 * (RCCL on that stream, or torch.distributed with that stream current), and returns 0 -- any other value aborts the update and
 * is returned as GINGR_ERR_STATE.  Nothing waits for the GPU: with an asynchronous collective all n iterations are enqueued
 * back to back.  ICP point-cloud correspondences need no segment-0 exchange (the rows are independent) and the callback is not
 * called for it.  Replaces the host loop of three phase calls + two collectives per iteration (gingr_amd/sharded.py);
 * reference: the per-iteration work of G/api/GingrAlgorithm.scala:192-254 on a row shard. */
typedef int (*gingr_allreduce_fn)(void *user, int32_t segment, void *device_ptr, int64_t count);
int gingr_fitter_update_cpd_sharded_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t n_iterations, gingr_allreduce_fn reduce,
                                          void *user);
int gingr_fitter_update_icp_sharded_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations, gingr_allreduce_fn reduce,
                                          void *user);

/* Any flavour, deterministic or sampled, as ONE call (round 4: the surface correspondence -- the reference's default ICP method,
 * G/api/registration/config/ICP.scala:63 -- the probabilistic proposal and the transition density are row-sharded too).
 *   flavour 0 CPD (cp), 1 ICP point cloud (ip), 2 ICP surface (ip; gingr_fitter_set_meshes on every shard with the triangles of the
 *   WHOLE template -- vertex ids of the full model -- and of the target; the shard's queries are its own rows, the tests against the
 *   template itself see all of it through the gathered fit, exchange segment GINGR_SEGMENT_FULLFIT), 3 the caller's pairs (cp and ip
 *   unused; gingr_fitter_set_pairs / _set_pairs_cov on every shard with the WHOLE lists, each keeps the pairs of its own rows; like
 *   ICP, no segment-0 exchange).
 *   z (nullable): rank standard-normal draws = update(current, probabilistic = true), n_iterations must be 1; the same z on every
 *   shard (the sample a + L^-T z is replicated r x r algebra).
 * gingr_fitter_posterior_logpdf_sharded: posterior(state).gp.logpdf(posterior.coefficients(mesh))
 * (G/api/sampling/generators/GeneratorWrapperStochastic.scala:42-63) with mesh_xyz_full = the FULL mesh [3 M_total] on every shard
 * (each takes its rows); Q0^T e travels in the tail of segment 1, the log-density kernel is replicated; synchronises.
 * Reversed correspondence direction (ICP.scala:46-48; gingr_fitter_set_correspondence_direction after gingr_fitter_set_meshes): every
 * shard scans its index range of the target queries against the gathered template; the per-template-vertex sums are all-reduced
 * (GINGR_SEGMENT_REVSUM, between phases 0 and 1) and every shard keeps the observations of its own rows.
 * gingr_fitter_fullfit_exchange / gingr_fitter_reversal_exchange: address / element count of the full-fit buffer / the reversal sums
 * for a host that drives the phases itself. */
int gingr_fitter_update_sharded_async(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                      int32_t n_iterations, const double *z, gingr_allreduce_fn reduce, void *user);
int gingr_fitter_posterior_logpdf_sharded(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                          const double *mesh_xyz_full, gingr_allreduce_fn reduce, void *user, double *logpdf);
int gingr_fitter_fullfit_exchange(gingr_fitter *f, void **dev_ptr, int64_t *count);
int gingr_fitter_reversal_exchange(gingr_fitter *f, void **dev_ptr, int64_t *count);
/* The gather of the fit through a real ALL-GATHER instead of the zero-padded all-reduce (half the wire bytes, no reduction) for hosts
 * that have one (the library's own RCCL path uses ncclAllGather this way).  The shards must be the balanced contiguous partition of
 * the rows over `world` shards (the first M_total % world shards hold one row more -- what gingr_group_* and gingr_amd.sharded use).
 *   gingr_fitter_gather_stage   enqueues the copy of this shard's rows (original order) into its slot of a staging buffer
 *                               [world][3][chunk], chunk = ceil(M_total / world), and returns the slot (send), the buffer (recv) and
 *                               the element count per rank (3 chunk): the host runs an in-place all-gather of exactly that shape on
 *                               the context's stream (ncclAllGather(send, recv, count, ncclDouble, ...));
 *   gingr_fitter_gather_finish  enqueues the kernel that spreads the slots over the planes of the full-fit buffer.
 * Together they replace phase GINGR_PHASE_GATHER + the all-reduce of segment GINGR_SEGMENT_FULLFIT; then phases 0, 1, 2 as above. */
int gingr_fitter_gather_stage(gingr_fitter *f, int32_t world, int32_t rank, void **send_ptr, void **recv_ptr, int64_t *count_per_rank);
int gingr_fitter_gather_finish(gingr_fitter *f, int32_t world);

/* ---- one Metropolis-Hastings step of GingrAlgorithm.run's chain in ONE call (G/api/GingrAlgorithm.scala:115-190; scalismo
 * MetropolisHastings.next = propose, evaluate both, transition ratio, accept / reject) ---------------------------------------------
 * The device state x (gingr_fitter_set_state, or what the previous step left) is the current sample.  The call enqueues
 *   x' = kind 0: update(x, probabilistic = true) with the r standard normals z (GeneratorWrapperStochastic.propose,
 *        G/api/sampling/generators/GeneratorWrapperStochastic.scala:28-40), or
 *        kind 1: the parameters a random-walk proposal chose (alpha, scalars incl. iteration + 1; the fit is re-instantiated on the
 *        device: GingrGeneratorWrapper.scala:28-39)
 *   log_q_forward  = logTransitionProbability(x, x') = posterior(x).gp.logpdf(posterior.coefficients(x.fit)): with step length 1 the
 *                    reference projects FROM.fit (GeneratorWrapperStochastic.scala:42-63), so this is a function of x alone -- the
 *                    log_q_backward of the step that produced x -- and is computed only with need_forward != 0 (else NaN, status -1)
 *   log_q_backward = logTransitionProbability(x', x) = posterior(x').gp.logpdf(posterior.coefficients(x'.fit))
 *   log_value      = sum over the first eval_points fit vertices of x' (0 = all) of log N(|v - closestPointOnSurface(v)|; 0, eval_sdev)
 *                    against the target surface (IndependentPointDistanceEvaluator.scala:54-70, ModelToTargetEvaluation)
 * and synchronises ONCE.  x' is the device state on return; alpha_out[r] / fit_out[3 M] (nullable) / res->scalars describe it.  A
 * density is -inf with its status GINGR_ERR_NOT_SPD / GINGR_ERR_NONFINITE when the posterior it needs fails (what the reference's Try
 * turns into Double.NegativeInfinity).  The host combines these with the densities of its random-walk components and decides; after a
 * rejection gingr_fitter_mh_restore makes x the device state again (asynchronous).  Every state's correspondences and Gram are
 * computed once (two-slot posterior memo).  Single shard, meshes set, flavour as in gingr_fitter_update_sharded_async. */
typedef struct gingr_mh_request {
    int32_t flavour, kind;
    const gingr_cpd_params *cpd; /* flavour 0 */
    const gingr_icp_params *icp; /* flavours 1, 2 */
    const double *z;             /* kind 0 */
    const double *alpha;         /* kind 1 */
    const gingr_state_scalars *scalars;
    double eval_sdev;
    int64_t eval_points;
    int32_t need_forward;
} gingr_mh_request;
typedef struct gingr_mh_result {
    gingr_state_scalars scalars; /* of x' */
    double log_value, dist_sum, dist_max;
    int64_t count;
    double log_q_forward, log_q_backward;
    int32_t forward_status, backward_status;
} gingr_mh_result;
int gingr_fitter_mh_step(gingr_fitter *f, const gingr_mh_request *request, double *alpha_out, double *fit_out, gingr_mh_result *result);
int gingr_fitter_mh_restore(gingr_fitter *f);

/* ---- native RCCL exchange: the row-sharded update with one process per GPU and the collective enqueued by the LIBRARY ------------
 * BASELINE.json north_star: "the N x M affinity/distance matrix shards by reference-point rows across the 8 GPUs of one node with an
 * RCCL all-reduce over xGMI for CPD column sums".  Every rank owns one context (one device, one stream), one row shard of the model
 * and one fitter, as with gingr_fitter_update_*_sharded_async; here the two per-iteration all-reduces are ncclAllReduce calls the
 * library itself places on the context's stream between the phase kernels -- n iterations are enqueued with no callback, no stream
 * hop and no host synchronisation.  librccl is bound at run time (dlopen; a copy already loaded in the process -- e.g. torch's -- is
 * shared), so a single-GPU host does not need it.
 *   bootstrap: rank 0 calls gingr_rccl_unique_id (128 bytes), the HOST distributes them to all ranks (a JVM host: its own channel;
 *   bench.py: the torch.distributed store), every rank calls gingr_ctx_rccl_init(ctx, id, world, rank) -- collective, returns when the
 *   communicator of the `world` ranks exists.  The communicator belongs to the context and dies with it.
 *   one-off: gingr_ctx_rccl_allreduce_async sums the basis moments (gingr_model_gram_exchange) before gingr_model_finalize.
 *   per n iterations: gingr_fitter_update_{cpd,icp}_rccl_async.
 * gingr_rccl_load (optional, before anything else): bind a specific librccl by path instead of the default search
 * (already-loaded librccl.so.1, then the loader's path).  gingr_ctx_rccl_info: what was bound (diagnostics; any pointer may be NULL).
 * Reference: none (the reference is single-process / single-device); the protocol is that of G/api/GingrAlgorithm.scala:192-254 on
 * a row shard as in the host-driven section above. */
#define GINGR_RCCL_UNIQUE_ID_BYTES 128
int gingr_rccl_load(gingr_ctx *ctx, const char *librccl_path);
int gingr_rccl_unique_id(gingr_ctx *ctx, void *id_bytes);
int gingr_ctx_rccl_init(gingr_ctx *ctx, const void *id_bytes, int32_t world, int32_t rank);
int gingr_ctx_rccl_info(gingr_ctx *ctx, int32_t *world, int32_t *rank, int32_t *version, char *library_path, int32_t path_capacity);
int gingr_ctx_rccl_allreduce_async(gingr_ctx *ctx, void *device_ptr, int64_t count);
int gingr_fitter_update_cpd_rccl_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t n_iterations);
int gingr_fitter_update_icp_rccl_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations);
/* any flavour / sampled proposal / transition density over the context's communicator: gingr_fitter_update_sharded_async and
 * gingr_fitter_posterior_logpdf_sharded with the library's own ncclAllReduce as the exchange */
int gingr_fitter_update_rccl_async(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                   int32_t n_iterations, const double *z);
int gingr_fitter_posterior_logpdf_rccl(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                       const double *mesh_xyz_full, double *logpdf);

/* ---- device group: the row-sharded update across the GPUs of ONE node from ONE host process (multi-GPU for a C / JVM host) ----
 * SURVEY.md section 8b "gingr_group_create(ndev, devs[], ...) wrapping the same calls with row-sharding".  The group owns one
 * context, one model shard (contiguous rows, the first M mod n shards hold one extra row) and one fitter per entry of `devices`;
 * the target cloud and the r-sized state are replicated.  Per iteration the two exchange segments above are summed across the
 * shards inside the library: every shard writes its partial segment to a send buffer, the shards exchange HIP events, and each
 * shard sums all send buffers in rank order (its own and, through the xGMI peer mapping, the remote ones) with one kernel --
 * a one-shot all-reduce; both messages are small (N doubles; rp*rp + rp + 8), so it is latency bound.  Every shard computes
 * bit-identical sums, the r x r solve is replicated, results do not depend on timing.  One host thread per device enqueues
 * that device's kernels; gingr_group_update_*_async returns when n iterations are ENQUEUED on every device
 * (gingr_group_synchronize / gingr_group_get_state wait for them).  Not thread-safe: one caller thread per group.
 * The same device may be listed several times (logical shards on one GPU: how the protocol is tested on a one-GPU box).
 * Reference: the reference is single-process / single-device; the calls mirror gingr_model_upload / gingr_gpmm_build_gaussian /
 * gingr_fitter_* one to one (same argument meaning; host arrays are always the FULL model / cloud / fit).
 * Errors: the gingr_status of the first failing shard; gingr_group_last_error has the text. */
typedef struct gingr_group gingr_group;
int gingr_group_create(int32_t ndev, const int32_t *devices, gingr_group **out);
void gingr_group_destroy(gingr_group *g);
int32_t gingr_group_size(const gingr_group *g);
const char *gingr_group_last_error(const gingr_group *g);
gingr_ctx *gingr_group_ctx(gingr_group *g, int32_t shard);      /* e.g. for the timing hooks of one shard */
int gingr_group_shard_rows(const gingr_group *g, int32_t shard, int64_t *row_begin, int64_t *row_end);
int gingr_group_model_upload(gingr_group *g, int64_t M_total, int32_t rank, const double *ref, const double *mean,
                             const double *basis_colmajor, const double *variance);
int gingr_group_gpmm_build_gaussian(gingr_group *g, int64_t M_total, const double *ref, int32_t n_kernels, const double *sigmas,
                                    const double *scalings, double relative_tolerance, int32_t max_rank);
int32_t gingr_group_model_rank(const gingr_group *g);
int gingr_group_set_target(gingr_group *g, int64_t N, const double *target_xyz);
int gingr_group_set_landmarks(gingr_group *g, int32_t n_lm, const int32_t *lm_pid, const double *lm_xyz, const double *lm_cov);
int gingr_group_set_options(gingr_group *g, int32_t global_transform, double step_length);
int gingr_group_set_state(gingr_group *g, const double *alpha, const gingr_state_scalars *s);
/* alpha[r] and scalars from shard 0 (replicated state), fit_xyz[3*M_total] gathered from all shards; synchronises */
int gingr_group_get_state(gingr_group *g, double *alpha, gingr_state_scalars *s, double *fit_xyz);
int gingr_group_update_cpd_async(gingr_group *g, const gingr_cpd_params *p, int32_t n_iterations);
int gingr_group_update_icp_async(gingr_group *g, const gingr_icp_params *p, int32_t n_iterations);
/* Round 4: the surface correspondence, the sampled proposal and the transition density through the group (the mirror of
 * gingr_fitter_set_meshes / _set_surface_method / gingr_fitter_update_sharded_async / gingr_fitter_posterior_logpdf_sharded; same
 * argument meaning: flavour 0 CPD, 1 ICP point cloud, 2 ICP surface; z nullable, then one iteration; triangles in the vertex ids of
 * the FULL model / target).  gingr_group_posterior_logpdf synchronises. */
int gingr_group_set_meshes(gingr_group *g, int64_t n_model_triangles, const int32_t *model_triangles, int64_t n_target_triangles,
                           const int32_t *target_triangles);
int gingr_group_set_surface_method(gingr_group *g, int32_t method);
/* gingr_fitter_set_correspondence_direction for every shard (ICP.scala:46-48).  With more than one shard the correspondence runs
 * against the GATHERED template (set the meshes first, also for the vertex-to-vertex flavour 1) and is sharded by QUERY range: every
 * shard scans its slice of the replicated target's vertices, the per-template-vertex sums of the slices are totalled by one more
 * exchange (GINGR_SEGMENT_REVSUM), and each shard then forms the observations of its own rows; Gram, right-hand side and everything
 * behind them stay sharded by rows.  gingr_group_set_meshes drops the direction again (as gingr_fitter_set_meshes does). */
int gingr_group_set_correspondence_direction(gingr_group *g, int32_t reversed);
int gingr_group_update_async(gingr_group *g, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip, int32_t n_iterations,
                             const double *z);
int gingr_group_posterior_logpdf(gingr_group *g, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                 const double *mesh_xyz_full, double *logpdf);
int gingr_group_synchronize(gingr_group *g);
/* How the group exchanges (diagnostics for a first run on real multi-GPU hardware): *distinct_devices = physical devices behind
 * the shards; *fine_grained = 1 when the peer-read send buffers are fine-grained device allocations (always the case when
 * distinct_devices > 1: gingr_group_set_target fails with GINGR_ERR_HIP instead of falling back to coarse-grained memory, which
 * a peer could not read coherently).  Either pointer may be NULL.  No reference counterpart (the reference is single-device). */
int gingr_group_exchange_info(const gingr_group *g, int32_t *distinct_devices, int32_t *fine_grained);

/* -------------------------------------------------------------- timing hooks
 * HIP-event timing of the dominant kernels on the context's stream (bench.py's live roofline measurement).
 * which: 0 = cpd_colsum, 1 = cpd_rowstats, 2 = gram, 3 = whole update, 4 = basis sweep (one streaming pass over Q0),
 * 5 = posterior solve (unfused tail only), 6 / 7 = the device group's exchange of segment 0 / 1 on this shard (from the record of
 * the shard's own event to the end of its sum kernel: includes the wait for the slowest peer; the host-driven sharded update records its two collectives there too), 8 = the
 * nearest-neighbour scan kernel alone, 9 = the per-vertex covariance pass over the basis alone, 10 = the basis pass of the posterior model (basis_rotate_kernel) alone,
 * 11 / 12 = the cross Gram pass / the two-source basis pass of gingr_model_augment alone, 13 .. 16 = the stages of gingr_mesh_decimate:
 * bounding box, bisection (every enqueued step, the ones that return at once included), clusters and representatives (insertion at
 * the chosen size, sort, means, argmin), compaction of vertices and triangles, 17 = the Chebyshev step of gingr_model_from_laplacian
 * (lap_cheb_kernel) alone, 18 / 19 / 20 = the passes of the model metrics alone: reconstruct and measure (gingr_model_generalization), samples
 * against training shapes (gingr_model_specificity), the stored basis x factor product (gingr_model_instances, gingr_model_specificity),
 * 21 = the pivot step of gingr_model_localize alone, 22 = the batched eigen-decomposition of the folds of gingr_pca_leave_one_out alone
 * (one launch per batch of folds; up to n_shapes = 193), 23 = the batched closest-point scan of the surface-distance metrics alone, 24 / 25 / 26 = the stages of gingr_rigid_search beside
 * its search (which is 8): the segmented selection, the segmented sums, the rest (pose, step and argmin kernels; the inlier and selection kernels of
 * gingr_rigid_search_poses), 27 / 28 / 29 = the kernels of gingr_cloud_fpfh behind its neighbour search (SPFH and FPFH), of
 * gingr_feature_match (chunks and their combination) and of gingr_rigid_poses_from_triples alone.  Returns accumulated ms and launches since
 * the last reset.  Enabling adds two event records per launch. */
int gingr_ctx_timing_enable(gingr_ctx *ctx, int32_t enable);
int gingr_ctx_timing_read(gingr_ctx *ctx, int32_t which, double *total_ms, int64_t *launches);
int gingr_ctx_timing_reset(gingr_ctx *ctx);
/* Diagnostics of the nearest-neighbour scan (ClosestPointRegistrator.scala:139-145 is an unpruned scan of every pair; this one prunes
 * exactly): with counting enabled every gingr_nn / ICP launch on this context adds the distance tests it really executed to a device
 * counter (a second instantiation of the kernel; the default one carries no counter).  gingr_ctx_nn_counting(ctx, 1) switches it on
 * and clears the counter, (ctx, 0) switches it off; gingr_ctx_nn_tests waits for the stream and returns the count. */
int gingr_ctx_nn_counting(gingr_ctx *ctx, int32_t enable);
int gingr_ctx_nn_tests(gingr_ctx *ctx, int64_t *tests);

/* ---- classic Coherent Point Drift (the reference's `other/` CPD family as a second consumer of the
 * affinity statistics and of the Gaussian kernel block) ----------------------------------------------------------------------
 * One handle = CPDFactory(templatePoints, lambda, beta, w).registerRigidly / registerAffine / registerNonRigidly(targetPoints)
 * (G/other/algorithms/cpd/CPDFactory.scala:28-80); kind 0 rigid (similarity: s, R, t; RigidCPD.scala:107-137), 1 affine
 * (AffineCPD.scala:35-60), 2 non-rigid (G + lambda sigma2 diag(1/P1)) W = diag(1/P1) P X - Y, TY = Y + G W
 * (NonRigidCPD.scala:45-88).  The state (TY, sigma2) of RigidCPD.Registration (:59-83) lives on the device; it starts at
 * (template, sum |y_m - x_n|^2 / (3 M N)).  gingr_classic_cpd_iterate runs n Iteration()s (:85-88) back to back and synchronises;
 * the caller owns the convergence test |sigma2' - sigma2| < tolerance (:70-78).  gingr_classic_cpd_get: any of ty_xyz [3 M],
 * sigma2, transform13 = {s, R or B row-major [9], t [3]} (rigid / affine, last Maximization), w_xyz [3 M] (non-rigid) may be NULL.
 * moving_xyz = the templatePoints [3 M], target_xyz = the targetPoints [3 N]. */
typedef struct gingr_classic_cpd gingr_classic_cpd;
int gingr_classic_cpd_create(gingr_ctx *ctx, int32_t kind, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz,
                             double lambda, double beta, double w, gingr_classic_cpd **out);
void gingr_classic_cpd_destroy(gingr_classic_cpd *h);
int gingr_classic_cpd_iterate(gingr_classic_cpd *h, int32_t n_iterations);
int gingr_classic_cpd_get(gingr_classic_cpd *h, double *ty_xyz, double *sigma2, double *transform13, double *w_xyz);
int gingr_classic_cpd_set(gingr_classic_cpd *h, const double *ty_xyz, double sigma2);

/* The non-rigid kind past dense sizes (Myronenko & Song 2010, "fast implementation"): G ~ L L^T by the pivoted Cholesky of the
 * Gaussian over the template (the factorisation of gingr_gpmm_build_*: at most GINGR_CLASSIC_CPD_MAX_COLUMNS columns, stopped when
 * the residual trace falls below relative_tolerance * trace) and the Woodbury identity: with D = diag(P1), c = lambda sigma2,
 *     (c I + L^T D L) z = L^T (P X - D Y),   TY = Y + L z,   W = D (D^-1 P X - Y - L z) / c,
 * which is the step of kind 2 with L L^T in place of G.  Nothing of size M x M is formed: no limit on M but the card's memory
 * (the factor takes 8 bytes x M rounded up to 32 x k rounded up to 64; the factorisation, at create time only, as much again for the
 * columns it may reach).  relative_tolerance in [0, 1); max_columns <= 0: to the tolerance under the ceiling, > 0: the
 * caller's stop, above the ceiling: GINGR_ERR_BAD_ARGUMENT.  Stopping at max_columns or at the ceiling before the tolerance is met is
 * no error: info (nullable) reports it.  The handle is a gingr_classic_cpd of kind 2 for iterate / get / set / destroy; w_xyz of
 * gingr_classic_cpd_get is the W above.  gingr_classic_cpd_get_factor: *columns (nullable) and L row-major [M][columns] (nullable);
 * GINGR_ERR_STATE on a handle of gingr_classic_cpd_create. */
#define GINGR_CLASSIC_CPD_MAX_COLUMNS 512
typedef struct {
    int32_t columns;           /* k */
    int32_t tolerance_reached; /* 1: residual trace < relative_tolerance * trace (or k = M) */
    double residual_fraction;  /* trace(G - L L^T) / trace(G) */
    int64_t factor_bytes;      /* device memory held for L */
} gingr_classic_cpd_lowrank_info;
int gingr_classic_cpd_create_lowrank(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz,
                                     double lambda, double beta, double w, double relative_tolerance, int32_t max_columns,
                                     gingr_classic_cpd_lowrank_info *info, gingr_classic_cpd **out);
int gingr_classic_cpd_get_factor(gingr_classic_cpd *h, int32_t *columns, double *L_rowmajor_M_by_k);

/* ---- Bayesian coherent point drift (Hirose 2020; the reference's draft other/algorithms/cpd/BCPD.scala, BCPDRegistration.scala) ----
 * One handle = BCPD(templatePoints, targetPoints, w, lambda, gamma, k, beta) with the Gaussian kernel of CPDFactory,
 * g(a, b) = exp(-|a - b|^2 / (2 beta^2)).  The definition is this package's (DESIGN.md section 5 lists where it follows the paper
 * against the draft): soft assignment with the row weights <alpha_m> exp(-1.5 s^2 sigma_m^2 / sigma2) and the outlier density 1 / V
 * (V: the volume of the target's bounding box), the deformation v^ = c2 Sigma r and sigma_m^2 = Sigma_mm through the Woodbury form of
 * Sigma = (lambda G^-1 + c2 diag nu)^-1 (one blocked Cholesky of I + D^1/2 (G / lambda) D^1/2 per iteration, G never inverted), the
 * similarity (s, R, t) from the singular vectors of S_xu, then y^ = s R (y + v^) + t and sigma2.  Nothing divides by nu_m.
 * The state (y^, sigma_m^2, <alpha_m>, s, R, t, sigma2) lives on the device and starts at (template, 1, 1 / M, 1, I, 0,
 * gamma sum |x_n - y_m|^2 / (3 N M)).  gingr_bcpd_iterate runs n iterations back to back and synchronises; the caller owns the
 * convergence test |sigma2' - sigma2| < tolerance.  It fails with GINGR_ERR_NONFINITE (w = 0 and a target point out of reach of every
 * template point) or GINGR_ERR_NOT_SPD; the handle stays usable after gingr_bcpd_set.
 * gingr_bcpd_create refuses (GINGR_ERR_BAD_ARGUMENT): w outside [0, 1), non-positive lambda, gamma, kappa, beta (kappa = +inf is
 * allowed: <alpha_m> = 1 / M), M or N < 1, a target whose bounding box has no volume while w > 0, and M > 32768 (the iteration keeps
 * M x M double buffers: G, the bordered system of twice that size and its workspace, 43 GB at the cap).
 * moving_xyz = the templatePoints [3 M], target_xyz = the targetPoints [3 N].
 * gingr_bcpd_get: every pointer may be NULL.  yhat_xyz, vhat_xyz [3 M] interleaved, sigma_diag, alpha, nu [M], nu_prime [N],
 * transform13 = {s, R row-major [9], t [3]} (x = s R u + t), scalars3 = {sigma2, N^ = sum nu, the nu-weighted mean of sigma_m^2}.
 * gingr_bcpd_set injects a state: NULL pointers and a sigma2 that is not > 0 leave their part as it is. */
typedef struct gingr_bcpd gingr_bcpd;
int gingr_bcpd_create(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, double w, double lambda,
                      double gamma, double kappa, double beta, gingr_bcpd **out);
void gingr_bcpd_destroy(gingr_bcpd *h);
int gingr_bcpd_iterate(gingr_bcpd *h, int32_t n_iterations);
int gingr_bcpd_get(gingr_bcpd *h, double *yhat_xyz, double *vhat_xyz, double *sigma_diag, double *alpha, double *nu, double *nu_prime,
                   double *transform13, double *scalars3);
int gingr_bcpd_set(gingr_bcpd *h, const double *yhat_xyz, const double *sigma_diag, const double *alpha, const double *transform13,
                   double sigma2);

/* Past dense sizes (the acceleration Hirose 2020 proposes): G ~ L L^T, the factor of gingr_classic_cpd_create_lowrank (the same
 * pivoted Cholesky of the same Gaussian over the template, the same ceiling GINGR_CLASSIC_CPD_MAX_COLUMNS, the same rules for
 * relative_tolerance and max_columns, the same info block).  With K = L L^T / lambda and c2 = s^2 / sigma2 the deformation step is
 *     S = L^T diag(nu) L,  C = I + (c2 / lambda) S = R R^T,  v^ = (c2 / lambda) L C^-1 L^T r,  sigma_m^2 = |R^-1 l_m|^2 / lambda
 * (l_m: row m of L), which is the step of gingr_bcpd_create with L L^T in place of G: a sum of squares, never negative, and nothing
 * divides by nu_m.  Nothing of size M x M is formed, so the cap of 32768 does not apply: no limit on M but the card's memory (the factor
 * takes 8 bytes x M rounded up to 32 x k rounded up to 64; the factorisation, at create time only, as much again for the columns it
 * may reach; the pair passes keep up to 256 chunk partials of N doubles or of 4 M doubles).  Every other argument rule is
 * gingr_bcpd_create's.
 * The handle is a gingr_bcpd for iterate / get / set / destroy, with the same failures of gingr_bcpd_iterate.
 * gingr_bcpd_get_factor: *columns (nullable) and L row-major [M][columns] (nullable); GINGR_ERR_BAD_ARGUMENT on a handle of
 * gingr_bcpd_create. */
int gingr_bcpd_create_lowrank(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, double w,
                              double lambda, double gamma, double kappa, double beta, double relative_tolerance, int32_t max_columns,
                              gingr_classic_cpd_lowrank_info *info, gingr_bcpd **out);
int gingr_bcpd_get_factor(gingr_bcpd *h, int32_t *columns, double *L_rowmajor_M_by_k);

/* ---- the fitted map at points off the template (kernel_warp.hip; BCPD++'s interpolation step, pycpd's transform_point_cloud) ----
 * With Y the task's original template (moving_xyz), g(a, b) = exp(-|a - b|^2 / (2 beta^2)) the task's Gaussian and z any point:
 *   rigid / affine CPD (kinds 0, 1)   T(z) = s B z + t, (s, B, t) the transform13 of the last Maximization;
 *   non-rigid CPD, dense and low-rank T(z) = z + sum_m g(z, y_m) W_m, W the w_xyz of gingr_classic_cpd_get (low-rank: the W of the
 *                                     comment above).  The sum uses the true Gaussian, not L L^T: on the dense route T(y_m) is the
 *                                     TY_m of a Maximization that started at Y, to rounding; on the low-rank route
 *                                     T(y_m) - TY_m = ((G - L L^T) W)_m, which follows the factor's tolerance;
 *   BCPD, dense and low-rank          T(z) = s R (z + sum_m g(z, y_m) c_m) + t, (s, R, t) of the state after the iteration and
 *                                     c = (c2 / lambda) (r - nu o v^), c2 = s^2 / sigma2 and r those that went into the iteration:
 *                                     Sigma^-1 v^ = c2 r with Sigma^-1 = lambda G^-1 + c2 diag nu gives v^ = G c (L L^T in place
 *                                     of G on the low-rank route), so c needs no inverse of G and no division by nu_m, and
 *                                     g(z, Y) c is the Gaussian-process posterior mean of the displacement at z; T(y_m) = y^_m.
 * As transform13 and w_xyz, the map is the LAST iteration's: the classic kinds feed TY back into the next iteration, so after
 * several iterations their T is the last step of the composition, not the whole of it.
 * The entries return GINGR_ERR_STATE before any iteration, after gingr_*_set with no iteration since, and after an iteration that
 * failed.  points_xyz, out_xyz: [3 P] interleaved host arrays, P limited by memory alone; they may be the same array.  P = 0 succeeds
 * and touches nothing, in any state; P < 0 or a NULL pointer with P > 0: GINGR_ERR_BAD_ARGUMENT.  A point's image depends on that point and the
 * handle's state alone -- not on P or on the other points of the call -- and two calls give the same bits: the sum over the centres
 * is taken in chunks whose boundaries depend on M alone, added in chunk order.  A kernel entry g(z, y_m) has the bits of the dense
 * route's G where z = y_m'.  The points pass through the device in slabs of at most 2^20; the handle keeps the buffers of its largest
 * call (two slabs of points and the chunk partials, at most 128 MiB unless 256 points need more) until it is destroyed.
 * gingr_bcpd_get_coefficients: c [3 M] interleaved, formed on the first query after an iteration. */
int gingr_classic_cpd_transform_points(gingr_classic_cpd *h, int64_t P, const double *points_xyz, double *out_xyz);
int gingr_bcpd_transform_points(gingr_bcpd *h, int64_t P, const double *points_xyz, double *out_xyz);
int gingr_bcpd_get_coefficients(gingr_bcpd *h, double *c_xyz);

/* ---- classic rigid / similarity ICP (the reference's other/ baseline) ------------------------------------------------
 * G/other/algorithms/icp/RigidICP.scala:24-84 (Iteration / Registration), ICPFactory.scala:28-38, RigidICPRegistration.scala:24-46
 * with the two registrators of G/other/utils/PoseRegistrator.scala:27-43: kind 0 = RigidRegistrator3D
 * (LandmarkRegistration.rigid3DLandmarkRegistration about the origin), kind 1 = AffineRegistrator3D
 * (similarity3DLandmarkRegistration).  One iteration = closest target point of every template point (exact, lowest index on
 * ties), least-squares transform of the pairs, template <- transform(template); the template lives in HBM.
 * gingr_rigid_icp_iterate: distances[k] (nullable) = mean closest-point distance measured by iteration k BEFORE it moves the
 * template (RigidICP.scala:60-71,79-82) -- what Registration's convergence test compares.  _get: current template [3M] and the
 * last transform {s, R[9] row-major, t[3]} (either may be NULL).  _set: replace the template points. */
typedef struct gingr_rigid_icp gingr_rigid_icp;
int gingr_rigid_icp_create(gingr_ctx *ctx, int32_t kind, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz,
                           gingr_rigid_icp **out);
void gingr_rigid_icp_destroy(gingr_rigid_icp *h);
int gingr_rigid_icp_iterate(gingr_rigid_icp *h, int32_t n_iterations, double *distances);
int gingr_rigid_icp_get(gingr_rigid_icp *h, double *points_xyz, double *transform13);
int gingr_rigid_icp_set(gingr_rigid_icp *h, const double *points_xyz);

/* ---- global rigid pre-alignment: batched multi-start trimmed ICP ---------------------------------------------------------
 * No reference counterpart (its demos ship pre-aligned data): what brings a scan from an arbitrary pose to the start every local
 * method above needs.  S poses advance together on the device (csrc/rigid_search.hip, planning in csrc/rigid_search_plan.h); the
 * definition is restated in numpy in tests/rigid_search_restatement.py.
 * Start pose of s: T_s(x) = R0_s (x - mean X) + mean Y, held as (R_s, t_s) with p = R_s x + t_s.  One iteration, per pose: p_i =
 * R_s x_i + t_s from the ORIGINAL points (the returned pose reproduces the points exactly); j_i = the exact nearest target (lowest
 * index on ties, d2 = dx*dx + dy*dy + dz*dz separately rounded); keep = ceil(overlap * M) of the float64 product, tau = the order
 * statistic of rank keep - 1 of d2 and the kept set {i: d2_i <= tau}, ties included (overlap = 1: everything, no selection is
 * launched); from the kept pairs, with sums centred on mean Y, H = sum (y - mu_y)(p - mu_p)^T / n, dR = the proper rotation closest
 * to H (polar factor, else SVD with the determinant fix; no Euler round trip), dt = mu_y - dR mu_p; R_s <- dR R_s, t_s <- dR t_s + dt.
 * After K iterations one more search and selection: score_s = sqrt(mean of the kept d2).  A pose whose transform is not finite gets
 * score +inf and failed = 1 and takes no further part.  *best_out = the pose of the smallest score, the lowest s on ties.
 * rotations9 [S][9] row-major: the start rotations (gingr_rotation_samples gives the default ones).  Outputs, each nullable:
 * poses12_out [S][12] (R row-major, then t), scores_out [S], kept_out [S] (size of the kept set of the scoring pass), failed_out [S].
 * Poses run in slabs whose size depends on M and N alone; no sum reaches across poses, every sum has a fixed order and there is no
 * float atomic: two calls give the same bits, and a pose's outputs do not depend on which other poses are in the call.  Nothing is
 * read back before the end: the call synchronises once.
 * GINGR_ERR_NONFINITE (before anything is launched): a non-finite coordinate or rotation entry; (after the run) every pose failed.
 * GINGR_ERR_BAD_ARGUMENT: M < 1, N < 1 or N >= 2^31, S < 1, K < 0, overlap outside (0, 1], a null input or best_out.
 * gingr_rotation_samples: host only -- the n >= 1 rotations of the super-Fibonacci spiral (Alexa 2022), row-major [n][9]: with
 * phi = sqrt 2, psi = 1.533751168755204288118041 and s = i + 1/2 the quaternion (x, y, z, w) = (sqrt(s/n) sin(2 pi s / phi),
 * sqrt(s/n) cos(2 pi s / phi), sqrt(1 - s/n) sin(2 pi s / psi), sqrt(1 - s/n) cos(2 pi s / psi)). */
int gingr_rotation_samples(int64_t n, double *rotations9_out);
int gingr_rigid_search(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S,
                       const double *rotations9, int32_t K, double overlap, int64_t *best_out, double *poses12_out, double *scores_out,
                       int64_t *kept_out, int32_t *failed_out);
/* gingr_rigid_search_poses: the same run from start poses the caller gives -- poses12_in [S][12], R row-major then t -- instead of
 * rotations about the centroids: given (R0, mean Y - R0 mean X) it runs the very code gingr_rigid_search runs from there and returns
 * its bits.  A start pose with a non-finite word is failed from the beginning and takes no part (score +inf, kept 0, inliers 0, the
 * pose returned as given): the way the degenerate triples of gingr_rigid_poses_from_triples pass through.  inliers_out [S]
 * (nullable): the number of moving points -- all of them, trimmed or not -- with d2 <= inlier_distance^2 in the scoring pass, an
 * integer sum per pose.  select = 0: *best_out as above; select = 1: the pose with the most inliers, then the smaller score, then the
 * lowest s.  Errors as above; also GINGR_ERR_BAD_ARGUMENT for inlier_distance < 0 or NaN and select outside {0, 1}. */
int gingr_rigid_search_poses(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t S,
                             const double *poses12_in, int32_t K, double overlap, double inlier_distance, int32_t select, int64_t *best_out,
                             double *poses12_out, double *scores_out, int64_t *kept_out, int32_t *failed_out, int64_t *inliers_out);

/* ---- feature-based global alignment for partial targets: descriptors, their match, poses from triples of matches -------------
 * No reference counterpart.  Trimmed ICP from a centroid start slides along the shaft when the target is only a part of the
 * template; correspondences from local shape descriptors do not need the centroids.  csrc/feature_align.hip, planning in
 * csrc/feature_align_plan.h; the definitions restated in numpy in tests/feature_alignment_restatement.py.
 *
 * gingr_cloud_fpfh: Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009) -- THIS PACKAGE'S DEFINITION, not a toolkit's.
 * Neighbours of i: the entries of i's gingr_cloud_knn list (k nearest by (d2, index)), in list order, with 0 < d2 <= radius^2 -- the
 * point itself and its duplicates drop out; the list never leaves the device.  Pair (i, j), u = n_i, d = x_j - x_i, dn = d / |d|:
 * phi = u . dn; v = dn x u, the pair is SKIPPED when |v|^2 <= 2^-40 or either normal is zero, else v is normalised; w = u x v;
 * alpha = v . n_j; theta = atan2(w . n_j, u . n_j).  Eleven bins per feature: min(10, max(0, floor((f + 1) / 2 * 11))) for alpha and
 * phi, the same of (theta + pi) / (2 pi).  counts_out [N][33] (nullable): the integer tallies, alpha bins, then phi, then theta;
 * valid_out [N] (nullable): the counted pairs.  SPFH_i = 100 counts_i / valid_i (0 when valid_i = 0);
 * FPFH_i = SPFH_i + (sum_j SPFH_j / d_j) / (sum_j 1 / d_j) over ALL neighbours in list order, d_j = sqrt(d2_j) (0 without
 * neighbours); then each third is rescaled to sum 100 (a third that sums to 0 is left alone): fpfh_out [N][33].
 * normals [N][3] are normalised on upload by the rule of gingr_fitter_set_target_normals; a zero normal means "none".  The tallies
 * are integers and every float sum has a fixed order: two calls give the same bits.  info as gingr_cloud_knn (nullable).
 * GINGR_ERR_BAD_ARGUMENT: k outside [3, 64] or above N, radius not a finite number > 0, a null input or fpfh_out;
 * GINGR_ERR_NONFINITE (before any launch): a non-finite coordinate or normal.
 *
 * gingr_feature_match: for every row of a [M][D] the row of b [N][D] with the smallest sum_c (a_c - b_c)^2, 1 <= D <= 64: products
 * and sums separately rounded, added in ascending c from 0 -- the bits of that expression on a CPU -- and the lowest index on ties.
 * idx_out [M], d2_out [M] (nullable).  No matrix instruction: the norm-expansion form would change the bits and the tie rule.
 * GINGR_ERR_NONFINITE: a non-finite entry.
 *
 * gingr_rigid_poses_from_triples: H triples of pairs (moving[tri_moving[h][q]], target[tri_target[h][q]]), q = 0, 1, 2 -> the rigid
 * pose of each, poses12_out [H][12] (R row-major, then t): the Kabsch step of the three pairs with the reflection fix -- the
 * routine the pose step of gingr_rigid_search uses -- with sums centred on the triple's own target mean.  degenerate_out [H]
 * (nullable) = 1 and the pose NaN when an index repeats within a triple or the squared area of either triangle is
 * <= 2^-40 (longest edge)^4.  GINGR_ERR_BAD_ARGUMENT: an index out of range; GINGR_ERR_NONFINITE: a non-finite coordinate. */
int gingr_cloud_fpfh(gingr_ctx *ctx, int64_t N, const double *xyz, const double *normals, int32_t k, double radius, int32_t *counts_out,
                     int32_t *valid_out, double *fpfh_out, gingr_cloud_knn_info *info);
int gingr_feature_match(gingr_ctx *ctx, int64_t M, const double *a, int64_t N, const double *b, int32_t D, int32_t *idx_out, double *d2_out);
int gingr_rigid_poses_from_triples(gingr_ctx *ctx, int64_t M, const double *moving_xyz, int64_t N, const double *target_xyz, int64_t H,
                                   const int32_t *tri_moving, const int32_t *tri_target, double *poses12_out, int32_t *degenerate_out);


/* ---- optimal-step non-rigid ICP baselines (G/other/algorithms/icp/NonRigidOptimalStepICP.scala:31-284) ------------------------
 * The reference's loop is: closest-point correspondence of the current template mesh (ClosestPointTriangleMesh3D, the same
 * query as the GiNGR ICP path), then one sparse least-squares solve `A \ B`.  Both halves run on the device:
 *
 * gingr_fitter_set_fit_points: replace the shape the fitter's NEXT correspondence query looks at (normally the instance of the
 * current state) by explicit points [3M] -- the N-ICP template is no instance of a model.  Then
 * gingr_fitter_icp_surface_phase_async(f, p, 0) + gingr_fitter_get_surface_correspondence give (closest points, weights).
 *
 * gingr_nicp_solve: the least-squares step as its normal equations (dense on the device, blocked MFMA Cholesky), kind 0 = N-ICP-T
 * (:151-190, unknown n x 3 displacements), kind 1 = N-ICP-A (:241-283, one 4 x 3 affine map per vertex).  edges [2E]: the unique
 * vertex pairs p1 < p2 of the template triangles (trianglesToEdges :67-76); w [n], cp_xyz [3n]: the correspondence; lm_ids [L]
 * template vertices of the landmarks, lm_target_xyz [3L] their targets (UL); alpha stiffness, beta landmark weight, gamma the
 * fourth diagonal entry of G (N-ICP-A).  out_xyz [3n]: the moved template; out_lm_xyz (nullable, [3L]): the moved landmark
 * vertices (DL X of N-ICP-A).  Quirks of the reference kept: N-ICP-T's landmark rows put their ones into the FIRST L columns and
 * are not scaled by beta (only their right-hand side is); N-ICP-A zeroes the weights of the landmark vertices. */
int gingr_fitter_set_fit_points(gingr_fitter *f, const double *fit_xyz);
int gingr_nicp_solve(gingr_ctx *ctx, int32_t kind, int64_t n, const double *moving_xyz, int64_t n_edges, const int32_t *edges,
                     const double *w, const double *cp_xyz, int32_t n_lm, const int32_t *lm_ids, const double *lm_target_xyz, double alpha,
                     double beta, double gamma, double *out_xyz, double *out_lm_xyz);

/* The same step past dense sizes: a handle over the template's edge graph, and the normal equations solved matrix-free by block-Jacobi
 * preconditioned conjugate gradients (nicp_sparse.hip; the system, its quirks and the arguments are gingr_nicp_solve's).  The handle
 * owns the CSR adjacency on the device and every work vector: a step allocates nothing.  gingr_nicp_create: an edge that is not
 * p1 < p2 < n, a REPEATED edge and a landmark id out of range are GINGR_ERR_BAD_ARGUMENT.  gingr_nicp_step: lm_target_xyz [3L] for the
 * lm_ids given at create (nullable when L = 0).  The three right-hand sides stop when |r| <= rel_tol |b| holds for each of them on the
 * recurrence residual (rel_tol <= 0: 1e-12), or after max_iterations (<= 0: 20 000): then the status is GINGR_ERR_NOT_CONVERGED, with
 * info and the outputs filled from the last iterate.  info (nullable): the iterations taken, converged 0 / 1, and per coordinate the
 * TRUE residual |b - A x| of the returned solution (one more pass behind the stop) and |b|.  A mesh component without any weighted
 * vertex or landmark term, or a vertex block that is not positive definite, is GINGR_ERR_NOT_SPD (nothing is iterated on); a non-finite
 * result GINGR_ERR_NONFINITE.  Two calls with the same input give the same bits.  Synchronises.
 * gingr_nicp_get_solution: the unknowns X of the last step that returned its outputs (GINGR_ERR_STATE without one), row-major
 * [n][3] (N-ICP-T, the displacements) or [4 n][3] (N-ICP-A, row 4 i + a of vertex i), the layout of the reference's `A \ B`. */
typedef struct gingr_nicp gingr_nicp;
typedef struct gingr_nicp_info {
    int32_t iterations;
    int32_t converged;
    double residual[3];
    double rhs_norm[3];
} gingr_nicp_info;
int gingr_nicp_create(gingr_ctx *ctx, int32_t kind, int64_t n, int64_t n_edges, const int32_t *edges, int32_t n_lm, const int32_t *lm_ids,
                      gingr_nicp **out);
void gingr_nicp_destroy(gingr_nicp *h);
int gingr_nicp_step(gingr_nicp *h, const double *moving_xyz, const double *w, const double *cp_xyz, const double *lm_target_xyz, double alpha,
                    double beta, double gamma, double rel_tol, int32_t max_iterations, double *out_xyz, double *out_lm_xyz,
                    gingr_nicp_info *info);
int gingr_nicp_get_solution(gingr_nicp *h, double *x);

#ifdef __cplusplus
}
#endif
#endif /* GINGR_HIP_H */
