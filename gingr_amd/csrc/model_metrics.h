// What model_metrics.hip offers to the other translation units (pca_leave_one_out.hip, surface_metrics.hip): shapes as a block of columns
// in the basis layout, the reconstruct-and-measure pass with its finish, the argument checks of the metric entries, the coefficient
// columns of a generalization call and the stored instances.  Internal to libgingr_hip.so.
#pragma once

#include "common.h"
#include "model_metrics_plan.h"

struct RankList {
    int32_t n;
    int32_t k[model_metrics_plan::kMaxRanks];
};

// the argument checks of gingr_model_generalization / _specificity: a complete, finalized model of this context (complete_model_fault,
// gp.h, as GINGR_ERR_STATE for a shard or a model that is not finalized); 1 <= n_ranks <= 16 strictly increasing ranks within the
// model's.  Finite values: check_finite (gp.h).
int metrics_check_model(gingr_ctx *ctx, const gingr_model *m, const char *who);
int metrics_check_ranks(gingr_ctx *ctx, const gingr_model *m, int32_t n_ranks, const int32_t *ranks, const char *who, RankList *out);

// P [3 M + 48][ldt] = ref + mean + Q0 T on ctx->stream, rows in the model's order (the slack rows are the caller's).  T: [rp][ldt],
// ldt a multiple of 16.  Timing hook 20.
void launch_instances(gingr_ctx *ctx, const gingr_model *m, const double *T, int ldt, double *P);
// T [rp][ldt] on the device: column c < cnt = the k leading entries of alphas[c] (device, [cnt][r]), zero elsewhere.  On ctx->stream.
void launch_sample_factor(gingr_ctx *ctx, const double *alphas, int cnt, int r, int k, int rp, int ldt, double *T);

// The front half of a generalization call (nothing synchronises; the struct owns every buffer in flight): D [3 M + 48][np] the centred
// shapes, T [rp][n_ranks np] with column q np + i = alpha_k(q) of shape i, coef [n_ranks][n][r] when wanted, *flag != 0 (device) when
// S_tot / eps + I was not positive definite.
struct RankFactors {
    DevBuf D, ws, C, work, T, coef;
    const int32_t *flag = nullptr;
};
int project_rank_factors(gingr_ctx *ctx, const gingr_model *model, int32_t n, const double *shapes_xyz, const RankList &rl, bool want_coef,
                         RankFactors &f);

// n shapes (host, interleaved xyz, caller's point order) as the columns [0, n) of D [3 M + 48][np]: D[3 s + d][j] = X_j[3 perm[s] + d],
// minus ref[d][s] + mean[d][s] (planes on the device) when `center`; perm == nullptr: the rows keep the caller's order.  The padding
// columns and the slack rows are zero.  Synchronises.
int pack_shape_columns(gingr_ctx *ctx, int64_t M, const int32_t *perm, const double *ref, const double *mean, int n, const double *shapes, bool center,
                       DevBuf &D, int np);

// res (device, 2 n_ranks n doubles): avg [n_ranks][n], then max [n_ranks][n], of |Q0 T - D| per vertex -- column q np + i of the product
// against column i of D; the product is formed on float64 MFMA and never stored.  Q0: [3 M + 48][rp], T: [rp][ldt], ldt = n_ranks np,
// D: [3 M + 48][np].  partial: allocated here (slab partials).  Timing hook 18: the measure pass alone.  On ctx->stream.
int launch_project_measure(gingr_ctx *ctx, const double *Q0, int64_t M, int rp, const double *T, int ldt, const double *D, int np, int n, int n_ranks,
                           DevBuf &partial, double *res);
