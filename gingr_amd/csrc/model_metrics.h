// What model_metrics.hip offers to the other translation units (pca_leave_one_out.hip): shapes as a block of columns in the basis layout,
// and the reconstruct-and-measure pass with its finish.  Internal to libgingr_hip.so.
#pragma once

#include "common.h"

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
