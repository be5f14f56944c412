// The low-rank Maximization of the non-rigid classic CPD (classic_cpd_lowrank.hip), for classic_cpd.hip, which owns the handle.
// Internal to libgingr_hip.so.
#pragma once

#include "common.h"
#include "classic_cpd_lowrank_plan.h"

// The factor of the kernel matrix in the blocked layout of the plan, with the work areas of the weighted Gram pass over it: what every
// consumer of G ~ L L^T holds (this file's Maximization; the deformation step of bcpd_lowrank.hip).  Nothing here is of size M x M.
struct LowRankFactor {
    lowrank_plan::Plan plan;
    int32_t tolerance_reached = 0;
    double residual_fraction = 0.0;
    DevBuf L;                         // plan.factor_doubles()
    DevBuf gram_part, rhs_part;       // slab partials of the Gram pass
    DevBuf S, svec;                   // L^T D L (kp x kp, both triangles), L^T (P X - D Y) (three planes of stride kp)
};

// What a low-rank handle of the classic CPD holds beside the state of the dense one: the factor, the k x k solve and the apply pass.
struct LowRankCpd : LowRankFactor {
    DevBuf Aw, Linv, Z, sysflag;      // the bordered k x k system (dense_spd.h) and its solution z (three planes of stride kp)
    DevBuf apply_part;                // [apply_groups][2]: the sums of the variance update
};

// G ~ L L^T of the Gaussian exp(-|a - b|^2 / (2 beta^2)) over the template Y by the pivoted Cholesky of gpmm.hip, stopped at the
// relative trace tolerance or at max_columns (<= 0: the ceiling lowrank_plan::kMaxColumns), laid out for the passes below, and the
// work areas of the Gram pass.  `who` names the caller in the text of a refusal.
int lowrank_factor_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, const char *who,
                         LowRankFactor &lr);
// the same, and the work areas of the classic Maximization
int lowrank_cpd_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, LowRankCpd &lr);
// Pass 1 over the factor: lr.S = L^T diag(P1) L, lr.svec = L^T (PX - diag(P1) ty).  Asynchronous on the context's stream.
void lowrank_gram(gingr_ctx *ctx, LowRankFactor &lr, const double *P1, const double *PX, const double *ty);
// One Maximization from the statistics of the Expectation: ty <- ty + L z, W (three planes of stride w_stride), scalars[8] <- sigma2'.
// Asynchronous on the context's stream; *flag receives GINGR_ERR_NOT_SPD / GINGR_ERR_NONFINITE.
void lowrank_cpd_mstep(gingr_ctx *ctx, LowRankCpd &lr, const double *P1, const double *PX, double *ty, double *scalars, double lambda,
                       double *W, int64_t w_stride, int32_t *flag);
// the factor, row-major M x plan.k, on the host
int lowrank_cpd_get_factor(gingr_ctx *ctx, const LowRankFactor &lr, double *out);
