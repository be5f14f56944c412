// The low-rank Maximization of the non-rigid classic CPD (classic_cpd_lowrank.hip), for classic_cpd.hip, which owns the handle.
// Internal to libgingr_hip.so.
#pragma once

#include "common.h"
#include "classic_cpd_lowrank_plan.h"

// What a low-rank handle holds beside the state of the dense one: the factor in the blocked layout of the plan and the work areas of
// the two passes and of the k x k solve.  Nothing here is of size M x M.
struct LowRankCpd {
    lowrank_plan::Plan plan;
    int32_t tolerance_reached = 0;
    double residual_fraction = 0.0;
    DevBuf L;                         // plan.factor_doubles()
    DevBuf gram_part, rhs_part;       // slab partials of the Gram pass
    DevBuf S, svec;                   // L^T D L (kp x kp, both triangles), L^T (P X - D Y) (three planes of stride kp)
    DevBuf Aw, Linv, Z, sysflag;      // the bordered k x k system (dense_spd.h) and its solution z (three planes of stride kp)
    DevBuf apply_part;                // [apply_groups][2]: the sums of the variance update
};

// G ~ L L^T of the Gaussian exp(-|a - b|^2 / (2 beta^2)) over the template Y by the pivoted Cholesky of gpmm.hip, stopped at the
// relative trace tolerance or at max_columns (<= 0: the ceiling lowrank_plan::kMaxColumns), laid out for the passes below.
int lowrank_cpd_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, LowRankCpd &lr);
// One Maximization from the statistics of the Expectation: ty <- ty + L z, W (three planes of stride w_stride), scalars[8] <- sigma2'.
// Asynchronous on the context's stream; *flag receives GINGR_ERR_NOT_SPD / GINGR_ERR_NONFINITE.
void lowrank_cpd_mstep(gingr_ctx *ctx, LowRankCpd &lr, const double *P1, const double *PX, double *ty, double *scalars, double lambda,
                       double *W, int64_t w_stride, int32_t *flag);
// the factor, row-major M x plan.k, on the host
int lowrank_cpd_get_factor(gingr_ctx *ctx, const LowRankCpd &lr, double *out);
