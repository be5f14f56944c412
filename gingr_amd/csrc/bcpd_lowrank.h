// The deformation step of the Bayesian coherent point drift over a low-rank factor of the kernel matrix (bcpd_lowrank.hip), for
// bcpd.hip, which owns the handle.  Internal to libgingr_hip.so.
#pragma once

#include "classic_cpd_lowrank.h"

// What a low-rank handle holds in place of G and the M x M system: the factor with its Gram work areas and the k x k system in its
// identity-border form (dense_spd.h).  Nothing here is of size M x M.
struct BcpdLowRank : LowRankFactor {
    DevBuf Aw, Linv;
};

// the factor of lowrank_factor_build over the template Y and the k x k workspace
int bcpd_lowrank_build(gingr_ctx *ctx, Cloud Y, double beta, double relative_tolerance, int32_t max_columns, BcpdLowRank &lr);
// S = L^T diag(nu) L, s = L^T r (lr.svec), C = I + (c2 / lambda) S = R R^T with c2 = params[0]^2 / sc[0] read on the device;
// returns X = R^-T (upper triangular, row stride plan.kp; rows and columns past k: the identity).  `zero`: 3 M zeros.  flags[0] is
// cleared and receives GINGR_ERR_NOT_SPD.  Asynchronous on the context's stream.
const double *bcpd_lowrank_system(gingr_ctx *ctx, BcpdLowRank &lr, const double *nu, const double *r, const double *zero,
                                  const double *params, const double *sc, double lambda, int32_t *flags);
// With wv = X^T s = R^-1 s (three planes of stride plan.kp) and T = L X (never stored):  v^ = (c2 / lambda) T wv,  u^ = y + v^,
// sigma_m^2 = |row m of T|^2 / lambda.  Asynchronous on the context's stream.
void bcpd_lowrank_deform(gingr_ctx *ctx, const BcpdLowRank &lr, const double *X, const double *wv, const double *y, const double *params,
                         const double *sc, double lambda, double *vhat, double *u, double *sig);
