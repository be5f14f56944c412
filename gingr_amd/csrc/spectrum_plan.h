// The spectrum cut of the derived-model builders (pca_model.hip, augment_model.hip, localize_model.hip, pca_leave_one_out.hip,
// posterior_model.hip): which leading eigenvalues of a descending spectrum become the variances of the new model.  Plain C++
// (compiled for the host alone by tests/test_spectrum_plan_host.py).
//
// The solvers decompose G + shift I (a centred or summed Gram matrix is singular; pca_model.hip, step 5, has the reasons), so
//   lam_j = max(ev_j - shift, 0)                                  a null direction is rounding around zero
//   k     = the leading j with lam_j > tol lam_0 and lam_j > 0    strictly: an entry equal to the threshold is not kept
//   k    <= min(available, max_rank > 0 ? min(max_rank, 512) : 512)
// `kept` and `total` are the sums of lam over the leading k and over all n, both in ascending index order.  gpmm_plan::conclude keeps
// a rule of its own (a tolerance on the residual trace).
#pragma once

#include "host_device.h"

namespace spectrum_plan {

constexpr int kMaxRank = 512;  // columns of a model (model_create_impl)

GINGR_HD inline double unshift(double ev, double shift) {
    const double lam = ev - shift;
    return lam < 0.0 ? 0.0 : lam;
}

GINGR_HD inline int rank_ceiling(int available, int max_rank) {
    const int cap = max_rank > 0 && max_rank < kMaxRank ? max_rank : kMaxRank;
    return available < cap ? available : cap;
}

// lam: descending, un-shifted, at least kmax entries (host memory, or LDS from device code)
GINGR_HD inline int leading_rank(const double *lam, int kmax, double tol) {
    int k = 0;
    while (k < kmax && lam[k] > tol * lam[0] && lam[k] > 0.0) ++k;
    return k;
}

struct Cut {
    int k;                // kept components
    double kept, total;   // sum of lam[:k], of lam[:n]
    int first_nonfinite;  // index of the first eigenvalue that is not finite, -1: none (the caller refuses)
};

// ev [n] descending: un-shifted in place, then cut
inline Cut cut(double *ev, int n, double shift, int available, int max_rank, double tol) {
    Cut c{0, 0.0, 0.0, -1};
    for (int j = 0; j < n; ++j) {
        if (c.first_nonfinite < 0 && !(ev[j] >= -kDblMax && ev[j] <= kDblMax)) c.first_nonfinite = j;
        ev[j] = unshift(ev[j], shift);
        c.total += ev[j];
    }
    c.k = leading_rank(ev, rank_ceiling(available < n ? available : n, max_rank), tol);
    for (int j = 0; j < c.k; ++j) c.kept += ev[j];
    return c;
}

}  // namespace spectrum_plan
