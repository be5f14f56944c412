// The 3 x 3 step of the rigid searches, one body for the pose step of rigid_search.hip (search_step_kernel) and the pose of a triple
// of pairs in feature_align.hip (poses_from_triples_kernel): from the sums of the pairs (p_i, y_i) centred on c -- S[0] = n, S[1..3] =
// sum (p - c), S[4..6] = sum (y - c), S[7..15] = sum (y - c)(p - c)^T row-major -- the cross-covariance H = sum / n - mu_y mu_p^T, dR =
// its Kabsch rotation (kabsch3_rotation of svd3.h: the polar factor, else the SVD with the determinant fix) and dt = mu_y - dR mu_p
// in the caller's frame.  Every expression is written out with its brackets: the bits do not depend on who calls.
#pragma once
#include "host_device.h"
#include "svd3.h"

GINGR_HD inline void kabsch_step_from_sums(const double *S, const double c[3], double dR[9], double dt[3]) {
    const double n = S[0];
    double mup[3], muy[3], H[9];
    for (int a = 0; a < 3; ++a) mup[a] = S[1 + a] / n, muy[a] = S[4 + a] / n;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a * 3 + b] = S[7 + a * 3 + b] / n - muy[a] * mup[b];
    double trace = 0.0;
    kabsch3_rotation(H, dR, &trace);
    const double mpa[3] = {mup[0] + c[0], mup[1] + c[1], mup[2] + c[2]};
    for (int a = 0; a < 3; ++a) dt[a] = (muy[a] + c[a]) - ((dR[a * 3] * mpa[0] + dR[a * 3 + 1] * mpa[1]) + dR[a * 3 + 2] * mpa[2]);
}
