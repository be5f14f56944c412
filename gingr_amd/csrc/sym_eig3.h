// Eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi rotations, and the normal it gives a point neighbourhood
// (cloud_knn.hip: cloud_normals_kernel).  Plain C++ for host and device: tests/c/cloud_knn_plan_driver.cpp runs it on the CPU.  Every
// index is a compile-time constant, so on the device the matrices stay in registers.
#pragma once

#include "host_device.h"

#include <cmath>

namespace sym_eig3 {

constexpr int kMaxSweeps = 16;  // a 3 x 3 matrix converges in 4-6 sweeps; the loop ends at the first sweep that finds nothing to rotate

// one rotation in the plane (P, Q) of A (symmetric, full storage) accumulated into the columns of V; R: the third index
template <int P, int Q, int R>
GINGR_HD inline bool rotate(double A[3][3], double V[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return false;
    // an off-diagonal entry that no longer changes either diagonal entry is taken for zero (Rutishauser)
    const double g = 128.0 * fabs(apq);
    if (fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) {
        A[P][Q] = A[Q][P] = 0.0;
        return false;
    }
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const double vip = V[i][P], viq = V[i][Q];
        V[i][P] = c * vip - s * viq;
        V[i][Q] = s * vip + c * viq;
    }
    return true;
}

// exchange eigenpairs I and J when lam[I] > lam[J]
template <int I, int J>
GINGR_HD inline void order(double lam[3], double V[3][3]) {
    if (!(lam[I] > lam[J])) return;
    const double l = lam[I];
    lam[I] = lam[J], lam[J] = l;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const double v = V[i][I];
        V[i][I] = V[i][J], V[i][J] = v;
    }
}

// c6 = {xx, xy, xz, yy, yz, zz}  ->  lam[0] <= lam[1] <= lam[2], column j of V the unit eigenvector of lam[j].  A diagonal matrix comes
// back as it is (no rotation, V a permutation of the identity): exact zeros stay exact.
GINGR_HD inline void eigh(const double c6[6], double lam[3], double V[3][3]) {
    double A[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    V[0][0] = V[1][1] = V[2][2] = 1.0;
    V[0][1] = V[0][2] = V[1][0] = V[1][2] = V[2][0] = V[2][1] = 0.0;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool any = rotate<0, 1, 2>(A, V);
        any = rotate<0, 2, 1>(A, V) || any;
        any = rotate<1, 2, 0>(A, V) || any;
        if (!any) break;
    }
    lam[0] = A[0][0], lam[1] = A[1][1], lam[2] = A[2][2];
    order<0, 1>(lam, V);
    order<1, 2>(lam, V);
    order<0, 1>(lam, V);
}

// The normal of a neighbourhood with second central moments c6 (this package's definition, include/gingr_hip.h: gingr_cloud_normals):
// the unit eigenvector of the smallest eigenvalue, zero when lam1 - lam0 <= 2^-26 lam2 (coincident points, a line, an isotropic blob:
// the direction has no correct digit); sign: the component of largest magnitude positive, lowest axis on ties.  variation = lam0 /
// trace (Pauly's surface variation), 0 when the trace is 0.
GINGR_HD inline void normal_of(const double c6[6], double n[3], double *variation) {
    double lam[3], V[3][3];
    eigh(c6, lam, V);
    const double trace = (lam[0] + lam[1]) + lam[2];
    *variation = trace != 0.0 ? lam[0] / trace : 0.0;
    n[0] = n[1] = n[2] = 0.0;
    if (lam[1] - lam[0] <= 0x1p-26 * lam[2] || !(trace <= kDblMax)) return;
    double x = V[0][0], y = V[1][0], z = V[2][0];
    const double len = sqrt((x * x + y * y) + z * z);
    x /= len, y /= len, z /= len;
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    if (lead < 0.0) x = -x, y = -y, z = -z;
    n[0] = x, n[1] = y, n[2] = z;
}

}  // namespace sym_eig3
