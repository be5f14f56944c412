// Host driver of the 3 x 3 rotation step (gingr_amd/csrc/svd3.h) for tests/test_rotation_step_host.py: reads 3 x 3 matrices (nine
// float64 each, row-major, raw bytes) from stdin until it ends, and writes 42 float64 per matrix to stdout:
//   U[9] s[3] V[9] of svd3 | accepted (1 / 0), R[9], trace of polar3_rotation (zeros where it declined) | R[9], trace of kabsch3_rotation
// Built as the host pass of the HIP compiler only: host arithmetic, no device.
#include <cstdio>

#include "svd3.h"

int main() {
    double A[9];
    while (fread(A, sizeof(double), 9, stdin) == 9) {
        double out[42];
        for (int q = 0; q < 42; ++q) out[q] = 0.0;
        svd3(A, out, out + 9, out + 12);
        double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tr = 0.0;
        if (polar3_rotation(A, R, &tr)) {
            out[21] = 1.0;
            for (int q = 0; q < 9; ++q) out[22 + q] = R[q];
            out[31] = tr;
        }
        kabsch3_rotation(A, out + 32, out + 41);
        if (fwrite(out, sizeof(double), 42, stdout) != 42) return 1;
    }
    return 0;
}
