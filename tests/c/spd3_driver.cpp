// Host driver of the 3 x 3 SPD inverse (gingr_amd/csrc/svd3.h: spd3_inverse) for tests/test_landmark_system_host.py: reads 3 x 3 matrices
// (nine float64 each, row-major, raw bytes) from stdin until it ends, and writes the nine float64 of the inverse per matrix to stdout.
// Built as the host pass of the HIP compiler only: host arithmetic, no device.  Its own main, so that it can be built and run with the
// address and undefined-behaviour sanitizers.
#include <cstdio>

#include "svd3.h"

int main() {
    double C[9], Ci[9];
    while (fread(C, sizeof(double), 9, stdin) == 9) {
        spd3_inverse(C, Ci);
        if (fwrite(Ci, sizeof(double), 9, stdout) != 9) return 1;
    }
    return 0;
}
