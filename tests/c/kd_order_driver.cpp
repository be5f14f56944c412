// Host driver of the k-d leaf order (gingr_amd/csrc/kd_order.h) for tests/test_kd_order_host.py.  Raw bytes on stdin and stdout:
//   kd_order_driver <mode> : int64 n, float64 xyz[3 n] -> int32 perm[n]
// mode: serial (no thread of its own), default (the library's setting: threads from 16 384 points on), parallel (the same threads
// from the first point on, so that small clouds take the threaded paths too).
// Plain C++ for the host compiler.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kd_order.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    KdParallel par;
    if (!strcmp(argv[1], "serial"))
        par = KdParallel::serial();
    else if (!strcmp(argv[1], "parallel"))
        par.min_points = 0;
    else if (strcmp(argv[1], "default"))
        return 2;
    int64_t n;
    if (fread(&n, sizeof(n), 1, stdin) != 1 || n < 0) return 1;
    std::vector<double> xyz((size_t)(3 * n));
    if (n && fread(xyz.data(), sizeof(double), xyz.size(), stdin) != xyz.size()) return 1;
    std::vector<int32_t> perm;
    kd_leaf_order(xyz.data(), n, perm, par);
    if ((int64_t)perm.size() != n) return 1;
    return n == 0 || fwrite(perm.data(), sizeof(int32_t), perm.size(), stdout) == perm.size() ? 0 : 1;
}
