// Stand-alone caller of the symmetric eigen-solver (gingr_amd/csrc/sym_eig.hip: sym_eig, sym_eig_strided) for tests/test_gpu_sym_eig.py:
// g++, libgingr_hip.so and the HIP runtime, no Python in the process.  The two entries are C++ functions of the library, not part of
// its C boundary; they are declared here as gp.h declares them (gp.h holds device code and cannot be read by g++), so a declaration
// that has drifted is an undefined symbol at link time.  The context comes from gingr_ctx_create; device memory is hipMalloc'ed and
// copied with blocking hipMemcpy (both entries synchronise the context's stream before they return).
//
//   sym_eig_driver IN OUT
//
// IN   int64 calls; per call: int64 entry (0 sym_eig, 1 sym_eig_strided), int64 blocks, int64 count; per problem: int64 n, int64 ldg,
//      double [ldg * ldg] (row stride ldg; sym_eig_strided takes no stride: every problem of its call has one n and ldg = n)
// OUT  per call: int64 return code, int64 length of the error text, the text (gingr_last_error after a non-zero code, else empty);
//      per problem double evals [n], double Vs [n * n].  The outputs are NaN before the call, so what a call leaves unwritten shows.
// A call that fails is recorded and the next one runs on the same context.  Exit code 0 when every call was made and written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "gingr_hip.h"

int sym_eig(gingr_ctx *ctx, int count, const double *const *G, const int32_t *ldg, const int32_t *n, double *const *evals,
            double *const *Vs, bool blocks);
int sym_eig_strided(gingr_ctx *ctx, int count, const double *G, int32_t n, double *evals, double *Vs);

namespace {

constexpr int64_t kMaxN = 512, kMaxStrided = 64;

#define HIP_OR_DIE(expr)                                                                         \
    do {                                                                                         \
        const hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                                  \
            fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__);       \
            return 4;                                                                            \
        }                                                                                        \
    } while (0)

bool read_i64(FILE *f, int64_t *v, int count) { return fread(v, sizeof(int64_t), (size_t)count, f) == (size_t)count; }

struct DevMem {
    void *p = nullptr;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    double *d() const { return static_cast<double *>(p); }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    gingr_ctx *ctx = nullptr;
    const int rc0 = gingr_ctx_create(0, &ctx);
    if (rc0 != GINGR_OK) {
        fprintf(stderr, "gingr_ctx_create: %d\n", rc0);
        return 3;
    }
    int64_t calls = 0;
    if (!read_i64(in, &calls, 1) || calls < 0) return 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < calls; ++c) {
        int64_t head[3];
        if (!read_i64(in, head, 3)) return 2;
        const int64_t entry = head[0], blocks = head[1], count = head[2];
        if (entry < 0 || entry > 1 || count < 1 || count > (entry == 0 ? 3 : kMaxStrided)) {
            fprintf(stderr, "call %lld: entry %lld, count %lld\n", (long long)c, (long long)entry, (long long)count);
            return 2;
        }
        std::vector<int32_t> n((size_t)count), ldg((size_t)count);
        std::vector<std::vector<double>> host((size_t)count);
        for (int64_t q = 0; q < count; ++q) {
            int64_t dims[2];
            if (!read_i64(in, dims, 2)) return 2;
            if (dims[0] < 1 || dims[0] > kMaxN || dims[1] < dims[0] || dims[1] > kMaxN + 64 ||
                (entry == 1 && (dims[1] != dims[0] || dims[0] != (q ? n[0] : dims[0])))) {
                fprintf(stderr, "call %lld problem %lld: n %lld, ldg %lld\n", (long long)c, (long long)q, (long long)dims[0], (long long)dims[1]);
                return 2;
            }
            n[(size_t)q] = (int32_t)dims[0], ldg[(size_t)q] = (int32_t)dims[1];
            host[(size_t)q].resize((size_t)(dims[1] * dims[1]));
            if (fread(host[(size_t)q].data(), sizeof(double), host[(size_t)q].size(), in) != host[(size_t)q].size()) return 2;
        }
        // one allocation each for the inputs, the eigenvalues and the eigenvectors of the call, problem after problem
        std::vector<int64_t> g_at((size_t)count + 1, 0), e_at((size_t)count + 1, 0), v_at((size_t)count + 1, 0);
        for (int64_t q = 0; q < count; ++q) {
            g_at[(size_t)q + 1] = g_at[(size_t)q] + (int64_t)ldg[(size_t)q] * ldg[(size_t)q];
            e_at[(size_t)q + 1] = e_at[(size_t)q] + n[(size_t)q];
            v_at[(size_t)q + 1] = v_at[(size_t)q] + (int64_t)n[(size_t)q] * n[(size_t)q];
        }
        DevMem dG, dE, dV;
        HIP_OR_DIE(hipMalloc(&dG.p, (size_t)g_at[(size_t)count] * sizeof(double)));
        HIP_OR_DIE(hipMalloc(&dE.p, (size_t)e_at[(size_t)count] * sizeof(double)));
        HIP_OR_DIE(hipMalloc(&dV.p, (size_t)v_at[(size_t)count] * sizeof(double)));
        std::vector<double> hE((size_t)e_at[(size_t)count], nan), hV((size_t)v_at[(size_t)count], nan);
        for (int64_t q = 0; q < count; ++q)
            HIP_OR_DIE(hipMemcpy(dG.d() + g_at[(size_t)q], host[(size_t)q].data(), host[(size_t)q].size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_OR_DIE(hipMemcpy(dE.p, hE.data(), hE.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_OR_DIE(hipMemcpy(dV.p, hV.data(), hV.size() * sizeof(double), hipMemcpyHostToDevice));
        int rc;
        if (entry == 0) {
            const double *G[3];
            double *E[3], *V[3];
            for (int64_t q = 0; q < count; ++q) G[q] = dG.d() + g_at[(size_t)q], E[q] = dE.d() + e_at[(size_t)q], V[q] = dV.d() + v_at[(size_t)q];
            rc = sym_eig(ctx, (int)count, G, ldg.data(), n.data(), E, V, blocks != 0);
        } else {
            rc = sym_eig_strided(ctx, (int)count, dG.d(), n[0], dE.d(), dV.d());
        }
        const char *text = rc != GINGR_OK ? gingr_last_error(ctx) : "";
        if (!text) text = "";
        // (a failed call may have left the device in an error state: the copies back say so)
        HIP_OR_DIE(hipMemcpy(hE.data(), dE.p, hE.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OR_DIE(hipMemcpy(hV.data(), dV.p, hV.size() * sizeof(double), hipMemcpyDeviceToHost));
        const int64_t words[2] = {rc, (int64_t)strlen(text)};
        bool ok = fwrite(words, sizeof(int64_t), 2, out) == 2 && fwrite(text, 1, (size_t)words[1], out) == (size_t)words[1];
        for (int64_t q = 0; q < count && ok; ++q) {
            const size_t ne = (size_t)n[(size_t)q], nv = ne * ne;
            ok = fwrite(hE.data() + e_at[(size_t)q], sizeof(double), ne, out) == ne && fwrite(hV.data() + v_at[(size_t)q], sizeof(double), nv, out) == nv;
        }
        if (!ok) {
            fprintf(stderr, "call %lld: short write\n", (long long)c);
            return 5;
        }
    }
    gingr_ctx_destroy(ctx);
    fclose(in);
    return fclose(out) == 0 ? 0 : 5;
}
