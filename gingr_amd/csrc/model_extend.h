// The kernel extension of a model built from a kernel (model_extend.hip): what the GPMM builders leave behind so that the model's basis
// functions can be evaluated at points off its reference.  The pivoted Cholesky reproduces the kernel exactly on its pivot rows, so
//     Q(x)[d, :] = sum_j k_d(x, p_{d,j}) C_d[j, :],      L_P^T C_d = V_d,
// L_P the rows of the factor at coordinate d's pivots (lower triangular in pivot order), V_d the eigenvectors the build kept, scattered
// into the model's columns.  The build keeps device copies of the raw material only (pivots, pivot rows, eigenvectors); the per-coordinate
// lists and C are formed at the first use.  Internal to libgingr_hip.so.
#pragma once

#include "gp.h"
#include "gpmm_factor.h"

// one coordinate's kernel, by value: kinds 0 (Gaussian mixture, mirror), 1 (dot product), 3 (radial terms without weight fields; family
// is the model's own copy of the table the build kept on the device)
struct ExtKernel {
    gpmm_factor::KSpec spec;
    int32_t family[gpmm_factor::kMaxMix];
};

struct KernelExtension {
    bool shared = false;          // one kernel and one pivot sequence for the three coordinates (the scalar factorisation)
    int32_t r = 0, rp = 0;        // the model's columns (rp: padded to 16)
    ExtKernel kernel[3];
    // ---- raw material of the build (released once formed)
    int32_t n = 0;                // pivots of the factorisation
    int32_t cnt[3] = {0, 0, 0};   // pivots per coordinate (shared: known at the build; generic: counted when formed)
    DevBuf raw;                   // one allocation for the five arrays below
    const int32_t *pivots = nullptr;  // [n]: point (shared) or entry 3 point + coordinate (generic), pivot order
    const double *LPt = nullptr;      // [n][n]: LPt[c n + i] = column c of the factor at pivot i
    const double *pxyz = nullptr;     // [3][n] coordinates of the pivots' points
    const double *V[3] = {nullptr, nullptr, nullptr};  // eigenvector blocks, V[b][row vn[b] + column]
    int32_t vn[3] = {0, 0, 0};
    int block_of[3] = {0, 0, 0};  // coordinate -> eigenvector block
    std::vector<int32_t> qdim, qidx;  // shared: column q of the model is eigenvector qidx[q] of coordinate qdim[q]'s block
    // ---- formed
    bool formed = false;
    int32_t np = 0;               // rows of P and C: the largest cnt padded to model_extend_plan::kPivotStep, zero behind cnt[d]
    std::vector<int32_t> ids[3];  // the pivots' points
    DevBuf P[3];                  // [3][np]
    DevBuf C[3];                  // [np][rp]
};

// gpmm.hip: the raw material of a finished factorisation into a new extension -- one allocation, device-to-device copies and one gather
// launch on the context's stream, no synchronisation: the caller keeps the factor and V alive until the stream has been synchronised
// (model_create_impl does).  V / vn: the eigenvector blocks (generic: block 0 alone, n x n); the caller fills kernel, shared, cnt,
// block_of, qdim, qidx, r, rp.
int kernel_extension_keep(gingr_ctx *ctx, const gpmm_factor::Factor &f, int32_t n, bool generic, const double *const V[3], const int32_t vn[3],
                          KernelExtension &ext);
// model.hip (gingr_model_truncate): the extension of src cut to the k leading columns
int kernel_extension_truncate(gingr_ctx *ctx, const gingr_model *src, int32_t k, std::shared_ptr<KernelExtension> *out);
