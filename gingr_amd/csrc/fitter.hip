// The device-resident fitter: lifecycle, setters and getters, the small pinned-buffer read-back, and the internal hooks of the
// device group (group.hip) and the RCCL exchange (rccl_exchange.hip).  C ABI in include/gingr_hip.h.  The update itself is in
// fitter_phases.hip, the surface set-up in fitter_surface.hip, the probabilistic path in fitter_mh.hip.
#include "fitter.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

namespace {

// out[0..nblock) = block; out[nblock + 3 perm[i] + d] = fit[d][i].  With `flag`: out is HOST memory (the fitter's pinned buffer through
// its device address); the last workgroup to finish stores `epoch` into *flag behind a system-scope fence, and the host, spinning on
// that word, has the results without a copy launch and without the wake-up of a stream synchronisation (~12 us of a 235 us step).
__global__ __launch_bounds__(256) void mh_readback_kernel(const double *__restrict__ block, int nblock, const double *__restrict__ fit, int64_t M,
                                                         const int32_t *__restrict__ perm, double *__restrict__ out, double *flag,
                                                         int32_t *__restrict__ done, double epoch) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nblock) out[i] = block[i];
    if (fit && i < M) {
        const int64_t o = perm ? perm[i] : i;
        double *dst = out + nblock + 3 * o;
        dst[0] = fit[i];
        dst[1] = fit[M + i];
        dst[2] = fit[2 * M + i];
    }
    if (!flag) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(done, 1) == (int)gridDim.x - 1) {
            *done = 0;  // (the next launch is behind this one in the stream)
            __threadfence_system();
            *reinterpret_cast<volatile double *>(flag) = epoch;
        }
    }
}

}  // namespace

void launch_mh_readback(gingr_ctx *ctx, int64_t n, const double *block, int nblock, const double *fit, int64_t M, const int32_t *perm,
                        double *out, double *flag, int32_t *done, double epoch) {
    hipLaunchKernelGGL(mh_readback_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, block, nblock, fit, M, perm, out, flag,
                       done, epoch);
}

SweepArgs base_args(const gingr_fitter *f) {
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.Q0 = f->m->Q0;
    a.ref = f->m->ref;
    a.mean = f->m->mean;
    a.M = f->m->M;
    a.rp = f->m->rp;
    a.state = f->st;
    a.pose = f->pose;
    a.c0[0] = f->m->c0[0];
    a.c0[1] = f->m->c0[1];
    a.c0[2] = f->m->c0[2];
    a.partial = f->ws;
    return a;
}

// boxes + |coordinate - centre| maximum of a fit that was NOT written by refresh_fit (explicit fit points; a target set after the state)
void fit_boxes_now(gingr_fitter *f) {
    if (!f->fboxes) return;
    (void)hipMemsetAsync(f->absmax + 1, 0, sizeof(double), f->ctx->stream);
    launch_tile_bbox(f->ctx, cloud_of(f->fit, f->m->M), f->fboxes, f->absmax + 2, f->absmax + 1);
    f->fit_boxes_valid = true;
}

// fit = modelInstanceShapePoseScale(model, state)
void refresh_fit(gingr_fitter *f, bool compact) {
    SweepArgs a = base_args(f);
    a.coef0 = f->alpha;
    a.shape_out = f->fit;
    if (f->fboxes && f->m->rp <= 512 && f->cpd_seen) {  // the pass also leaves the quarter boxes and the |coordinate - centre| maximum
        if (compact) a.Qc = f->m->Qc, a.sep_map = f->m->sep_map;  // (only the quarter-box form has a compact instance)
        a.qboxes = f->fboxes + 6 * ceil_div(f->m->M, 256);
        a.box_centre = f->absmax + 2;
        a.absmax_slot = f->absmax + 1;
        launch_sweep(f->ctx, SWEEP_FIT, a);
        f->fit_boxes_valid = true;
    } else {
        launch_sweep(f->ctx, SWEEP_FIT, a);
        f->fit_boxes_valid = false;
        if (f->cpd_seen) fit_boxes_now(f);  // rank > 512: the generic pass, the boxes by a launch of their own
    }
}

int check_ready(gingr_fitter *f) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    if (!f->target) return gingr_set_error(f->ctx, GINGR_ERR_STATE, "update: no target set (gingr_fitter_set_target)");
    if (!f->has_state) return gingr_set_error(f->ctx, GINGR_ERR_STATE, "update: no state set (gingr_fitter_set_state)");
    if (hipSetDevice(f->ctx->device) != hipSuccess) return gingr_set_error(f->ctx, GINGR_ERR_HIP, "hipSetDevice failed");
    return GINGR_OK;
}

// ready, then the parameter rules of correspondence.h with the texts the entry points have always answered with
int check_parameters(gingr_fitter *f, const Correspondence &c) {
    GINGR_TRY(check_ready(f));
    switch (correspondence_error(c)) {
        case CorrespondenceError::None: return GINGR_OK;
        case CorrespondenceError::CpdParams: return gingr_set_error(f->ctx, GINGR_ERR_BAD_ARGUMENT, "cpd params: need 0 <= w < 1 and lambda > 0");
        case CorrespondenceError::IcpParams: return gingr_set_error(f->ctx, GINGR_ERR_BAD_ARGUMENT, "icp params: max_iterations < 1");
        case CorrespondenceError::BadFlavour: break;
    }
    return gingr_set_error(f->ctx, GINGR_ERR_BAD_ARGUMENT, "correspondence flavour %d out of range", (int)c.kind);
}

// ... then what the flavour needs of the fitter (the order of correspondence.h)
int check_correspondence(gingr_fitter *f, const Correspondence &c) {
    GINGR_TRY(check_parameters(f, c));
    if (needs_meshes(c) && (!f->Tm || !f->Tt)) return gingr_set_error(f->ctx, GINGR_ERR_STATE, "icp surface: no meshes set (gingr_fitter_set_meshes)");
    if (c.kind == Flavour::Pairs) GINGR_TRY(pairs_ensure_planes(f));  // (no gingr_fitter_set_pairs yet: no pairs)
    return GINGR_OK;
}

std::vector<double> state_key_values(int32_t r, const double *alpha, const double euler[3], const double center[3], const double t[3],
                                     double scale, double sigma2) {
    std::vector<double> v(alpha, alpha + r);
    for (int q = 0; q < 3; ++q) v.push_back(euler[q]);
    for (int q = 0; q < 3; ++q) v.push_back(center[q]);
    for (int q = 0; q < 3; ++q) v.push_back(t[q]);
    v.push_back(scale);
    v.push_back(sigma2);
    return v;
}

void scalars_of_state(const DevState &hst, gingr_state_scalars *s) {
    for (int q = 0; q < 3; ++q) {
        s->euler[q] = hst.euler[q];
        s->center[q] = hst.center[q];
        s->translation[q] = hst.t[q];
    }
    s->scale = hst.scale;
    s->sigma2 = hst.sigma2;
    s->iteration = hst.iteration;
    s->status = hst.status;
}

// The host side of mh_readback_kernel's flag: spin on the word, look at the clock every 1024 spins, give up 2 s after the call.  The
// acquire fence orders the reads of the pinned buffer behind the flag.  Not seen = a launch that never finished or a buffer the host
// does not see coherently: the caller's stream synchronisation reports the one and covers the other.
bool wait_pinned_flag(const PinnedWords &w, double epoch) {
    volatile double *flag = w.pin + w.pin_doubles - 1;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
    bool seen = false;
    for (unsigned spins = 0;; ++spins) {
        if (*flag == epoch) {
            seen = true;
            break;
        }
        if ((spins & 1023u) == 1023u) {
            if (std::chrono::steady_clock::now() > deadline) break;
            if (spins > 65536u) std::this_thread::yield();  // (a long wait: leave the core to whoever else needs it)
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return seen;
}

static PinnedWords pinned_words_of(const gingr_fitter *f) { return PinnedWords{f->pin, f->pin_doubles, f->pin_dev, f->mh_done, f->mh_epoch}; }

bool wait_pinned_flag(gingr_fitter *f, double epoch) { return wait_pinned_flag(pinned_words_of(f), epoch); }

// n doubles from the device into the pinned buffer at `dst` (a pointer INTO w.pin) without a copy + stream synchronisation: one small
// launch writes them through the buffer's device address and stores the launch number into the flag word, the host spins on it (see
// mh_readback_kernel).  Everything enqueued before on the stream is complete when this returns.
int pull_small(gingr_ctx *ctx, PinnedWords &w, const double *src, int n, double *dst) {
    if (!w.pin_dev) {
        HIP_TRY(ctx, hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return GINGR_OK;
    }
    const double epoch = (double)(++w.epoch);
    launch_mh_readback(ctx, n, src, n, nullptr, 0, nullptr, w.pin_dev + (dst - w.pin), w.pin_dev + w.pin_doubles - 1, w.done, epoch);
    GINGR_TRY(check_launch(ctx));
    if (!wait_pinned_flag(w, epoch)) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int pull_small(gingr_fitter *f, const double *src, int n, double *dst) {
    PinnedWords w = pinned_words_of(f);
    const int rc = pull_small(f->ctx, w, src, n, dst);
    f->mh_epoch = w.epoch;
    return rc;
}

extern "C" {

int gingr_fitter_create(gingr_ctx *ctx, const gingr_model *model, gingr_fitter **out) {
    if (!ctx || !model || !out) return GINGR_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!model->finalized)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "fitter_create: sharded model not finalized (gingr_model_finalize)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gingr_fitter *f = new gingr_fitter();
    f->ctx = ctx;
    f->m = model;
    const int64_t M = model->M;
    const int32_t rp = model->rp;
    int rc;
    if ((rc = dev_alloc(ctx, &f->fit, (size_t)3 * M)) || (rc = dev_alloc(ctx, &f->P1, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->PX, (size_t)3 * M)) || (rc = dev_alloc(ctx, &f->nn_idx, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->nn_d2, (size_t)M)) || (rc = dev_alloc(ctx, &f->weight, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->zero_counts, (size_t)ceil_div(M, 256))) ||
        (rc = dev_alloc(ctx, &f->evec, (size_t)3 * M)) || (rc = dev_alloc(ctx, &f->newshape, (size_t)3 * M)) ||
        (rc = dev_alloc(ctx, &f->state_block, (size_t)rp + kScalarsDoubles + kDevStateDoubles + 8)) || (rc = dev_alloc(ctx, &f->acoef, (size_t)rp)) ||
        (rc = dev_alloc(ctx, &f->fxbuf[0], (size_t)rp * rp + 2 * rp)) || (rc = dev_alloc(ctx, &f->fxbuf[1], (size_t)rp * rp + 2 * rp)) ||
        (rc = dev_alloc(ctx, &f->nfac[0], (size_t)(rp + 16) * rp)) || (rc = dev_alloc(ctx, &f->nfac[1], (size_t)(rp + 16) * rp)) ||
        (rc = dev_alloc(ctx, &f->alt_seg, (size_t)rp * rp + 2 * rp + 8)) || (rc = dev_alloc(ctx, &f->lp_sync, (size_t)2)) ||
        (rc = dev_alloc(ctx, &f->alpha_c, (size_t)rp)) || (rc = dev_alloc(ctx, &f->zbuf, (size_t)PostVec::kZRows * rp)) || (rc = dev_alloc(ctx, &f->zrand, (size_t)rp)) ||
        (rc = dev_alloc(ctx, &f->pose, 1)) || (rc = dev_alloc(ctx, &f->fit_alt, (size_t)3 * M)) ||
        (rc = dev_alloc(ctx, &f->mh_save, (size_t)rp + kScalarsDoubles + kDevStateDoubles)) ||
        (rc = dev_alloc(ctx, &f->scalars, 8)) || (rc = dev_alloc(ctx, &f->part, GINGR_SCALAR_PART)) || (rc = dev_alloc(ctx, &f->absmax, GINGR_AUX)) || (rc = dev_alloc(ctx, &f->work, (size_t)std::max<int64_t>((int64_t)rp * rp, posterior_work_doubles(rp)))) ||
        (rc = dev_alloc(ctx, &f->lm_mask, (size_t)M))) {
        gingr_fitter_destroy(f);
        return rc;
    }
    f->alpha = f->state_block;
    f->hs_dev = reinterpret_cast<gingr_state_scalars *>(f->state_block + rp);
    f->st = reinterpret_cast<DevState *>(f->state_block + rp + kScalarsDoubles);
    f->small = f->state_block + rp + kScalarsDoubles + kDevStateDoubles;  // behind the state: one transfer brings both back (mh_step)
    f->pin_doubles = (size_t)3 * M + rp + kScalarsDoubles + kDevStateDoubles + 16 + 2;  // (+ the eight results of gingr_fitter_mh_step, + its flag)
    if (hipHostMalloc(reinterpret_cast<void **>(&f->pin), f->pin_doubles * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        f->pin = nullptr;
        gingr_fitter_destroy(f);
        return gingr_set_error(ctx, GINGR_ERR_HIP, "fitter_create: pinned host buffer");
    }
    if ((rc = dev_alloc(ctx, &f->retry, 1)) || (rc = dev_alloc(ctx, &f->mh_done, 1))) {
        gingr_fitter_destroy(f);
        return rc;
    }
    f->pin[f->pin_doubles - 1] = 0.0;
    if (hipMemset(f->mh_done, 0, sizeof(int32_t)) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&f->pin_dev), f->pin, 0) != hipSuccess) {
        (void)hipGetLastError();
        f->pin_dev = nullptr;  // (the step then copies its results back as before)
    }
    {
        const int32_t init = GINGR_RETRY_INIT;
        if (hipMemcpy(f->retry, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            gingr_fitter_destroy(f);
            return gingr_set_error(ctx, GINGR_ERR_HIP, "fitter_create: retry counter upload");
        }
    }
    (void)hipMemsetAsync(f->lm_mask, 0, (size_t)M * sizeof(int32_t), ctx->stream);
    (void)hipMemsetAsync(f->alpha, 0, (size_t)rp * sizeof(double), ctx->stream);
    (void)hipMemsetAsync(f->scalars, 0, 8 * sizeof(double), ctx->stream);
    *out = f;
    return GINGR_OK;
}

void gingr_fitter_destroy(gingr_fitter *f) {
    if (!f) return;
    if (f->ctx) {
        (void)hipSetDevice(f->ctx->device);
        (void)hipStreamSynchronize(f->ctx->stream);
    }
    delete f->stat_scratch;
    void *ptrs[] = {f->target, f->inv_den, f->Pt1, f->fit, f->fit_alt, f->mh_save, f->mh_rb, f->mh_done, f->P1, f->PX,
                    f->nn_idx, f->nn_d2, f->weight, f->evec, f->newshape, f->state_block, f->acoef, f->alpha_c, f->zbuf,
                    f->zrand, f->pose, f->scalars, f->fxbuf[0], f->fxbuf[1], f->alt_seg, f->nfac[0], f->nfac[1],
                    f->lp_sync, f->lp_scratch, f->retry, f->part, f->absmax, f->tperm, f->tboxes, f->fboxes,
                    f->tile_bad, f->xch, f->fullfit, f->gstage, f->zero_counts, f->ws, f->work, f->aos, f->lm_pid,
                    f->lm_xyz, f->lm_cov, f->lm_mask, f->tnormals};
    for (void *q : ptrs) dev_free(q);
    if (f->pin) (void)hipHostFree(f->pin);
    if (f->zpin) (void)hipHostFree(f->zpin);
    if (f->zpin_done) (void)hipEventDestroy(f->zpin_done);
    nn_grid_free(&f->tgrid);
    tri_grid_free(&f->ttgrid);
    free_meshes(f);
    free_pairs(f);
    delete f;
}

int gingr_fitter_set_target(gingr_fitter *f, int64_t N, const double *target_xyz) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    f->nn_warm = f->surf_nn_warm = f->surf_tri_warm = false;  // positions in another target (any in-range position would still be a valid start)
    f->forget_posteriors();  // the posterior memos describe other inputs
    gingr_ctx *ctx = f->ctx;
    if (N < 1 || N > INT32_MAX || !target_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_target: bad N");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t M = f->m->M;
    const int32_t rp = f->m->rp;
    void *old[] = {f->target, f->inv_den, f->Pt1, f->xch, f->ws, f->aos, f->tperm, f->tboxes, f->fboxes, f->tile_bad, f->tnormals};
    for (void *q : old) dev_free(q);
    f->tnormals = nullptr;  // (normals of the previous target's points)
    free_meshes(f);  // the target triangles refer to the previous target
    f->target = f->inv_den = f->Pt1 = f->xch = f->ws = f->tboxes = f->fboxes = nullptr;
    f->aos = nullptr;
    f->tperm = f->tile_bad = nullptr;
    f->N = N;
    GINGR_TRY(dev_alloc(ctx, &f->target, (size_t)3 * N));
    GINGR_TRY(dev_alloc(ctx, &f->inv_den, (size_t)N));
    GINGR_TRY(dev_alloc(ctx, &f->Pt1, (size_t)N));
    // exchange segments (float64 elements)
    f->cnt[0] = N;
    f->cnt[1] = (int64_t)rp * rp + rp + 8 + rp;  // G, rhs, the scalar sums, and Q0^T e of a sharded transition-density query
    int64_t o = 0;
    for (int s = 0; s < GINGR_NUM_SEGMENTS; ++s) {
        f->off[s] = o;
        o += round_up(f->cnt[s], 32);  // 256-byte aligned segments
    }
    GINGR_TRY(dev_alloc(ctx, &f->xch, (size_t)o));
    f->seg_swapped = false;  // (the posterior memos were forgotten above: nothing lives in either slot)
    HIP_TRY(ctx, hipMemsetAsync(f->xch, 0, (size_t)o * sizeof(double), ctx->stream));
    int64_t w = cpd_colsum_ws_doubles(M, N);
    auto mx = [&](int64_t v) {
        if (v > w) w = v;
    };
    mx(cpd_rowstats_ws_doubles(M, N));
    mx(ceil_div(nn_ws_bytes(M, N), 8));
    mx(ceil_div(nn_ws_bytes(N, M), 8));  // reversed correspondence direction: the targets query the model vertices
    mx(gram_ws_doubles(M, rp) + sweep_ws_doubles(M, rp));  // phase 1 keeps both sets of partials until its finalize kernel
    if (f->m->Qc) mx(gram_compact_ws_doubles(M));           // (the compact pass: Gram and right-hand-side partials in one block)
    f->ws_doubles = w;
    GINGR_TRY(dev_alloc(ctx, &f->ws, (size_t)w));
    const int64_t big = M > N ? M : N;
    double *aos = nullptr;
    GINGR_TRY(dev_alloc(ctx, &aos, (size_t)3 * big));
    f->aos = aos;
    HIP_TRY(ctx, hipMemcpyAsync(aos, target_xyz, (size_t)3 * N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    kd_leaf_order(target_xyz, N, f->h_tperm);
    GINGR_TRY(nn_grid_build(ctx, target_xyz, N, f->h_tperm.data(), M, &f->tgrid));
    GINGR_TRY(dev_alloc(ctx, &f->tperm, (size_t)N));
    HIP_TRY(ctx, hipMemcpyAsync(f->tperm, f->h_tperm.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GINGR_TRY(dev_alloc(ctx, &f->tboxes, (size_t)ceil_div(N, 256) * 30));  // tile boxes + four quarter boxes per tile
    GINGR_TRY(dev_alloc(ctx, &f->fboxes, (size_t)ceil_div(M, 256) * 30));
    f->fit_boxes_valid = false;
    GINGR_TRY(dev_alloc(ctx, &f->tile_bad, (size_t)ceil_div(N, 256)));
    launch_aos_to_soa(ctx, aos, N, f->target, f->tperm);
    launch_tile_bbox(ctx, cloud_of(f->target, N), f->tboxes);
    launch_cloud_centroid(ctx, cloud_of(f->target, N), f->absmax + 2);
    launch_cloud_absmax(ctx, cloud_of(f->target, N), f->absmax + 2, f->absmax);
    if (f->has_state) fit_boxes_now(f);  // the fit on the device predates this target (its centre)
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GINGR_OK;
}

int gingr_fitter_set_landmarks(gingr_fitter *f, int32_t n_lm, const int32_t *lm_pid, const double *lm_xyz,
                               const double *lm_cov) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    f->forget_posteriors();  // the posterior memos describe other inputs
    gingr_ctx *ctx = f->ctx;
    if (n_lm < 0 || (n_lm > 0 && (!lm_pid || !lm_xyz || !lm_cov)))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_landmarks: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    dev_free(f->lm_pid);
    dev_free(f->lm_xyz);
    dev_free(f->lm_cov);
    f->lm_pid = nullptr;
    f->lm_xyz = f->lm_cov = nullptr;
    f->n_lm = n_lm;
    const int64_t M = f->m->M;
    std::vector<int32_t> mask((size_t)M, 0), local((size_t)(n_lm > 0 ? n_lm : 1), -1);
    for (int32_t l = 0; l < n_lm; ++l) {
        if (lm_pid[l] < 0 || lm_pid[l] >= f->m->M_total)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_landmarks: point id %d out of range", lm_pid[l]);
        const int64_t lp = (int64_t)lm_pid[l] - f->m->row_begin;
        if (lp >= 0 && lp < M) {
            const int32_t pos = f->m->hiperm[(size_t)lp];  // device (Morton) position of the original point
            local[(size_t)l] = pos;
            mask[(size_t)pos] = 1;
        }
    }
    HIP_TRY(ctx, hipMemcpy(f->lm_mask, mask.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice));
    // host copies for the pairs flavour: its covariance pairs share the landmark launch (fitter_pairs.hip)
    f->h_lm_mask = mask;
    f->h_lm_row.assign(local.begin(), local.begin() + n_lm);
    f->h_lm_xyz.clear(), f->h_lm_cov.clear();
    if (n_lm > 0) {
        f->h_lm_xyz.assign(lm_xyz, lm_xyz + (size_t)3 * n_lm);
        f->h_lm_cov.assign(lm_cov, lm_cov + (size_t)9 * n_lm);
    }
    if (f->n_pc > 0) GINGR_TRY(pairs_rebuild_cov_list(f));
    if (n_lm > 0) {
        GINGR_TRY(dev_alloc(ctx, &f->lm_pid, (size_t)n_lm));
        GINGR_TRY(dev_alloc(ctx, &f->lm_xyz, (size_t)3 * n_lm));
        GINGR_TRY(dev_alloc(ctx, &f->lm_cov, (size_t)9 * n_lm));
        HIP_TRY(ctx, hipMemcpy(f->lm_pid, local.data(), (size_t)n_lm * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(f->lm_xyz, lm_xyz, (size_t)3 * n_lm * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(f->lm_cov, lm_cov, (size_t)9 * n_lm * sizeof(double), hipMemcpyHostToDevice));
    }
    return GINGR_OK;
}

int gingr_fitter_set_options(gingr_fitter *f, int32_t global_transform, double step_length) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    if (global_transform < 0 || global_transform > 2)
        return gingr_set_error(f->ctx, GINGR_ERR_BAD_ARGUMENT, "set_options: unknown global transformation %d", global_transform);
    f->global_transform = global_transform;
    f->step_length = step_length;
    return GINGR_OK;
}

int gingr_fitter_set_stop_threshold(gingr_fitter *f, double threshold) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (threshold != threshold) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_stop_threshold: NaN");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    f->stop_threshold = threshold < 0.0 ? -1.0 : threshold;
    f->stop_hit = 0;
    // a state the rule stopped at earlier takes updates again
    if (f->has_state) HIP_TRY(ctx, hipMemsetAsync(&f->st->stopped, 0, sizeof(int32_t), ctx->stream));
    return GINGR_OK;
}

int gingr_fitter_stop_rule_hit(gingr_fitter *f, int32_t *hit) {
    if (!f || !hit) return GINGR_ERR_BAD_ARGUMENT;
    *hit = f->stop_hit;
    return GINGR_OK;
}

int gingr_fitter_last_update_error(gingr_fitter *f, int32_t *code) {
    if (!f || !code) return GINGR_ERR_BAD_ARGUMENT;
    *code = f->last_err;
    return GINGR_OK;
}

int gingr_fitter_set_state(gingr_fitter *f, const double *alpha, const gingr_state_scalars *s) {
    if (!f || !alpha || !s) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t r = f->m->r, rp = f->m->rp;
    memset(f->pin, 0, ((size_t)rp + kScalarsDoubles) * sizeof(double));
    memcpy(f->pin, alpha, (size_t)r * sizeof(double));
    memcpy(f->pin + rp, s, sizeof(*s));
    HIP_TRY(ctx, hipMemcpyAsync(f->state_block, f->pin, ((size_t)rp + kScalarsDoubles) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_state_init(ctx, f->st, f->hs_dev, f->absmax + 1);
    if (!f->ws) {  // no target yet: allocate the sweep workspace so the fit can be instantiated
        f->ws_doubles = sweep_ws_doubles(f->m->M, rp);
        GINGR_TRY(dev_alloc(ctx, &f->ws, (size_t)f->ws_doubles));
    }
    refresh_fit(f);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    f->has_state = true;
    f->mh_saved = false;
    f->state_key.v = state_key_values(r, alpha, s->euler, s->center, s->translation, s->scale, s->sigma2);
    f->state_key_valid = true;
    return GINGR_OK;
}

int gingr_fitter_set_fit_points(gingr_fitter *f, const double *fit_xyz) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!fit_xyz) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_fit_points: null argument");
    if (!f->has_state) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_fit_points: set a state first (its pose / sigma2 stay in force)");
    if (!f->aos) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_fit_points: set a target first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    double *stage = reinterpret_cast<double *>(f->aos);
    HIP_TRY(ctx, hipMemcpyAsync(stage, fit_xyz, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, stage, M, f->fit, f->m->perm);
    fit_boxes_now(f);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller's buffer is free again
    // the shape on the device is no instance of the model any more: nothing memoised describes it
    f->forget_posteriors();
    f->state_key_valid = false;
    f->mh_saved = false;
    return GINGR_OK;
}

int gingr_fitter_get_state(gingr_fitter *f, double *alpha, gingr_state_scalars *s, double *fit_xyz) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!f->has_state) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_state: no state set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    const int32_t rp_ = f->m->rp;
    const size_t head = (size_t)rp_ + kScalarsDoubles + kDevStateDoubles;  // [alpha | scalars | DevState], one transfer
    bool seen = false;
    if (f->pin_dev && M <= 8192) {
        // small templates: one launch gathers state and fit straight into the pinned buffer and the call spins on the flag word (as
        // gingr_fitter_mh_step does) instead of two copies, a reordering launch and a stream synchronisation
        const double epoch = (double)(++f->mh_epoch);
        const int64_t n = fit_xyz ? std::max<int64_t>(M, (int64_t)head) : (int64_t)head;
        launch_mh_readback(ctx, n, f->state_block, (int)head, fit_xyz ? f->fit : nullptr, M, f->m->perm, f->pin_dev, f->pin_dev + f->pin_doubles - 1,
                           f->mh_done, epoch);
        GINGR_TRY(check_launch(ctx));
        seen = wait_pinned_flag(f, epoch);
        if (!seen) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that never finished: the error is reported here)
    }
    if (!seen) HIP_TRY(ctx, hipMemcpyAsync(f->pin, f->state_block, head * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DevBuf tmp;
    if (fit_xyz && !seen) {
        double *stage = reinterpret_cast<double *>(f->aos);  // the fitter's interleaved staging buffer (max(3M, 3N) doubles)
        if (!stage) {                                        // no target yet: a temporary
            HIP_TRY(ctx, tmp.alloc((size_t)3 * M * sizeof(double)));
            stage = tmp.as<double>();
        }
        launch_soa_to_aos(ctx, f->fit, M, stage, f->m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(f->pin + head, stage, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!seen) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DevState hst;
    memcpy(&hst, f->pin + rp_ + kScalarsDoubles, sizeof(hst));
    if (alpha) memcpy(alpha, f->pin, (size_t)f->m->r * sizeof(double));
    if (fit_xyz) memcpy(fit_xyz, f->pin + head, (size_t)3 * M * sizeof(double));
    if (s) scalars_of_state(hst, s);
    f->stop_hit = hst.stopped;
    f->last_err = hst.pad;
    if (alpha) {  // what was just read IS the device state: the posterior memo can recognise it without a gingr_fitter_set_state
        f->state_key.v = state_key_values(f->m->r, alpha, hst.euler, hst.center, hst.t, hst.scale, hst.sigma2);
        f->state_key_valid = true;
    }
    return GINGR_OK;
}

int gingr_fitter_get_cpd_stats(gingr_fitter *f, double *P1, double *PX, double *den, double *scalars6) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (f->corr_stale)  // see gingr_fitter::alt_seg
        return gingr_set_error(ctx, GINGR_ERR_STATE, "get_cpd_stats: a probabilistic query brought another state's posterior back; the correspondences on the device are not this state's -- run an update or a phase first");
    if (!f->target) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_cpd_stats: no target");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    DevBuf tmp, tmp1, tmpd;
    if (P1) {  // back to the caller's point order
        HIP_TRY(ctx, tmp1.alloc((size_t)M * sizeof(double)));
        launch_scatter(ctx, f->P1, M, f->m->perm, tmp1.as<double>());
        HIP_TRY(ctx, hipMemcpyAsync(P1, tmp1.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (PX) {
        HIP_TRY(ctx, tmp.alloc((size_t)3 * M * sizeof(double)));
        launch_soa_to_aos(ctx, f->PX, M, tmp.as<double>(), f->m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(PX, tmp.p, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (den) {
        HIP_TRY(ctx, tmpd.alloc((size_t)f->N * sizeof(double)));
        launch_scatter(ctx, f->xch + f->off[0], f->N, f->tperm, tmpd.as<double>());
        HIP_TRY(ctx, hipMemcpyAsync(den, tmpd.p, (size_t)f->N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    double sc[8];
    const double *red = f->seg1_live() + (int64_t)f->m->rp * f->m->rp + f->m->rp;
    HIP_TRY(ctx, hipMemcpyAsync(sc, red, sizeof(sc), hipMemcpyDeviceToHost, ctx->stream));
    double loc[8];
    HIP_TRY(ctx, hipMemcpyAsync(loc, f->scalars, sizeof(loc), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (scalars6) {
        for (int q = 0; q < 4; ++q) scalars6[q] = sc[q];
        scalars6[4] = (sc[1] - 2 * sc[2] + sc[3]) / (sc[0] * 3.0);
        scalars6[5] = loc[5];
    }
    return GINGR_OK;
}

int gingr_fitter_get_icp_idx(gingr_fitter *f, int32_t *idx, double *d2) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (f->corr_stale)  // see gingr_fitter::alt_seg
        return gingr_set_error(ctx, GINGR_ERR_STATE, "get_icp_idx: a probabilistic query brought another state's posterior back; the correspondences on the device are not this state's -- run an update or a phase first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    std::vector<int32_t> hidx((size_t)M);
    std::vector<double> hd2((size_t)M);
    HIP_TRY(ctx, hipMemcpyAsync(hidx.data(), f->nn_idx, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hd2.data(), f->nn_d2, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // device positions -> the caller's numbering (rows and targets are kept in Morton order on the device)
    for (int64_t sidx = 0; sidx < M; ++sidx) {
        const int32_t row = f->m->hperm[(size_t)sidx];
        const int32_t pos = hidx[(size_t)sidx];
        if (idx) idx[row] = (pos >= 0 && (size_t)pos < f->h_tperm.size()) ? f->h_tperm[(size_t)pos] : -1;
        if (d2) d2[row] = hd2[(size_t)sidx];
    }
    return GINGR_OK;
}

int gingr_fitter_retry_counter(gingr_fitter *f, int32_t set_to, int32_t *value_out) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (set_to >= 0) HIP_TRY(ctx, hipMemcpyAsync(f->retry, &set_to, sizeof(set_to), hipMemcpyHostToDevice, ctx->stream));
    int32_t v = set_to;
    if (value_out && set_to < 0) HIP_TRY(ctx, hipMemcpyAsync(&v, f->retry, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (value_out) *value_out = v;
    return GINGR_OK;
}

int gingr_fitter_exchange(gingr_fitter *f, void **dev_ptr, int64_t offsets[GINGR_NUM_SEGMENTS],
                          int64_t counts[GINGR_NUM_SEGMENTS]) {
    if (!f || !dev_ptr) return GINGR_ERR_BAD_ARGUMENT;
    if (!f->xch) return gingr_set_error(f->ctx, GINGR_ERR_STATE, "exchange: no target set");
    *dev_ptr = f->xch;
    for (int s = 0; s < GINGR_NUM_SEGMENTS; ++s) {
        if (offsets) offsets[s] = f->off[s];
        if (counts) counts[s] = f->cnt[s];
    }
    return GINGR_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------- internal hooks (group.hip)
void fitter_set_partial_output(gingr_fitter *f, double *base) { f->partial_out = base; }
void fitter_set_group_member(gingr_fitter *f) { f->group_member = true; }
void fitter_set_partial_fullfit(gingr_fitter *f, double *base) { f->partial_fullfit = base; }
double *fitter_fullfit(gingr_fitter *f) { return f->fullfit; }
void fitter_set_partial_revsum(gingr_fitter *f, double *base) { f->partial_revsum = base; }
double *fitter_revsum(gingr_fitter *f) { return f->revsum; }
// z (r standard normals, host) -> f->zrand (rp doubles, zero padded) on the context's stream, without waiting for the stream
int fitter_upload_zrand(gingr_fitter *f, const double *z) {
    gingr_ctx *ctx = f->ctx;
    const size_t bytes = (size_t)f->m->rp * sizeof(double);
    if (!f->zpin) {
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&f->zpin), bytes, hipHostMallocDefault));
        if (hipEventCreateWithFlags(&f->zpin_done, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(f->zpin);
            f->zpin = nullptr, f->zpin_done = nullptr;
            return gingr_set_error(ctx, GINGR_ERR_HIP, "upload of the posterior draws: hipEventCreate failed");
        }
    } else {
        HIP_TRY(ctx, hipEventSynchronize(f->zpin_done));  // the previous upload has read the buffer (long ago, in practice)
    }
    memset(f->zpin, 0, bytes);
    memcpy(f->zpin, z, (size_t)f->m->r * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(f->zrand, f->zpin, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(f->zpin_done, ctx->stream));
    return GINGR_OK;
}
int fitter_set_zrand(gingr_fitter *f, const double *z) {
    f->zrand_active = false;
    if (!z) return GINGR_OK;
    GINGR_TRY(fitter_upload_zrand(f, z));
    f->zrand_active = true;  // only once the draws are on their way: a failed upload must not sample from stale ones
    return GINGR_OK;
}
gingr_ctx *fitter_ctx(gingr_fitter *f) { return f->ctx; }
// this shard's rows are shard `rank` of the balanced partition over `world` shards, and it has the gathered-fit buffer (pure check)
bool fitter_gather_possible(gingr_fitter *f, int32_t world, int32_t rank) {
    if (!f || !f->fullfit || world < 1 || rank < 0 || rank >= world) return false;
    const gingr_model *m = f->m;
    const int64_t Mt = m->M_total, base = Mt / world, extra = Mt % world;
    const int64_t b = rank * base + (rank < extra ? rank : extra), e = b + base + (rank < extra ? 1 : 0);
    return b == m->row_begin && e - b == m->M;
}
int fitter_gather_agreed(gingr_fitter *f, int32_t world) { return f->gather_agreed_world == world ? f->gather_agreed : -1; }
void fitter_set_gather_agreed(gingr_fitter *f, int32_t world, int agreed) {
    f->gather_agreed = agreed;
    f->gather_agreed_world = world;
}
bool fitter_reversed(gingr_fitter *f) { return f->reversed; }
const gingr_model *fitter_model(gingr_fitter *f) { return f->m; }
