// The probabilistic path of the fitter: sampled updates, the transition density (single shard and the two halves of a row shard),
// and one Metropolis-Hastings step per native call with its restore (C ABI in include/gingr_hip.h).
#ifdef GINGR_MH_TRACE
#include <chrono>
#include <cstdio>
#endif
#include "fitter.h"

#include <algorithm>
#include <cmath>

namespace {

// ---- one Metropolis-Hastings step: small transfers as kernels (round 5).  A blit copy on this stack costs 4-8 us on the device
// timeline with the barrier packets around it; the step had 4.7 of them.  (a) the proposal's draws / parameters travel in the
// kernel's ARGUMENT (<= 160 doubles) and the same launch parks the current state; (b) the state block, the eight results and the
// fit (original order, interleaved) are gathered into ONE buffer for ONE device-to-host copy.
constexpr int kMhPayload = 160;
struct MhPayload {
    double v[kMhPayload];
};
// save[0..m) = src[0..m), THEN dst[0..n) = payload (dst may be src: the random-walk parameters overwrite the state block that was just parked)
// st != nullptr: the payload was [alpha | scalars] of a random-walk proposal -- the device state is initialised from it in the same launch
// (state_init_kernel's work: one launch less per such step)
__global__ __launch_bounds__(256) void mh_begin_kernel(MhPayload payload, int n, double *dst, const double *src, int m, double *__restrict__ save,
                                                       DevState *st, const gingr_state_scalars *hs, double *zero_slot) {
    const int t = threadIdx.x;
    double keep = 0.0;
    if (t < m) keep = src[t];
    __syncthreads();
    if (t < m) save[t] = keep;
    if (t < n) dst[t] = payload.v[t];
    if (st) {
        __syncthreads();  // (the scalars just written by this workgroup are read back by its thread 0)
        if (t == 0) state_init_body(st, hs, zero_slot);
    }
}

// pose <- rigid part of the state (scale 1): the frame a mesh is projected in by the transition-density query
__global__ void pose_of_state_kernel(const DevState *__restrict__ st, DevPose *__restrict__ pose) {
    const int t = threadIdx.x;
    if (t < 9) pose->R[t] = st->R[t];
    if (t < 3) {
        pose->euler[t] = st->euler[t];
        pose->t[t] = st->t[t];
        pose->center[t] = st->center[t];
    }
    if (t == 0) pose->scale = 1.0;
}

}  // namespace

// ------------------------------------------------------------------------------------------ probabilistic proposal
int fitter_sample_update(gingr_fitter *f, const Correspondence &c, const double *z) {
    GINGR_TRY(check_correspondence(f, c));
    gingr_ctx *ctx = f->ctx;
    if (!z) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "update_sample: z is null");
    if (f->m->M != f->m->M_total) return gingr_set_error(ctx, GINGR_ERR_STATE, "update_sample: single shard only");
    // (this entry point returns without synchronising: the draws go through the fitter's own event-guarded pinned buffer, not
    // through `pin`, which the synchronous entry points rewrite)
    GINGR_TRY(fitter_upload_zrand(f, z));
    f->zrand_active = true;
    int rc = GINGR_OK;
    f->allow_alt = true;
    for (int ph = 0; ph < GINGR_NUM_PHASES && rc == GINGR_OK; ++ph) rc = fitter_run_phase(f, c, ph);
    f->allow_alt = false;
    f->zrand_active = false;
    return rc;
}

int fitter_posterior_logpdf(gingr_fitter *f, const Correspondence &c, const double *mesh_xyz, double *logpdf) {
    GINGR_TRY(check_correspondence(f, c));
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (!mesh_xyz || !logpdf) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "posterior_logpdf: null argument");
    if (m->M != m->M_total) return gingr_set_error(ctx, GINGR_ERR_STATE, "posterior_logpdf: single shard only");
    const int64_t M = m->M;
    const int32_t r = m->r, rp = m->rp;
    // posterior of the current state: correspondences, Gram, right-hand side (phases 0 and 1 do not touch the state)
    GINGR_TRY(fitter_posterior_inputs(f, c));
    if (f->lp_epoch == 0) HIP_TRY(ctx, hipMemsetAsync(f->lp_sync, 0, 2 * sizeof(unsigned), ctx->stream));  // before the first hand-over
    const bool cached = f->fx_valid[f->live];  // this state's factors are on the device: only the mesh-dependent part is left
    double *G = f->seg1_live();
    double *rhs = G + (int64_t)rp * rp;
    // Q0^T e with e = R^T(mesh - c - t) - (ref - c) - mean in the pose of the state (copied on the device, no host round trip)
    double *out2 = f->small;
    double *aos = reinterpret_cast<double *>(f->aos);
    memcpy(f->pin, mesh_xyz, (size_t)3 * M * sizeof(double));  // pinned: the copy is a plain asynchronous DMA
    HIP_TRY(ctx, hipMemcpyAsync(aos, f->pin, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos, M, f->newshape, m->perm);
    hipLaunchKernelGGL(pose_of_state_kernel, dim3(1), dim3(64), 0, ctx->stream, f->st, f->pose);
    SweepArgs a = base_args(f);
    a.shape_in = f->newshape;
    a.out = f->alpha_c;
    launch_sweep(ctx, SWEEP_PROJ2, a);
    // one kernel: posterior coefficients a = (I + G)^-1 rhs, then the ridge projection of the mesh and its log-density
    GINGR_TRY(launch_posterior_logpdf(ctx, r, rp, G, rhs, m->mom + MomentLayout{rp}.stot(), f->alpha_c, f->fxbuf[f->live], cached, f->work,
                                      out2, f->lp_sync, ++f->lp_epoch));
    GINGR_TRY(check_launch(ctx));
    double *res = f->pin + (size_t)3 * M;  // behind the mesh (pin holds 3M + rp + ... doubles)
    GINGR_TRY(pull_small(f, out2, 2, res));
    if (res[1] != 0.0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "posterior_logpdf: posterior of the current state failed");
    if (!std::isfinite(res[0])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "posterior_logpdf: non-finite result");
    if (f->post_stage == 2) f->fx_valid[f->live] = true;  // (not memoised: sharded / state unknown to the host -> nothing to key it by)
    *logpdf = res[0];
    return GINGR_OK;
}

extern "C" {

int gingr_fitter_update_cpd_sample_async(gingr_fitter *f, const gingr_cpd_params *p, const double *z) {
    return fitter_sample_update(f, abi_correspondence(0, p, nullptr), z);
}
int gingr_fitter_update_icp_sample_async(gingr_fitter *f, const gingr_icp_params *p, const double *z) {
    return fitter_sample_update(f, abi_correspondence(1, nullptr, p), z);
}
int gingr_fitter_update_icp_surface_sample_async(gingr_fitter *f, const gingr_icp_params *p, const double *z) {
    return fitter_sample_update(f, abi_correspondence(2, nullptr, p), z);
}
int gingr_fitter_update_pairs_sample_async(gingr_fitter *f, const double *z) {
    return fitter_sample_update(f, abi_correspondence(3, nullptr, nullptr), z);
}

int gingr_fitter_posterior_logpdf_cpd(gingr_fitter *f, const gingr_cpd_params *p, const double *mesh_xyz, double *logpdf) {
    return fitter_posterior_logpdf(f, abi_correspondence(0, p, nullptr), mesh_xyz, logpdf);
}
int gingr_fitter_posterior_logpdf_icp(gingr_fitter *f, const gingr_icp_params *p, const double *mesh_xyz, double *logpdf) {
    return fitter_posterior_logpdf(f, abi_correspondence(1, nullptr, p), mesh_xyz, logpdf);
}
int gingr_fitter_posterior_logpdf_icp_surface(gingr_fitter *f, const gingr_icp_params *p, const double *mesh_xyz, double *logpdf) {
    return fitter_posterior_logpdf(f, abi_correspondence(2, nullptr, p), mesh_xyz, logpdf);
}
int gingr_fitter_posterior_logpdf_pairs(gingr_fitter *f, const double *mesh_xyz, double *logpdf) {
    return fitter_posterior_logpdf(f, abi_correspondence(3, nullptr, nullptr), mesh_xyz, logpdf);
}

}  // extern "C"

// ---- transition density on a row shard: the two halves around the exchange of segment 1 (the device group drives them itself)
// prepare: this shard's rows of the mesh (host, the FULL mesh in the caller's point order) -> e = R^T (mesh - c - t) - (ref - c) - mean
// in the pose of the state -> the partial Q0^T e into the tail of exchange segment 1 (summed with the Gram bundle).
int fitter_logpdf_prepare(gingr_fitter *f, const double *mesh_xyz_full) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    const int32_t rp = m->rp;
    double *aos = reinterpret_cast<double *>(f->aos);
    memcpy(f->pin, mesh_xyz_full + 3 * m->row_begin, (size_t)3 * M * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(aos, f->pin, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_aos_to_soa(ctx, aos, M, f->newshape, m->perm);
    hipLaunchKernelGGL(pose_of_state_kernel, dim3(1), dim3(64), 0, ctx->stream, f->st, f->pose);
    SweepArgs a = base_args(f);
    a.shape_in = f->newshape;
    a.out = (f->partial_out ? f->partial_out : f->xch) + f->off[1] + (int64_t)rp * rp + rp + 8;
    launch_sweep(ctx, SWEEP_PROJ2, a);
    return check_launch(ctx);
}

// finish (segment 1 reduced): the replicated log-density kernel, read-back, and the tail of segment 1 back to zero
int fitter_logpdf_finish(gingr_fitter *f, double *logpdf) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int32_t r = m->r, rp = m->rp;
    double *G = f->xch + f->off[1];
    double *rhs = G + (int64_t)rp * rp, *qte = rhs + rp + 8;
    double *fx = nullptr;
    unsigned *sync = nullptr;
    unsigned epoch = 0;
    if (rp >= 128) {  // the two factorisations side by side on the super-panel solve (gp.hip: posterior_logpdf_wide_kernel)
        if (!f->lp_scratch) GINGR_TRY(dev_alloc(ctx, &f->lp_scratch, (size_t)rp * rp + 2 * rp));
        if (f->lp_epoch == 0) HIP_TRY(ctx, hipMemsetAsync(f->lp_sync, 0, 2 * sizeof(unsigned), ctx->stream));  // before the first hand-over
        fx = f->lp_scratch, sync = f->lp_sync, epoch = ++f->lp_epoch;
    }
    GINGR_TRY(launch_posterior_logpdf(ctx, r, rp, G, rhs, m->mom + MomentLayout{rp}.stot(), qte, fx, false, f->work, f->small, sync, epoch));
    GINGR_TRY(check_launch(ctx));
    double *res = f->pin + (size_t)3 * m->M;
    // in-place exchanges (RCCL, host callback) would keep adding a stale tail up, so it goes back to zero.  NOT the device group's send
    // buffer: a slower peer may still be reading it (double buffering protects the next WRITE, two exchanges later, not a write now);
    // its stale partial is harmless -- the group's sum is out of place, and updates never read the tail.
    if (!f->partial_out) HIP_TRY(ctx, hipMemsetAsync(qte, 0, (size_t)rp * sizeof(double), ctx->stream));
    GINGR_TRY(pull_small(f, f->small, 2, res));
    if (res[1] != 0.0) return gingr_set_error(ctx, GINGR_ERR_NOT_SPD, "posterior_logpdf: posterior of the current state failed");
    if (!std::isfinite(res[0])) return gingr_set_error(ctx, GINGR_ERR_NONFINITE, "posterior_logpdf: non-finite result");
    *logpdf = res[0];
    return GINGR_OK;
}

// posterior(of the current state).gp.logpdf(posterior.coefficients(mesh)) on a row shard (GeneratorWrapperStochastic.scala:42-63):
// phases 0 and 1 with their exchanges; Q0^T e rides in segment 1; the log-density kernel is replicated.
int fitter_sharded_logpdf(gingr_fitter *f, const Correspondence &c, const double *mesh_xyz_full, gingr_allreduce_fn reduce, void *user,
                          double *logpdf, fitter_gather_fn gather) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (!mesh_xyz_full || !logpdf || !reduce || correspondence_error(c) == CorrespondenceError::BadFlavour)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sharded posterior_logpdf: bad arguments");
    GINGR_TRY(check_correspondence(f, c));
    if (f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "sharded posterior_logpdf: this fitter belongs to a device group");
    if (needs_gathered_fit(c, f->reversed) && f->sharded()) GINGR_TRY(gather_fit(f, c, reduce, user, gather, "sharded posterior_logpdf"));
    GINGR_TRY(fitter_run_phase(f, c, 0));
    if (exchanges_segment0(c) && reduce(user, 0, f->xch + f->off[0], f->cnt[0]) != 0)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "sharded posterior_logpdf: the all-reduce callback failed (segment 0)");
    if (exchanges_reversal_sums(c, f->reversed) && f->sharded() && reduce(user, GINGR_SEGMENT_REVSUM, f->revsum, 4 * f->m->M_total) != 0)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "sharded posterior_logpdf: the all-reduce callback failed (reversal sums)");
    GINGR_TRY(fitter_run_phase(f, c, 1));
    GINGR_TRY(fitter_logpdf_prepare(f, mesh_xyz_full));
    if (reduce(user, 1, f->xch + f->off[1], f->cnt[1]) != 0)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "sharded posterior_logpdf: the all-reduce callback failed (segment 1)");
    return fitter_logpdf_finish(f, logpdf);
}

extern "C" {

int gingr_fitter_posterior_logpdf_sharded(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                          const double *mesh_xyz_full, gingr_allreduce_fn reduce, void *user, double *logpdf) {
    return fitter_sharded_logpdf(f, abi_correspondence(flavour, cp, ip), mesh_xyz_full, reduce, user, logpdf);
}

// ------------------------------------------------------------------------------------------ one Metropolis-Hastings step
// What MetropolisHastings.next asks of the device for ONE step of GingrAlgorithm.run's chain (G/api/GingrAlgorithm.scala:115-190,
// generators/GeneratorWrapperStochastic.scala:28-63, evaluators/IndependentPointDistanceEvaluator.scala:54-70), enqueued as one
// sequence with one synchronisation at the end:
//   x  = the device state                         (its posterior inputs come from the memo: every state's are computed once)
//   x' = update(x, probabilistic = true) with z   (kind 0)   or   the parameters the host's random walk proposes (kind 1)
//   q(x'|x)  = posterior(x).logpdf(coefficients(x.fit))       -- with step length 1 the reference projects from.fit, NOT to.fit
//              (GeneratorWrapperStochastic.scala:50-55): a function of x alone, so only asked for when the host does not hold it
//   posterior inputs of x' (correspondences, Gram, right-hand side)
//   L(x')    = sum over the first n fit vertices of log N(|v - closest point of the target surface|; 0, sdev)
//              -- with the surface correspondence these distances ARE the ones the correspondences of x' just measured
//   q(x|x')  = posterior(x').logpdf(coefficients(x'.fit))     -- the q(.|x') of every later step that starts from x'
// The host decides; a rejection is gingr_fitter_mh_restore (x becomes the device state again, nothing waits).
static void mh_tag_state(gingr_fitter *f) {
    f->state_key.v.assign({-1.2345678901234567e300, (double)++f->mh_serial});
    f->state_key_valid = true;
}

static int mh_logpdf_enqueue(gingr_fitter *f, const DevState *frame, const double *mesh_soa, double *out2, bool keep_factor) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int32_t r = m->r, rp = m->rp;
    double *G = f->seg1_live(), *rhs = G + (int64_t)rp * rp;
    if (f->lp_epoch == 0) HIP_TRY(ctx, hipMemsetAsync(f->lp_sync, 0, 2 * sizeof(unsigned), ctx->stream));
    const bool cached = f->fx_valid[f->live];
    SweepArgs a = base_args(f);
    a.frame = frame;
    a.shape_in = mesh_soa;
    a.out = f->alpha_c;
    launch_sweep(ctx, SWEEP_PROJ2, a);
    const bool split = !cached && rp <= 112;  // (launch_posterior_logpdf's own choice: the two-workgroup form also leaves the factor of I + G)
    GINGR_TRY(launch_posterior_logpdf(ctx, r, rp, G, rhs, m->mom + MomentLayout{rp}.stot(), f->alpha_c, f->fxbuf[f->live], cached, f->work, out2,
                                      f->lp_sync, ++f->lp_epoch, keep_factor, f->nfac[f->live]));
    if (split && f->post_stage == 2) f->nf_valid[f->live] = true;
    // (taken back after the synchronisation when the kernel reports a failure; ranks above 112 always leave the factor behind)
    if (f->post_stage == 2 && (keep_factor || rp > 112)) f->fx_valid[f->live] = true;
    return check_launch(ctx);
}

#ifdef GINGR_MH_TRACE  // diagnostic build only (tools/mkvar.sh mhtrace fitter_mh -DGINGR_MH_TRACE): where the host side of a step goes
static double g_mh_t[4];  // between calls, enqueue, wait, after the wait (seconds)
static long g_mh_n;
static std::chrono::steady_clock::time_point g_mh_last;
static bool g_mh_has_last;
struct MhTrace {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t1, t2;
    MhTrace() {
        if (g_mh_has_last) g_mh_t[0] += std::chrono::duration<double>(t0 - g_mh_last).count();
    }
    ~MhTrace() {
        const auto t3 = std::chrono::steady_clock::now();
        g_mh_t[1] += std::chrono::duration<double>(t1 - t0).count();
        g_mh_t[2] += std::chrono::duration<double>(t2 - t1).count();
        g_mh_t[3] += std::chrono::duration<double>(t3 - t2).count();
        g_mh_last = t3, g_mh_has_last = true;
        if (++g_mh_n % 100 == 0)
            fprintf(stderr, "mh_step x%ld: between calls %.1f us, enqueue %.1f, wait %.1f, after %.1f\n", g_mh_n, 1e6 * g_mh_t[0] / g_mh_n,
                    1e6 * g_mh_t[1] / g_mh_n, 1e6 * g_mh_t[2] / g_mh_n, 1e6 * g_mh_t[3] / g_mh_n);
    }
};
#endif

int gingr_fitter_mh_step(gingr_fitter *f, const gingr_mh_request *q, double *alpha_out, double *fit_out, gingr_mh_result *res) {
#ifdef GINGR_MH_TRACE
    MhTrace trace;
#endif
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (!q || !res || !alpha_out || q->flavour < 0 || q->flavour > 2 || (q->kind != 0 && q->kind != 1) || !(q->eval_sdev > 0.0) ||
        q->eval_points < 0 || q->eval_points > m->M || (q->flavour == 0 ? !q->cpd : !q->icp) || (q->kind == 0 ? !q->z : (!q->alpha || !q->scalars)))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mh_step: bad request");
    const Correspondence c = abi_correspondence(q->flavour, q->cpd, q->icp);
    GINGR_TRY(check_parameters(f, c));
    if (m->M != m->M_total || f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "mh_step: single shard only");
    // (the likelihood of a step is measured on the surfaces, whatever the flavour: the surface flavour's precondition with this entry
    // point's own text; there is no step for the pairs flavour)
    if (!f->Tm || !f->Tt) return gingr_set_error(ctx, GINGR_ERR_STATE, "mh_step: no meshes set (gingr_fitter_set_meshes)");
    if (f->step_length != 1.0) return gingr_set_error(ctx, GINGR_ERR_STATE, "mh_step: step length 1 only (the transition density projects from.fit)");
    if (!f->state_key_valid)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "mh_step: the device state is not one the host set or read (gingr_fitter_set_state)");
    const int64_t M = m->M;
    const int32_t r = m->r, rp = m->rp;
    const size_t head = (size_t)rp + kScalarsDoubles + kDevStateDoubles;
    int rc = GINGR_OK;
    f->allow_alt = true;
    struct Restore {  // whatever happens below, the entry-point-scoped switches go back
        gingr_fitter *f;
        ~Restore() { f->allow_alt = false, f->zrand_active = false; }
    } restore{f};
    // (1) the posterior inputs of x (memo: they exist unless x is the first state of the chain)
    for (int ph = 0; ph < 2 && rc == GINGR_OK; ++ph) rc = fitter_run_phase(f, c, ph);
    GINGR_TRY(rc);
    // (2) x stays: parameters + device state in mh_save (parked by the launch that also brings the proposal's draws / parameters, or
    // by a copy where those do not fit a kernel argument), the fit by exchanging the two fit buffers
    const bool by_kernel = (size_t)rp + kScalarsDoubles <= (size_t)kMhPayload && head <= 256;
    if (!by_kernel) HIP_TRY(ctx, hipMemcpyAsync(f->mh_save, f->state_block, head * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    f->mh_key = f->state_key;
    std::swap(f->fit, f->fit_alt);
    // From here on the device state is in flux (fit pointers exchanged, state block and memo keys about to be rewritten): a failure
    // on the way must not leave something behind that the next mh_step / mh_restore would take for a consistent state -- the
    // caller is sent back through gingr_fitter_set_state.
    struct Poison {
        gingr_fitter *f;
        bool armed = true;
        ~Poison() {
            if (!armed) return;
            f->state_key_valid = false;
            f->mh_saved = false;
            f->forget_posteriors();
        }
    } poison{f};
    const DevState *x_state = reinterpret_cast<const DevState *>(f->mh_save + rp + kScalarsDoubles);
    // (3) the proposal
    memset(f->pin, 0, ((size_t)rp + kScalarsDoubles) * sizeof(double));
    MhPayload payload;
    if (by_kernel) memset(&payload, 0, sizeof(payload));
    if (q->kind == 0) {
        if (by_kernel) {
            memcpy(payload.v, q->z, (size_t)r * sizeof(double));
            hipLaunchKernelGGL(mh_begin_kernel, dim3(1), dim3(256), 0, ctx->stream, payload, (int)rp, f->zrand, f->state_block, (int)head, f->mh_save,
                               (DevState *)nullptr, (const gingr_state_scalars *)nullptr, (double *)nullptr);
        } else {
            memcpy(f->pin, q->z, (size_t)r * sizeof(double));
            HIP_TRY(ctx, hipMemcpyAsync(f->zrand, f->pin, (size_t)rp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        }
        f->zrand_active = true;
        rc = fitter_run_phase(f, c, 2);
        f->zrand_active = false;
        GINGR_TRY(rc);
        mh_tag_state(f);
    } else {
        if (by_kernel) {
            memcpy(payload.v, q->alpha, (size_t)r * sizeof(double));
            memcpy(payload.v + rp, q->scalars, sizeof(*q->scalars));
            hipLaunchKernelGGL(mh_begin_kernel, dim3(1), dim3(256), 0, ctx->stream, payload, (int)(rp + kScalarsDoubles), f->state_block, f->state_block,
                               (int)head, f->mh_save, f->st, (const gingr_state_scalars *)f->hs_dev, f->absmax + 1);
        } else {
            memcpy(f->pin, q->alpha, (size_t)r * sizeof(double));
            memcpy(f->pin + rp, q->scalars, sizeof(*q->scalars));
            HIP_TRY(ctx, hipMemcpyAsync(f->state_block, f->pin, ((size_t)rp + kScalarsDoubles) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            launch_state_init(ctx, f->st, f->hs_dev, f->absmax + 1);
        }
        refresh_fit(f);
        GINGR_TRY(check_launch(ctx));
        const gingr_state_scalars *s = q->scalars;  // the host knows this state: keyed by value, like gingr_fitter_set_state
        f->state_key.v = state_key_values(r, q->alpha, s->euler, s->center, s->translation, s->scale, s->sigma2);
        f->state_key_valid = true;
    }
    // (4) q(x'|x): the live posterior slot still holds x; frame and mesh of x
    const int slot_fw = f->live;
    if (q->need_forward) GINGR_TRY(mh_logpdf_enqueue(f, x_state, f->fit_alt, f->small, true));
    // (5) the posterior inputs of x' (x's are parked in the second slot)
    rc = fitter_run_phase(f, c, 0);
    const bool memo_hit = f->skip_phase1;
    if (rc == GINGR_OK) rc = fitter_run_phase(f, c, 1);
    GINGR_TRY(rc);
    // (6) the likelihood of x'
    if (!f->stat_scratch) f->stat_scratch = new StatScratch;
    StatScratch &sc = *f->stat_scratch;
    HIP_TRY(ctx, ensure(sc.part, (size_t)distance_stats_ws_doubles() * sizeof(double)));
    const double *d2 = f->surf_d2;
    if (!(c.kind == Flavour::IcpSurface && !memo_hit && !f->reversed && f->surface_method == 0)) {  // no fresh closest-point scan of x' to share
        const Cloud fit = cloud_of(f->fit, M), tgt = cloud_of(f->target, f->N);
        HIP_TRY(ctx, ensure(sc.cp, (size_t)3 * M * sizeof(double)));
        HIP_TRY(ctx, ensure(sc.d2, (size_t)M * sizeof(double)));
        HIP_TRY(ctx, ensure(sc.pos, (size_t)M * sizeof(int32_t)));
        const bool warm = sc.pos_K == M && sc.pos_T == f->Tt && sc.pos_tri == f->ttri;
        launch_surface_closest_point(ctx, fit, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttboxes, sc.cp.as<double>(), sc.d2.as<double>(), nullptr,
                                     sc.pos.as<int32_t>(), warm, f->ttribox);
        sc.pos_K = M, sc.pos_T = f->Tt, sc.pos_tri = f->ttri;
        d2 = sc.d2.as<double>();
    }
    const bool all = q->eval_points == 0 || q->eval_points == M;
    launch_distance_stats(ctx, M, d2, all ? nullptr : m->perm, q->eval_points, nullptr, nullptr, q->eval_sdev, sc.part.as<double>(), f->small + 4);
    // (7) q(x|x'): frame, posterior and mesh of x'
    const int slot_bw = f->live;
    // (this state's density is asked for once: the host keeps the number, so the factor need not be left behind)
    GINGR_TRY(mh_logpdf_enqueue(f, f->st, f->fit, f->small + 2, false));
    // (8) ONE transfer back: [alpha | scalars | DevState] of x', the eight results (small follows the state block) and, on request, the fit,
    // gathered by one launch
    // Small results (always) and the fit of small templates go straight into the pinned buffer, the host spins on the flag word; the
    // fit of a large template (scattered 24-byte stores over the host link) keeps the gather on the device + one copy.
    const bool direct = f->pin_dev != nullptr && (!fit_out || M <= 8192);
    if (!direct && !f->mh_rb) GINGR_TRY(dev_alloc(ctx, &f->mh_rb, head + 8 + (size_t)3 * M));
    const double epoch = (double)(++f->mh_epoch);
    const int64_t n = fit_out ? std::max<int64_t>(M, (int64_t)head + 8) : (int64_t)head + 8;
    const double *fit = fit_out ? f->fit : nullptr;
    if (direct) {
        launch_mh_readback(ctx, n, f->state_block, (int)(head + 8), fit, M, m->perm, f->pin_dev, f->pin_dev + f->pin_doubles - 1, f->mh_done, epoch);
    } else {
        launch_mh_readback(ctx, n, f->state_block, (int)(head + 8), fit, M, m->perm, f->mh_rb, nullptr, nullptr, 0.0);
        HIP_TRY(ctx, hipMemcpyAsync(f->pin, f->mh_rb, (head + 8 + (fit_out ? (size_t)3 * M : 0)) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    GINGR_TRY(check_launch(ctx));
#ifdef GINGR_MH_TRACE
    trace.t1 = std::chrono::steady_clock::now();
#endif
    // spin on the flag; a launch that never finishes (a fault) is left to the stream synchronisation below to report
    const bool seen = direct && wait_pinned_flag(f, epoch);
    if (!seen) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
#ifdef GINGR_MH_TRACE
    trace.t2 = std::chrono::steady_clock::now();
#endif
    poison.armed = false;
    f->mh_saved = true;
    DevState hst;
    memcpy(&hst, f->pin + rp + kScalarsDoubles, sizeof(hst));
    memcpy(alpha_out, f->pin, (size_t)r * sizeof(double));
    if (fit_out) memcpy(fit_out, f->pin + head + 8, (size_t)3 * M * sizeof(double));
    memset(res, 0, sizeof(*res));
    scalars_of_state(hst, &res->scalars);
    const double *o = f->pin + head;
    auto density = [&](const double *v, int slot, double *lp, int32_t *status) {
        *status = v[1] != 0.0 ? GINGR_ERR_NOT_SPD : (std::isfinite(v[0]) ? GINGR_OK : GINGR_ERR_NONFINITE);
        *lp = *status == GINGR_OK ? v[0] : -INFINITY;
        if (*status != GINGR_OK) f->fx_valid[slot] = f->nf_valid[slot] = false;  // nothing usable was left behind for the cached forms
    };
    if (q->need_forward) {
        density(o, slot_fw, &res->log_q_forward, &res->forward_status);
    } else {
        res->log_q_forward = NAN;
        res->forward_status = -1;  // not asked for
    }
    density(o + 2, slot_bw, &res->log_q_backward, &res->backward_status);
    res->dist_sum = o[4];
    res->dist_max = o[5];
    res->count = (int64_t)o[6];
    res->log_value = o[7];
    if (q->kind == 0) {  // the host now knows the state the update produced: value key, so that set_state of the same numbers finds its memo
        gingr_fitter::Key k = f->state_key;
        k.v = state_key_values(r, alpha_out, hst.euler, hst.center, hst.t, hst.scale, hst.sigma2);
        if (f->post_stage == 2 && f->post_key.v == f->state_key.v) f->post_key.v = k.v;
        if (f->alt_stage == 2 && f->alt_key.v == f->state_key.v) f->alt_key.v = k.v;
        f->state_key.v = k.v;
    }
    return GINGR_OK;
}

int gingr_fitter_mh_restore(gingr_fitter *f) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (!f->mh_saved) return gingr_set_error(ctx, GINGR_ERR_STATE, "mh_restore: no gingr_fitter_mh_step since the state was last set");
    const size_t head = (size_t)f->m->rp + kScalarsDoubles + kDevStateDoubles;
    HIP_TRY(ctx, hipMemcpyAsync(f->state_block, f->mh_save, head * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    refresh_fit(f);  // (recomputed rather than taken from fit_alt: the pass also leaves the boxes the CPD passes prune with)
    GINGR_TRY(check_launch(ctx));
    f->state_key = f->mh_key;
    f->state_key_valid = true;
    f->mh_saved = false;
    return GINGR_OK;
}

}  // extern "C"
