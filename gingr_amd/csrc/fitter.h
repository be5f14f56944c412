// Internal header of the fitter family -- model.hip, fitter.hip, fitter_phases.hip, fitter_surface.hip, fitter_mh.hip: the
// device-resident fitter's state and the host helpers more than one of those files needs.  Not part of the C ABI
// (include/gingr_hip.h); the hooks for group.hip and rccl_exchange.hip are declared in gp.h.
#pragma once

#include "gp.h"
#include "surface.h"

#include <cstdlib>
#include <vector>

// what the surface distance statistics keep across calls (fitter_surface.hip: run_distance_stats; fitter_mh.hip: the likelihood of a step)
struct StatScratch {
    DevBuf cp, d2, nn, nnd2, ws, part, out;
    // warm start of the closest-point scan: last call's winning triangle per query, valid for the same number of queries against the
    // same triangle array (successive likelihood evaluations of a chain look at nearby shapes)
    DevBuf pos;
    int64_t pos_K = -1, pos_T = -1;
    const int32_t *pos_tri = nullptr;
};

struct gingr_fitter {
    gingr_ctx *ctx = nullptr;
    const gingr_model *m = nullptr;
    int64_t N = 0;
    double *target = nullptr;  // SoA [3][N]
    double *inv_den = nullptr, *Pt1 = nullptr;
    double *fit = nullptr;  // SoA [3][M]
    double *P1 = nullptr, *PX = nullptr;
    int32_t *nn_idx = nullptr;
    double *nn_d2 = nullptr;
    double *weight = nullptr, *evec = nullptr, *newshape = nullptr;
    double *alpha = nullptr, *acoef = nullptr, *alpha_c = nullptr, *zbuf = nullptr;
    double *zrand = nullptr;     // [rp] standard-normal draws of a probabilistic update (posterior.sample())
    bool zrand_active = false;
    // upload of the draws by the asynchronous entry points: a pinned buffer of its own (the synchronous entry points rewrite `pin`),
    // guarded by an event -- the buffer is rewritten only after the previous upload has left it, and nothing depends on when a copy
    // from pageable memory happens to consume its source
    double *zpin = nullptr;
    hipEvent_t zpin_done = nullptr;
    DevState *st = nullptr;
    DevPose *pose = nullptr;
    gingr_state_scalars *hs_dev = nullptr;
    // alpha [rp], hs_dev and st live in ONE allocation (state_block), in this order: set_state pushes [alpha | scalars] and get_state
    // pulls [alpha | scalars | DevState] in a single transfer each, through the pinned host buffer `pin` (no pageable staging)
    double *state_block = nullptr;
    double *pin = nullptr;
    size_t pin_doubles = 0;
    // the Metropolis-Hastings step's results straight into the pinned buffer (round 6): the device's view of `pin`, a counter of the
    // read-back kernel's finished workgroups, and the launch number the last of them stores into pin[pin_doubles - 1]
    double *pin_dev = nullptr;
    int32_t *mh_done = nullptr;
    uint64_t mh_epoch = 0;
    double *scalars = nullptr;  // local {Np, xPx, trPXY, yPy, -, c, -, -}
    double *part = nullptr;     // block partials of the scalar sums
    double *absmax = nullptr;   // [0] target, [1] fit: largest |coordinate| (exponent-argument range check)
    int32_t *tperm = nullptr;   // target cloud is kept in Morton order: tperm[s] = original target index of device position s
    std::vector<int32_t> h_tperm;
    double *tboxes = nullptr, *fboxes = nullptr;  // bounding boxes of the 256-point tiles of target / fit
    int32_t *tile_bad = nullptr;                  // target tiles holding a non-finite 1/den (never culled)
    double *xch = nullptr;
    int64_t off[GINGR_NUM_SEGMENTS] = {0, 0}, cnt[GINGR_NUM_SEGMENTS] = {0, 0};
    double *ws = nullptr;
    int64_t ws_doubles = 0;
    int colsum_chunks = 0;  // > 0: the column sums of phase 0 are still chunk partials in ws (single shard; added up by den_finalize)
    double *work = nullptr;
    void *aos = nullptr;  // staging for interleaved transfers, max(3M, 3N) doubles
    int32_t n_lm = 0;
    int32_t *lm_pid = nullptr;
    double *lm_xyz = nullptr, *lm_cov = nullptr;
    int32_t *lm_mask = nullptr;
    int32_t global_transform = GINGR_RIGID_TRANSFORMS;
    double step_length = 1.0;
    double stop_threshold = -1.0;  // gingr_fitter_set_stop_threshold: the run's stopping rule, applied by post_solve_kernel (< 0: none)
    int32_t stop_hit = 0;          // DevState::stopped as of the last gingr_fitter_get_state
    int32_t last_err = 0;          // DevState::pad (error code of the last update, 0: it committed) as of the last gingr_fitter_get_state
    bool has_state = false;
    // ---- ICP surface correspondence (surface.h, surface*.hip): triangles in device vertex positions and a spatial triangle order
    int32_t surface_method = 0;                    // 0 TriangularClosestPoint, 1 AlongNormalClosestPoint (ICP.scala:32-34)
    // reversed correspondence direction (ICP.scala:46-48): per TARGET vertex buffers, then one observation per model vertex
    bool reversed = false;
    // ... on a row shard the correspondence itself is replicated work (its queries are the replicated target) against the GATHERED
    // template, so the per-template-vertex arrays cover the whole template in ORIGINAL vertex order (set_meshes builds them); the
    // observations of this shard's rows are picked out afterwards (reversal_local_kernel)
    int32_t *radj_ptr = nullptr, *radj_tri = nullptr, *rmbnd = nullptr;
    double *rmvn = nullptr, *rfboxes = nullptr;
    void *rws = nullptr;
    // Round 5: the SCAN of the reversed direction is sharded too.  Its queries are the replicated target, so they partition by index
    // range -- this shard takes the device positions [rq0, rq0 + rqn) of the target, the fraction of the cloud that its rows are of
    // the template -- and every shard accumulates, per TEMPLATE vertex of the whole template (original ids), the sum of its accepted
    // target points and their number: revsum [4][M_total] = {sum x, sum y, sum z, count}.  One all-reduce (sum) of that buffer
    // (exchange segment GINGR_SEGMENT_REVSUM, between phases 0 and 1) gives every shard the totals; it keeps its own rows
    // (reversal_local_kernel).  partial_revsum: where the contribution goes when the sum lands elsewhere (device group).
    int64_t rq0 = 0, rqn = 0;
    double *rtvn_loc = nullptr;   // [3][rqn] vertex normals of the target's query range (the target is fixed: built once)
    double *revsum = nullptr, *partial_revsum = nullptr;
    // The nearest-template-VERTEX search of that direction runs against a spatially ordered copy of the gathered template: the
    // gathered fit is in original vertex order (the triangles index it), whose 256-vertex tiles are not compact, so the box-pruned
    // scan degenerated to all pairs (100 us for 5 121 queries x 40 962 vertices).  gperm (k-d leaf order of the first gathered fit,
    // fixed afterwards: a deforming template stays coherent) / gsorted [3][M_total]; matches are mapped back to original ids.
    int32_t *gperm = nullptr;
    double *gsorted = nullptr;
    int32_t *rnn_pos = nullptr;  // last search's matches as POSITIONS in gsorted: the warm start of the next one (queries and order are fixed)
    bool rnn_warm = false;
    // ... and the closest-point scan of that direction (target vertices against the MOVING template's triangles) starts every query
    // from the triangle that was closest to it last time (round 5; the forward direction has done so since round 2): positions in mtri
    int32_t *rtri_pos = nullptr;
    bool rtri_warm = false;
    int32_t *mtri_orig = nullptr, *mboundary = nullptr;
    double *rcp = nullptr, *rd2 = nullptr, *rnnd2 = nullptr, *rw01 = nullptr, *robs = nullptr, *rwin = nullptr;
    int32_t *rnn = nullptr, *rpre = nullptr, *rhit = nullptr, *rkeys = nullptr, *rvals = nullptr, *rskeys = nullptr, *rsvals = nullptr;
    void *rsort = nullptr;
    size_t rsort_bytes = 0;
    int64_t Tm = 0, Tt = 0;                        // model / target triangle counts
    int32_t *mtri = nullptr, *ttri = nullptr, *ttri_orig = nullptr;
    int32_t *madj_ptr = nullptr, *madj_tri = nullptr, *tadj_ptr = nullptr, *tadj_tri = nullptr;  // vertex -> triangles
    double *mcn = nullptr, *tcn = nullptr, *mvn = nullptr, *tvn = nullptr;  // cell / vertex normals (SoA)
    double *mtboxes = nullptr, *ttboxes = nullptr;  // triangle tile boxes [nt][6], quarter boxes [4 nt][6], group boxes [nt / 16 + 1][6] (line_nearest)
    double *mtribox = nullptr, *ttribox = nullptr;  // per-triangle boxes [T][6] (tri_tile_bbox_kernel), staged by the scan kernels
    int32_t *tboundary = nullptr;                   // target boundary vertices (device target positions)
    double *surf_cp = nullptr, *surf_d2 = nullptr, *surf_w01 = nullptr, *surf_win = nullptr, *surf_nnd2 = nullptr;
    int32_t *surf_nn = nullptr, *surf_pre = nullptr, *surf_hit = nullptr;
    // ---- memo of the posterior inputs (the reference keeps Memoize(computePosterior, 10), GingrAlgorithm.scala:68): phases 0 and
    // 1 (correspondences, Gram, right-hand side) depend only on (shape, pose, sigma2) of the state and on the flavour / its
    // parameters.  state_key describes the state last written by gingr_fitter_set_state while the device still holds it; post_key
    // the state whose phase-0/1 results sit in the exchange buffer.  A Metropolis-Hastings step asks for the posterior of the same
    // state up to three times (proposal, both transition densities); single shard only (a sharded run all-reduces the buffer).
    struct Key {
        std::vector<double> v;  // alpha[r], euler, center, translation, scale, sigma2
        int flavour = -1;       // memo_flavour_key (correspondence.h)
        double p0 = 0, p1 = 0;  // CPD: w, lambda
        bool compact = false;   // phase 1 ran the compact Gram pass of a coordinate-separable model (fitter_phases.hip: use_compact)
        bool same(const Key &o) const { return flavour == o.flavour && p0 == o.p0 && p1 == o.p1 && compact == o.compact && v == o.v; }
    };
    Key state_key, post_key;
    bool state_key_valid = false;
    int post_stage = 0;       // 0 nothing, 1 phase 0 done, 2 phases 0 and 1 done for post_key
    bool skip_phase1 = false;
    double *small = nullptr;  // 8 doubles of device scratch for scalar results
    StatScratch *stat_scratch = nullptr;  // of gingr_fitter_surface_distance_stats and gingr_fitter_mh_step (kept across calls)
    // Second memo slot and the factor cache of the transition-density query.  A Metropolis-Hastings step works on two states, the
    // current x and the candidate x' (proposal from x, q(x'|x), q(x|x')), and the next step starts from one of the two: `alt_seg`
    // keeps the [G, rhs, scalars] segment of the state the live memo held before (alt_key), and is swapped back in instead of
    // recomputing phases 0 and 1.  Only the probabilistic entry points use it (allow_alt): after a swap the correspondence arrays
    // on the device belong to the other state (corr_stale), which the getters of the deterministic path must never see.
    // fxbuf[live] / fxbuf[live ^ 1] go with the live / alt slot: [rp*rp] factor of S_tot + eps (I + G), [rp] posterior
    // coefficients, [rp] reciprocal diagonal -- what posterior_logpdf_lds_kernel leaves for posterior_logpdf_cached_kernel.
    double *alt_seg = nullptr;
    // The two memo slots exchange ROLES, not contents: seg_swapped = the live [G, rhs, scalars] segment is alt_seg and the parked one
    // sits in the exchange buffer.  Entry points that work on the exchange buffer itself (deterministic, sharded) move it back first.
    bool seg_swapped = false;
    double *seg1_live() const { return seg_swapped ? alt_seg : xch + off[1]; }
    double *seg1_parked() const { return seg_swapped ? xch + off[1] : alt_seg; }
    Key alt_key;
    int alt_stage = 0;
    bool allow_alt = false, corr_stale = false;
    double *fxbuf[2] = {nullptr, nullptr};
    unsigned *lp_sync = nullptr;  // hand-over words of posterior_logpdf_split_kernel
    double *lp_scratch = nullptr;  // [rp*rp + 2 rp], ranks >= 128 on a row shard: where the two-workgroup transition density leaves its
                                   // state-only part when no memo slot wants it (fitter_logpdf_finish; allocated on first use)
    unsigned lp_epoch = 0;
    bool fx_valid[2] = {false, false};
    // nfac[slot]: [rp*rp] Cholesky factor of I + G, [16*rp] the transposed inverses of its diagonal blocks -- left by the two-workgroup log-density kernel for the
    // sampled proposal that may start from this state (a + L^-T z without factoring again); a sits in fxbuf[slot] + rp*rp
    double *nfac[2] = {nullptr, nullptr};
    bool nf_valid[2] = {false, false};
    int live = 0;
    int32_t *surf_tri_pos = nullptr;  // per model vertex: position (in ttri) of its closest target triangle of the last scan
    bool surf_tri_warm = false;
    bool nn_warm = false, surf_nn_warm = false;  // nn_idx / surf_nn hold last time's matches against the CURRENT target
    NNGrid tgrid;  // uniform grid over the target cloud (set_target): the point-cloud ICP's closest-point search (nn_grid.hip)
    TriGrid ttgrid;  // uniform grid over the target TRIANGLES (set_meshes): the surface ICP's closest surface point (surface_grid.hip, surface.hip)
    MovGrid mgrid;   // the same over the TEMPLATE's triangles, rebuilt on the device every iteration: the self-intersection test (round 5)
    void forget_posteriors() {
        post_stage = 0;
        alt_stage = 0;
        fx_valid[0] = fx_valid[1] = false;
        nf_valid[0] = nf_valid[1] = false;
    }
    // Where phases 0 / 1 put THIS shard's partial sums (same segment layout as xch).  nullptr: into xch itself (single shard, or a
    // host that all-reduces xch in place -- torch.distributed).  The device group (group.hip) points it at the shard's send
    // buffer: peers read that while the summed result lands in xch, so nobody overwrites what a peer may still be reading.
    double *partial_out = nullptr;
    bool group_member = false;  // created by a device group (group.hip), of one device or more: the dense passes only (use_compact)
    // Row-sharded surface ICP: the tests against the template itself (vertex normals, self-intersection) need the WHOLE posed template,
    // so every iteration starts with a gather -- each shard contributes its rows of the fit to a [3][M_total] buffer in ORIGINAL
    // point order (zeros elsewhere), the buffers are summed across the shards (exchange segment 2: an all-gather spelled as the
    // all-reduce the other segments already use) -- and the template triangles index that buffer.  partial_fullfit: where the
    // contribution goes when the sum lands elsewhere (device group); nullptr = in place.
    double *fullfit = nullptr, *partial_fullfit = nullptr;
    // ... or, where the host has a real all-gather (RCCL: rccl_exchange.hip; gingr_fitter_gather_stage / _finish): the shard's rows go
    // into ITS slot of gstage [world][3][chunk] (original row order, chunk = ceil(M_total / world)), the slots are all-gathered in
    // place and one kernel spreads them over the planes of `fullfit` -- half the wire bytes of the zero-padded all-reduce, no sum
    int32_t *zero_counts = nullptr;  // [ceil(M / 256)] zero-weight vertices per block of the surface observations (gp.h: ZeroGate)
    double *gstage = nullptr;
    int gstage_world = 0;
    // what the ranks agreed on for this (model, meshes, world): -1 not asked yet, 0 the zero-padded all-reduce, 1 the all-gather
    // (rccl_exchange.hip: the choice between two different collectives must be the same on every rank)
    int gather_agreed = -1, gather_agreed_world = 0;
    bool sharded() const { return m->M != m->M_total; }
    int32_t *retry = nullptr;  // device word: retryCounter of the algorithm instance this fitter stands for (GingrAlgorithm.scala:69-70)
    // ---- one Metropolis-Hastings step per call (gingr_fitter_mh_step): the state x the step started from stays on the device --
    // [alpha | scalars | DevState] in mh_save, its fit in fit_alt (the proposal's fit is written to the OTHER buffer and the two
    // pointers are exchanged, no copy) -- so that a rejected proposal costs one small copy and one pass over the basis.  The states
    // a step produces on the device are unknown to the host until it reads them: the posterior memo keys them by a serial number.
    double *fit_alt = nullptr, *mh_save = nullptr;
    double *mh_rb = nullptr;  // [head + 8 + 3M]: what one step sends back, gathered for one copy
    Key mh_key;
    bool mh_saved = false;
    uint64_t mh_serial = 0;
    // The quarter boxes / |coordinate - centre| maximum of the fit are read by the two CPD pair loops only: the pass that writes the
    // fit produces them once a CPD phase has asked for them (cpd_seen), an ICP-only fitter runs the plain, shorter pass.
    bool cpd_seen = false, fit_boxes_valid = false;
    // GINGR_OPT_SPLIT_EXCHANGE (fitter_sharded_update): 0 the whole column-sum pass; 1 / 2 only the first / second half of the target
    // tiles (phase 0 is then run twice, with the all-reduce of the first half in between on the context's second stream)
    int split_half = 0;
    // gingr_fitter_posterior_covariance_* (posterior_cov.hip): the bordered system the factor L^-T of I + G is left in, and the
    // [6 M] result before it goes to the host; allocated on first use, kept across calls
    DevBuf cov_work, cov_out;
    // ---- correspondences given by the caller, flavour 3 (fitter_pairs.hip).  Isotropic pairs: the list as uploaded (ppid global ids,
    // pxyz interleaved, pvar), the sort buffers, and the per-vertex planes they are consolidated into once per gingr_fitter_set_pairs
    // -- pobs [3][M] / pwin [M], what launch_obs_points reads every iteration.  All sized for pairs_cap pairs, grown only.
    int64_t n_pairs = 0, pairs_cap = -1;
    int32_t *ppid = nullptr, *pkeys = nullptr, *pvals = nullptr, *pskeys = nullptr, *psvals = nullptr;
    double *pxyz = nullptr, *pvar = nullptr, *pobs = nullptr, *pwin = nullptr;
    void *psort = nullptr;
    size_t psort_bytes = 0;
    // Pairs with a full covariance ride in the landmark pass: cat_* = [covariance pairs | landmarks] (device rows, -1 = another shard's
    // or a vertex a landmark overrides), rebuilt from the host copies below by whichever of set_pairs_cov / set_landmarks came last
    int32_t n_pc = 0, n_cat = 0;  // covariance pairs; entries of cat_* (n_pc + the landmarks they were built with)
    std::vector<int32_t> h_pc_row, h_lm_row, h_lm_mask;
    std::vector<double> h_pc_xyz, h_pc_cov, h_lm_xyz, h_lm_cov;
    DevBuf cat_pid, cat_xyz, cat_cov;
    // The dense covariance list (gingr_fitter_set_pairs_cov_dense): a third, independent list for one pair per vertex.  The list as
    // uploaded (dpid global ids, dxyz, dcov [9 K]) and its sort buffers, sized for dense_cap pairs and grown only; the per-vertex planes
    // it is consolidated into once per call -- dobs [3][M] / dprec [6][M], what launch_gram_cov reads every iteration -- and that
    // pass's workspace (gram_cov_ws_doubles).  n_dense = 0: no list, nothing of this is launched or read.
    int64_t n_dense = 0, dense_cap = -1;
    int32_t *dpid = nullptr, *dkeys = nullptr, *dvals = nullptr, *dskeys = nullptr, *dsvals = nullptr;
    double *dxyz = nullptr, *dcov = nullptr, *dobs = nullptr, *dprec = nullptr;
    void *dsort = nullptr;
    size_t dsort_bytes = 0;
    DevBuf dense_ws;
    // gingr_fitter_set_pairs_plane_async fills the same planes on the device (n_dense = M marks them as a list: nothing of the uploaded
    // list is read per iteration).  plane_live: one device word, whether the state could take the update that follows
    // (plane_pairs_kernel writes it, plane_schedule_kernel reads it); allocated on first use.
    int32_t *plane_live = nullptr;
    // point-to-plane against a point cloud: a unit (or zero) normal per target point, planes [3][N] in the target's device order
    // (gingr_fitter_set_target_normals / _estimate_target_normals); nullptr = none, and a new target drops them
    double *tnormals = nullptr;
    // robust (M-estimator) weighting of the point-to-plane pairs (gingr_fitter_set_plane_robust; loss 0 = off: nothing below is
    // allocated, launched or read).  Per device row: the residual rs_s, its selection key rs_key and the variance inflation rs_u
    // (0 = not observed); rs_parts: observed rows per workgroup of the residual kernel; rs_counts / rs_sel: the selection's partial
    // counts and words (robust_select.hip).  rs_fresh: a robust refresh has filled them for the current setting.
    gingr_robust_params robust = {0, 0, 0.0, 0.0};
    double *rs_s = nullptr, *rs_u = nullptr;
    uint64_t *rs_key = nullptr, *rs_sel = nullptr;
    int32_t *rs_parts = nullptr;
    uint32_t *rs_counts = nullptr;
    bool rs_fresh = false;
};

// GINGR_OPT_GRAM_DOWNDATE by default: from this many local rows on.  The downdate pays while fewer than ~20 % of the rows have weight 0
// (41k: 15 + 17.5 us of downdate + right-hand-side sweep against 44 us of the weighted Gram pass at 0.2 % rejected; it costs one memory
// round trip per four zero-weight vertices of a slab); small meshes -- the femur chain rejects a fifth of its 1 622 vertices -- keep
// the pass over the basis, which is cheap there (13.6 us).  A fixed rule, not a measured one: both forms round differently.
constexpr int64_t kGramDowndateMinRows = 16384;
// The triangle grid pays from a few ten thousand target triangles on (41k x 82k: 94 -> 27 + 10 us per closest-point search); on a
// small mesh the tile scan with its sixteen query copies per workgroup is faster (femur, 3 240 triangles: 16 us against 15 + 7).
constexpr int64_t kTriGridMinTriangles = 16384;
constexpr size_t kScalarsDoubles = (sizeof(gingr_state_scalars) + 7) / 8, kDevStateDoubles = (sizeof(DevState) + 7) / 8;

// ---- small host helpers (inline: every file of the family allocates and checks launches)
template <typename T>
int dev_alloc(gingr_ctx *ctx, T **p, size_t count) {
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T)));
    // diagnostic (GINGR_DEBUG_POISON=1): new buffers start as NaN / 0xFFFFFFFF instead of whatever the allocator hands out, so that a
    // read of something never written shows instead of depending on what ran before
    static const bool poison = getenv("GINGR_DEBUG_POISON") != nullptr;
    if (poison) {  // (memsets of device memory are asynchronous to the host and not ordered with the context's non-blocking stream)
        HIP_TRY(ctx, hipMemset(*p, 0xFF, (count ? count : 1) * sizeof(T)));
        HIP_TRY(ctx, hipDeviceSynchronize());
    }
    return GINGR_OK;
}

inline void dev_free(void *p) { if (p) (void)hipFree(p); }

inline Cloud cloud_of(const double *soa, int64_t n) { return Cloud{soa, soa + n, soa + 2 * n, n}; }

// grow-only: steady-state queries (one likelihood evaluation per Metropolis-Hastings step) do not allocate
inline hipError_t ensure(DevBuf &b, size_t bytes) { return b.p && b.bytes >= bytes ? hipSuccess : b.alloc(bytes); }

// ---- fitter.hip
int check_ready(gingr_fitter *f);  // target and state set; makes the context's device current
int check_parameters(gingr_fitter *f, const Correspondence &c);  // check_ready, then the parameters of the flavour
SweepArgs base_args(const gingr_fitter *f);
// fit = modelInstanceShapePoseScale(model, state); compact: through the model's compact basis (the caller has checked that it exists)
void refresh_fit(gingr_fitter *f, bool compact = false);
void fit_boxes_now(gingr_fitter *f);  // boxes + |coordinate - centre| maximum of a fit that refresh_fit did not write
// Key::v of a state the host knows by value: alpha[r], euler, center, translation, scale, sigma2
std::vector<double> state_key_values(int32_t r, const double *alpha, const double euler[3], const double center[3], const double t[3],
                                     double scale, double sigma2);
void scalars_of_state(const DevState &hst, gingr_state_scalars *s);  // the fields a caller sees of the device state read back
int fitter_upload_zrand(gingr_fitter *f, const double *z);
// the one launch of mh_readback_kernel (n threads): out = [block | fit, original order, interleaved]; flag != nullptr: out is the pinned
// buffer through its device address and the last workgroup stores `epoch` into *flag
void launch_mh_readback(gingr_ctx *ctx, int64_t n, const double *block, int nblock, const double *fit, int64_t M, const int32_t *perm,
                        double *out, double *flag, int32_t *done, double epoch);
// the host's wait for that store into pin[pin_doubles - 1]; false: not seen within the deadline (the caller synchronises the stream)
bool wait_pinned_flag(gingr_fitter *f, double epoch);
int pull_small(gingr_fitter *f, const double *src, int n, double *dst);  // n <= 256 doubles from the device to `dst` inside f->pin
// The state behind both, for a caller without a fitter (pca_model.hip): a pinned host buffer whose last word is the flag, the device's
// view of it (nullptr: pull_small copies and synchronises), the read-back kernel's workgroup counter and the launch number.  A view --
// it owns nothing; the fitter's two functions above go through these with a view of its own fields.
struct PinnedWords {
    double *pin = nullptr;
    size_t pin_doubles = 0;
    double *pin_dev = nullptr;
    int32_t *done = nullptr;
    uint64_t epoch = 0;
};
bool wait_pinned_flag(const PinnedWords &w, double epoch);
int pull_small(gingr_ctx *ctx, PinnedWords &w, const double *src, int n, double *dst);  // `dst` inside w.pin
// ---- model.hip: a short-lived fitter posed by (euler, center, translation) with zero shape coefficients, and the posterior system of
// the stateless observations of gingr_model_posterior_mean: G [rp*rp] then rhs [rp] in `sys`.  The caller destroys the fitter.
int model_observation_system(gingr_ctx *ctx, const gingr_model *model, const double euler[3], const double center[3],
                             const double translation[3], const double *obs_xyz, const double *weight, int32_t n_lm, const int32_t *lm_pid,
                             const double *lm_xyz, const double *lm_cov, gingr_fitter **f_out, DevBuf &sys);
// ---- posterior_model.hip: dst->Q0 = R (src->Q0 T) on MFMA, one pass over the source basis; both models hold the same points (each in
// its own row order), T: [src->rp][dst->rp] on the device, zero beyond the two ranks
struct Rot3 {
    double R[9];  // row-major
};
void launch_basis_rotate(gingr_ctx *ctx, const gingr_model *src, const double *T, const Rot3 &rot, gingr_model *dst);
// ---- fitter_phases.hip
int gather_fit(gingr_fitter *f, const Correspondence &c, gingr_allreduce_fn reduce, void *user, fitter_gather_fn gather, const char *who);
int fitter_posterior_inputs(gingr_fitter *f, const Correspondence &c);  // phases 0 and 1 of the current state for a query (allow_alt)
// the forward surface correspondence of the current fit on its own (phase0_surface; single shard, meshes set: the caller has checked)
void fitter_surface_scan(gingr_fitter *f);
// the forward point-cloud correspondence of the current fit on its own (phase0_nearest_vertex; single shard: the caller has checked)
void fitter_cloud_scan(gingr_fitter *f);
// ---- fitter_surface.hip
void free_meshes(gingr_fitter *f);
// ---- fitter_pairs.hip
int pairs_ensure_planes(gingr_fitter *f);  // pobs / pwin exist (all zero before the first gingr_fitter_set_pairs)
int pairs_rebuild_cov_list(gingr_fitter *f);  // cat_* from the host copies of the covariance pairs and the landmarks
void free_pairs(gingr_fitter *f);
// ---- robust_select.hip: the key of rank k among keys [n_keys] into sel[2], everything enqueued on the context's stream.  parts != nullptr:
// the keys that take part are counted by parts [nparts] and k is their lower median's rank; else n_fixed / k_fixed.  counts:
// robust_select_plan::count_words(n_keys) words; sel: kRobustSelWords words ([0] n, [1] k, [2] key, [3] the scale c when `robust` is given)
constexpr int kRobustSelWords = 24;
void robust_select_enqueue(gingr_ctx *ctx, int64_t n_keys, const uint64_t *keys, int64_t nparts, const int32_t *parts, int64_t n_fixed,
                           int64_t k_fixed, uint32_t *counts, uint64_t *sel, const gingr_robust_params *robust);
