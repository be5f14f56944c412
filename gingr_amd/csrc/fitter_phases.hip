// One GiNGR update of the device-resident fitter as a fixed sequence of kernels with no host synchronisation, and its row-sharded
// drivers (C ABI in include/gingr_hip.h).
//
// One update = GingrAlgorithm.update (G/api/GingrAlgorithm.scala:192-254) followed by GingrGeneratorWrapper.propose's
// fit refresh and iteration++ (G/api/sampling/generators/GingrGeneratorWrapper.scala:28-39), split into three phases
// whose boundaries are exactly the points where a row-sharded run exchanges partial sums:
//   0  CPD column sums of K over the local rows (ICP: nearest neighbour, nothing to exchange)        -> segment 0
//   1  den, row statistics, observations, weighted Gram + right-hand side (+ landmarks), sigma2 sums -> segment 1
//   2  replicated O(r^2) algebra: posterior solve, then (moment form, gp.h) alpha_1, step blend, Umeyama, second
//      projection, alpha', state commit or failure status; finally the new fit of the local rows (one pass over Q0)
// run_phase dispatches one phase; its steps are the functions above it, in the order they run.
#include "fitter.h"

#include <algorithm>
#include <utility>

namespace {

// a <-> b (exchange != 0) or a <- b: the [G, rhs, scalars] segments of the two posterior memo slots
__global__ __launch_bounds__(256) void swap_segments_kernel(double *__restrict__ a, double *__restrict__ b, int64_t n, int exchange) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double va = a[i], vb = b[i];
    a[i] = vb;
    if (exchange) b[i] = va;
}

// full[d][g] = this shard's fit of original point g (device position iperm[g - row_begin]) or 0 for the points of other shards
__global__ __launch_bounds__(256) void fit_contribution_kernel(const double *__restrict__ fit, const int32_t *__restrict__ iperm, int64_t M,
                                                               int64_t row_begin, int64_t M_total, double *__restrict__ full) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= M_total) return;
    const int64_t l = g - row_begin;
    const bool mine = l >= 0 && l < M;
    const int64_t pos = mine ? iperm[l] : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) full[d * M_total + g] = mine ? fit[d * M + pos] : 0.0;
}

// stage[d][l] = this shard's fit of its l-th row in ORIGINAL order (device position iperm[l]); l < M
__global__ __launch_bounds__(256) void fit_to_stage_kernel(const double *__restrict__ fit, const int32_t *__restrict__ iperm, int64_t M, int64_t chunk,
                                                           double *__restrict__ stage) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= M) return;
    const int64_t pos = iperm[l];
#pragma unroll
    for (int d = 0; d < 3; ++d) stage[d * chunk + l] = fit[d * M + pos];
}
// full[d][g] = stage[q][d][g - begin(q)], q = the shard that owns row g under the balanced contiguous partition of M_total rows over
// `world` shards (the first M_total % world shards hold one row more)
__global__ __launch_bounds__(256) void stage_to_fullfit_kernel(const double *__restrict__ stage, int world, int64_t chunk, int64_t M_total,
                                                               double *__restrict__ full) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= M_total) return;
    const int64_t base = M_total / world, extra = M_total % world;
    const int64_t cut = extra * (base + 1);  // rows below `cut` sit in shards of base + 1 rows
    const int64_t q = g < cut ? g / (base + 1) : extra + (g - cut) / (base > 0 ? base : 1);
    const int64_t b = q * base + (q < extra ? q : extra);
    const double *p = stage + q * 3 * chunk + (g - b);
#pragma unroll
    for (int d = 0; d < 3; ++d) full[d * M_total + g] = p[d * chunk];
}

// the observations of this shard's rows out of the per-template-vertex arrays of the whole template (original vertex order): device
// position p of the shard holds original vertex row_begin + perm[p]
// (sums: [4][M_total] = {sum x, sum y, sum z, count} of the accepted target points per template vertex, summed over all shards'
// query ranges: the observation of a vertex is their mean, its weight count / sigma2 -- k isotropic observations of one point)
__global__ __launch_bounds__(256) void reversal_local_kernel(int64_t M, int64_t row_begin, const int32_t *__restrict__ perm, int64_t M_total,
                                                             const double *__restrict__ sums, const double *__restrict__ sigma2,
                                                             double *__restrict__ obs, double *__restrict__ win) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    const int64_t g = row_begin + perm[p];
    const double k = sums[3 * M_total + g];
    const double kk = k > 0.0 ? k : 1.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) obs[d * M + p] = sums[d * M_total + g] / kk;
    win[p] = k / sigma2[0];
}

// dst[d][p] = src[d][perm[p]] (SoA planes of n points)
__global__ __launch_bounds__(256) void soa_permute_kernel(const double *__restrict__ src, const int32_t *__restrict__ perm, int64_t n,
                                                          double *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t g = perm[p];
#pragma unroll
    for (int d = 0; d < 3; ++d) dst[d * n + p] = src[d * n + g];
}
// idx[j] = map[pos[j]] (positions in the spatially ordered template -> original vertex ids); negative entries stay
__global__ __launch_bounds__(256) void index_map_kernel(const int32_t *__restrict__ pos, int64_t n, const int32_t *__restrict__ map,
                                                        int32_t *__restrict__ idx) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t v = pos[j];
    idx[j] = v >= 0 ? map[v] : v;
}

// where GINGR_OPT_SPLIT_EXCHANGE cuts the target cloud: half of its 256-point tiles
int64_t split_cut(int64_t N) { return (N / 512) * 256; }

// idx / d2 = nearest TARGET vertex of every query (positions in the target's device order; lowest original index on ties): the grid
// search over the fixed target cloud first (nn_grid.hip), then the tile scan masked to the queries the grid could not certify -- a
// launch that exits at once when there are none.  warm: idx holds the previous matches of the same queries.
void nearest_target_vertex(gingr_ctx *ctx, gingr_fitter *f, Cloud query, Cloud tgt, int32_t *idx, double *d2, bool warm) {
    const int32_t *w = warm ? idx : nullptr;
    if (ctx->nn_grid && f->tgrid.ready && ctx->cull && query.n <= f->tgrid.max_queries) {
        if (!launch_nn_grid(ctx, query, tgt, f->tperm, f->tgrid, w, idx, d2))  // (true: a small cloud, nothing left to scan)
            launch_nn(ctx, query, tgt, f->tperm, f->tboxes, f->ws, idx, d2, idx, f->tgrid.flag, f->tgrid.cur_nflag());
    } else {
        launch_nn(ctx, query, tgt, f->tperm, f->tboxes, f->ws, idx, d2, w);
    }
}

// --------------------------------------------------------------------------------------------------- phases
// The exchange segments as one run_phase call sees them: the reduced (summed over shards) segments, read by phases 1 and 2 ...
struct Segments {
    double *seg0, *G, *rhs, *sc8;
    // ... and where this shard's partial sums are written by phases 0 and 1
    double *seg0w, *Gw, *rhsw, *sc8w;
};

// Whether this update runs the compact passes of a coordinate-separable model (gp.h: gingr_model::Qc) in place of the weighted Gram pass
// and the fit pass: a single shard, the flavours that take the weighted pass with nothing added to G behind it (CPD; the caller's pairs
// without covariances), no landmarks, no sampled proposal, no query that leaves the state as it is, no device group (whatever its size).  A fixed rule:
// the two forms add in different orders -- which is also why the answer is part of the posterior memo's key (memo_enter): phase-1 results
// are reused only by a caller that would have computed them the same way.
bool use_compact(const gingr_fitter *f, const Correspondence &c) {
    const gingr_model *m = f->m;
    if (!m->Qc || f->ctx->separable == 0) return false;
    if (m->M != m->M_total || f->partial_out || f->group_member) return false;
    if (!(c.kind == Flavour::Cpd || (c.kind == Flavour::Pairs && f->n_pc == 0 && f->n_dense == 0))) return false;
    return f->n_lm == 0 && !f->zrand_active && !f->allow_alt;
}

// Posterior memo (see gingr_fitter::Key): phases 0 and 1 are skipped when their results for exactly this state are still in place.
// Returns whether `phase` is already satisfied.  The state it mutates:
//   phase 0  skip_phase1; post_key, post_stage; alt_key, alt_stage; seg_swapped and live (the two slots exchange roles);
//            fx_valid / nf_valid of the live slot; corr_stale
//   phase 1  skip_phase1; post_stage 1 -> 2
//   phase 2  state_key_valid, mh_saved
bool memo_enter(gingr_fitter *f, const Correspondence &c, int phase) {
    const gingr_model *m = f->m;
    if (phase == 0) {
        f->skip_phase1 = false;
        gingr_fitter::Key k;
        k.flavour = memo_flavour_key(c, f->surface_method, f->reversed);
        k.p0 = c.cpd.w;  // (zero for every flavour but CPD)
        k.p1 = c.cpd.lambda;
        k.compact = use_compact(f, c);
        const bool single = m->M == m->M_total;
        if (single && f->state_key_valid) {
            k.v = f->state_key.v;
            if (f->post_stage == 2 && f->post_key.same(k)) {
                f->skip_phase1 = true;
                return true;
            }
            if (f->allow_alt && !f->partial_out && f->alt_stage == 2 && f->alt_key.same(k)) {
                // the other slot holds this state: the two slots exchange roles (no copy)
                const bool both = f->post_stage == 2;
                f->seg_swapped = !f->seg_swapped;
                if (both) {
                    std::swap(f->post_key, f->alt_key);
                } else {  // the live slot held nothing finished: nothing is parked now
                    f->post_key = f->alt_key;
                    f->alt_stage = 0;
                    f->fx_valid[f->live] = f->nf_valid[f->live] = false;
                }
                f->live ^= 1;
                f->post_stage = 2;
                f->corr_stale = true;
                f->skip_phase1 = true;
                return true;
            }
            if (f->allow_alt && !f->partial_out && f->post_stage == 2) {  // keep what is about to be overwritten: it becomes the parked slot
                f->seg_swapped = !f->seg_swapped;
                f->alt_key = f->post_key;
                f->alt_stage = 2;
                f->live ^= 1;  // its factors stay with it
            }
            f->fx_valid[f->live] = f->nf_valid[f->live] = false;
            f->post_key = k;
            f->post_stage = 1;
        } else {
            f->post_stage = 0;
            f->fx_valid[f->live] = f->nf_valid[f->live] = false;
        }
        f->corr_stale = false;  // phase 0 recomputes the correspondences of this state
    } else if (phase == 1) {
        if (f->skip_phase1) {
            f->skip_phase1 = false;
            return true;
        }
        if (f->post_stage == 1) f->post_stage = 2;
    } else {
        f->state_key_valid = false;  // the commit moves the device state away from the key
        f->mh_saved = false;
    }
    return false;
}

// ---- phase 0, one function per correspondence flavour
// CPD: the column sums of K over the local rows -> segment 0 (the split exchange asks for one half of the target tiles per call)
void phase0_cpd_colsums(gingr_fitter *f, const Segments &s, Cloud fit, Cloud tgt) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    // (the quarter boxes of the fit and its |coordinate - centroid| maximum were left by the pass that wrote the fit:
    // refresh_fit / fit_boxes_now)
    f->cpd_seen = true;
    if (!f->fit_boxes_valid) fit_boxes_now(f);  // (first CPD phase of this fitter, or the fit was written while it ran ICP)
    // single shard: nothing is exchanged, so the chunk partials stay in ws and phase 1's den_finalize adds them up
    const bool alone = m->M == m->M_total && !f->partial_out;
    if (f->split_half != 0 && !alone) {
        // one half of the target tiles (tile-aligned cut): its own launch, chunk plan and slice of the workspace
        const int64_t NA = split_cut(tgt.n);
        const bool first = f->split_half == 1;
        const Cloud th = first ? Cloud{tgt.x, tgt.y, tgt.z, NA} : Cloud{tgt.x + NA, tgt.y + NA, tgt.z + NA, tgt.n - NA};
        // (twice the chunks of the whole pass: half the targets x half-length chunks = the same number of workgroups)
        const int nch2 = 2 * cpd_colsum_chunks(M, tgt.n);
        (void)launch_cpd_colsum(ctx, fit, th, &f->st->sigma2, f->absmax, f->fboxes, first ? f->ws : f->ws + (int64_t)nch2 * NA,
                                s.seg0w + (first ? 0 : NA), nch2);
        f->colsum_chunks = 0;
        return;
    }
    f->colsum_chunks = launch_cpd_colsum(ctx, fit, tgt, &f->st->sigma2, f->absmax, f->fboxes, f->ws, alone ? nullptr : s.seg0w);
    if (!alone) f->colsum_chunks = 0;
}

// ICP on the point cloud: the nearest target vertex of every fit vertex
void phase0_nearest_vertex(gingr_fitter *f, Cloud fit, Cloud tgt) {
    nearest_target_vertex(f->ctx, f, fit, tgt, f->nn_idx, f->nn_d2, f->nn_warm);
    f->nn_warm = true;
}

// ICP on the surface, forward: ClosestPointTriangleMesh3D.closestPointCorrespondence (ClosestPointRegistrator.scala:75-100).
// meshc: the template mesh of the tests against the template itself -- the fit, or on a row shard the gathered fit of all shards
void phase0_surface(gingr_fitter *f, Cloud fit, Cloud tgt, Cloud meshc) {
    gingr_ctx *ctx = f->ctx;
    const int64_t M = f->m->M;
    launch_tri_tile_bbox(ctx, meshc, f->mtri, f->Tm, f->mtboxes, f->mtribox, f->mcn);  // boxes + cell normals of the template
    launch_vertex_normals(ctx, f->madj_ptr, f->madj_tri, f->mcn, f->Tm, M, f->mvn);
    const bool along = f->surface_method == 1;  // ClosestPointAlongNormalTriangleMesh3D (:102-131)
    if (along && ctx->tri_grid && (ctx->tri_grid == 2 || f->Tt >= kTriGridMinTriangles) && ctx->cull && f->ttgrid.ready)
        launch_line_nearest_grid(ctx, fit, f->mvn, f->ttgrid, f->surf_cp, f->surf_hit);
    else if (along)
        launch_line_nearest(ctx, fit, f->mvn, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttboxes, f->surf_cp, f->surf_hit);
    else if (ctx->tri_grid && (ctx->tri_grid == 2 || f->Tt >= kTriGridMinTriangles) && ctx->cull && f->ttgrid.ready &&
             f->surf_tri_warm && M <= f->ttgrid.max_queries) {
        // grid search from the previous iteration's triangles, then the masked tile scan for what it flagged
        launch_surface_cp_grid(ctx, fit, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttgrid, f->surf_cp, f->surf_d2, nullptr, f->surf_tri_pos);
        launch_surface_closest_point(ctx, fit, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttboxes, f->surf_cp, f->surf_d2, nullptr,
                                     f->surf_tri_pos, true, f->ttribox, f->ttgrid.flag, f->ttgrid.cur_nflag());
    } else {
        launch_surface_closest_point(ctx, fit, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttboxes, f->surf_cp, f->surf_d2, nullptr,
                                     f->surf_tri_pos, f->surf_tri_warm, f->ttribox);
        f->surf_tri_warm = true;
    }
    nearest_target_vertex(ctx, f, cloud_of(f->surf_cp, M), tgt, f->surf_nn, f->surf_nnd2, f->surf_nn_warm);
    f->surf_nn_warm = true;
    if (ctx->tri_grid == 2 && ctx->cull && f->mgrid.ready && M <= f->mgrid.max_queries) {
        launch_surface_prereject(ctx, M, f->surf_nn, f->tboundary, f->mvn, f->tvn, f->N, along ? f->surf_hit : nullptr,
                                 f->surf_pre);
        // GINGR_OPT_TRI_GRID = 2 only: the template's triangles binned for THIS iteration (boxes and tile boxes are the ones
        // computed above), the test over the cells the segment's ball reaches, the tile scan for what that could not
        // certify.  Same decisions; NOT the default -- at 41k x 82k the four build launches (setup, count, scan, fill:
        // ~30 us) + the query (31 us) lose to the barrier-free tile scan (50 us): tools/experiments/README.md, round 5
        launch_mov_grid_build(ctx, f->mgrid, meshc, f->mtri, nullptr, f->mtribox, f->mtboxes);
        launch_self_intersect_grid(ctx, fit, f->surf_cp, f->mgrid, f->surf_pre, f->surf_hit);
        launch_self_intersect(ctx, fit, f->surf_cp, f->mtri, f->Tm, f->mtboxes, f->surf_pre, f->surf_hit, f->mtribox, &meshc,
                              f->mgrid.flag, f->mgrid.cur_nflag());
        launch_surface_weight(ctx, M, f->surf_pre, f->surf_hit, &f->st->sigma2, f->surf_w01, f->surf_win);
    } else {
        // one launch: the first two rejection tests in its prologue, the third (self-intersection) in its tile scan, the
        // weights in its epilogue (until round 5: surface_prereject_kernel + this + surface_weight_kernel)
        SelfIntersectFuse fu;
        fu.nn_vertex = f->surf_nn, fu.boundary = f->tboundary, fu.q_vn = f->mvn, fu.t_vn = f->tvn, fu.Nt = f->N;
        fu.found = along ? f->surf_hit : nullptr, fu.pre_out = f->surf_pre;
        fu.sigma2 = &f->st->sigma2, fu.w01 = f->surf_w01, fu.weight_in = f->surf_win;
        launch_self_intersect(ctx, fit, f->surf_cp, f->mtri, f->Tm, f->mtboxes, nullptr, f->surf_hit, f->mtribox, &meshc, nullptr, nullptr, &fu);
    }
}

// The template side of the reversed correspondence, which a single shard and a row shard name differently
struct ReversedSide {
    Cloud mesh;                        // what the template triangles index: the fit (device order) / the gathered fit (original order)
    const int32_t *adj_ptr, *adj_tri;  // its vertex -> triangles lists,
    double *vn;                        //   vertex normals [3][mesh.n]
    const int32_t *boundary;           //   and boundary mask
    Cloud q;                           // the target queries: the whole target / this shard's range of it, which starts at
    int64_t q0;                        //   position q0 of the per-target arrays,
    const double *q_vn;                //   and their vertex normals
    const Cloud *whole_target;         // what the TARGET triangles index where q is only a range of it (nullptr: q itself)
    double *sums;                      // row shard: the range's per-template-vertex sums leave the phase; nullptr: the observations
};

// One-off on a row shard (synchronises once): the spatial order of the gathered template for the vertex search -> gperm, gsorted,
// rnn_pos.  Failure-atomic: the three members are set together, once everything exists and the order is on the device -- a half-built
// set would make every later phase 0 skip this and index with garbage.
int build_template_order(gingr_fitter *f) {
    gingr_ctx *ctx = f->ctx;
    const int64_t Mt = f->m->M_total;
    std::vector<double> soa((size_t)3 * Mt), aosv((size_t)3 * Mt);
    HIP_TRY(ctx, hipMemcpyAsync(soa.data(), f->fullfit, soa.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t g = 0; g < Mt; ++g)
        for (int d = 0; d < 3; ++d) aosv[(size_t)(3 * g + d)] = soa[(size_t)(d * Mt + g)];
    std::vector<int32_t> order;
    kd_leaf_order(aosv.data(), Mt, order);
    int32_t *gperm = nullptr, *rnn_pos = nullptr;
    double *gsorted = nullptr;
    int rc = dev_alloc(ctx, &gperm, (size_t)Mt);
    if (!rc) rc = dev_alloc(ctx, &gsorted, (size_t)3 * Mt);
    if (!rc) rc = dev_alloc(ctx, &rnn_pos, (size_t)(f->N > 0 ? f->N : 1));
    if (!rc && hipMemcpy(gperm, order.data(), (size_t)Mt * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        rc = gingr_set_error(ctx, GINGR_ERR_HIP, "reversed direction: copying the template order failed");
    if (rc) {
        dev_free(gperm), dev_free(gsorted), dev_free(rnn_pos);
        return rc;
    }
    f->gperm = gperm, f->gsorted = gsorted, f->rnn_pos = rnn_pos;
    return GINGR_OK;
}

// -> f->rnn: the template vertex nearest to every query, warm-started from the last search (the queries are the same target vertices,
// the template moved a little -- with it the chunks a small query range is split into all start from a tight bound)
void nearest_template_vertex(gingr_fitter *f, const ReversedSide &s, Cloud q) {
    gingr_ctx *ctx = f->ctx;
    if (s.sums) {  // against the spatially ordered copy of the gathered template; rnn: ORIGINAL vertex ids (lowest id on exact ties)
        launch_nn(ctx, q, cloud_of(f->gsorted, s.mesh.n), f->gperm, f->rfboxes, f->rws, f->rnn_pos, f->rnnd2, f->rnn_warm ? f->rnn_pos : nullptr);
        f->rnn_warm = true;
        hipLaunchKernelGGL(index_map_kernel, dim3((unsigned)ceil_div(q.n, 256)), dim3(256), 0, ctx->stream, f->rnn_pos, q.n, f->gperm, f->rnn);
    } else {  // rnn: positions in the fit's device order -- last iteration's matches start this one's scan
        launch_nn(ctx, q, s.mesh, f->m->perm, f->fboxes, f->ws, f->rnn, f->rnnd2, f->rnn_warm ? f->rnn : nullptr);
        f->rnn_warm = true;
    }
}

// ICP, reversed direction: closestPointCorrespondenceReversal (ClosestPointRegistrator.scala:34-49) -- the roles of the two meshes are
// swapped, then every accepted target vertex becomes an observation of the template vertex nearest to its match.
// On a row shard the same correspondence runs against the GATHERED template (meshc: original vertex order, so a matched vertex IS its
// original id and ties go to the lowest id as on a single shard), for THIS shard's range of the target queries only; what leaves the
// phase is the per-template-vertex sums of the range (see gingr_fitter::revsum).  The tests that involve the target mesh itself
// (self-intersection) see the whole target.
int phase0_reversed(gingr_fitter *f, const Correspondence &c, Cloud fit, Cloud tgt, Cloud meshc) {
    gingr_ctx *ctx = f->ctx;
    ReversedSide s;
    if (f->sharded()) {
        if (!f->fullfit || !f->revsum)
            return gingr_set_error(ctx, GINGR_ERR_STATE, "reversed correspondence direction on a row shard: meshes / direction not set");
        const int64_t Mt = f->m->M_total, q0 = f->rq0;
        if (!f->gperm) GINGR_TRY(build_template_order(f));
        hipLaunchKernelGGL(soa_permute_kernel, dim3((unsigned)ceil_div(Mt, 256)), dim3(256), 0, ctx->stream, f->fullfit, f->gperm, Mt, f->gsorted);
        launch_tile_bbox(ctx, cloud_of(f->gsorted, Mt), f->rfboxes);
        s = ReversedSide{meshc, f->radj_ptr, f->radj_tri, f->rmvn, f->rmbnd, Cloud{tgt.x + q0, tgt.y + q0, tgt.z + q0, f->rqn}, q0, f->rtvn_loc, &tgt,
                         f->partial_revsum ? f->partial_revsum : f->revsum};
    } else {
        launch_tile_bbox(ctx, fit, f->fboxes);
        s = ReversedSide{fit, f->madj_ptr, f->madj_tri, f->mvn, f->mboundary, tgt, 0, f->tvn, nullptr, nullptr};
    }
    const int64_t Mv = s.mesh.n;
    const bool surface = c.kind == Flavour::IcpSurface, along = f->surface_method == 1;
    if (surface) {
        launch_cell_normals(ctx, s.mesh, f->mtri, f->Tm, f->mcn);
        launch_vertex_normals(ctx, s.adj_ptr, s.adj_tri, f->mcn, f->Tm, Mv, s.vn);
        launch_tri_tile_bbox(ctx, s.mesh, f->mtri, f->Tm, f->mtboxes, f->mtribox);
    }
    if (s.q.n > 0 && surface) {  // (an empty range: a shard with few rows; a single shard's target is never empty)
        if (along) {
            launch_line_nearest(ctx, s.q, s.q_vn, s.mesh, f->mtri, f->mtri_orig, f->Tm, f->mtboxes, f->rcp, f->rhit);
        } else {
            launch_surface_closest_point(ctx, s.q, s.mesh, f->mtri, f->mtri_orig, f->Tm, f->mtboxes, f->rcp, f->rd2, nullptr, f->rtri_pos,
                                         f->rtri_warm, f->mtribox);
            f->rtri_warm = true;
        }
        nearest_template_vertex(f, s, cloud_of(f->rcp, s.q.n));
        SelfIntersectFuse fu;  // (the first two rejection tests ride in the self-intersection launch)
        fu.nn_vertex = f->rnn, fu.boundary = s.boundary, fu.q_vn = s.q_vn, fu.t_vn = s.vn, fu.Nt = Mv;
        fu.found = along ? f->rhit : nullptr, fu.pre_out = f->rpre;
        launch_self_intersect(ctx, s.q, f->rcp, f->ttri, f->Tt, f->ttboxes, nullptr, f->rhit, f->ttribox, s.whole_target, nullptr, nullptr, &fu);
    } else if (s.q.n > 0) {  // ClosestPointTriangleMesh3DSimple: nearest template vertex, weight 1
        nearest_template_vertex(f, s, s.q);
    }
    const int32_t *pre = surface ? f->rpre : nullptr, *hit = surface ? f->rhit : nullptr;
    if (s.sums)
        launch_reversal_sums(ctx, Mv, s.q, f->rnn, pre, hit, f->rkeys, f->rvals, f->rskeys, f->rsvals, f->rsort, f->rsort_bytes, f->rw01 + s.q0, s.sums);
    else
        launch_reversal_observations(ctx, Mv, s.q, f->rnn, pre, hit, &f->st->sigma2, f->rkeys, f->rvals, f->rskeys, f->rsvals, f->rsort,
                                     f->rsort_bytes, f->rw01, f->robs, f->rwin);
    return GINGR_OK;
}

// ---- phase 1
// The observations (correspondence point, uncertainty) of the local rows -> weight, evec; CPD: also den and the row statistics.
// Fills the scalar-sum fields of `fa`.
void phase1_observations(gingr_fitter *f, const Correspondence &c, const Segments &s, Cloud fit, Cloud tgt, Phase1FinalizeArgs &fa) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    if (c.kind == Flavour::Pairs) {  // the caller's pairs, consolidated per vertex by gingr_fitter_set_pairs; weight 0: no pair
        launch_obs_points(ctx, m, f->st, f->pobs, f->pwin, f->weight, f->evec, f->lm_mask);
        fa.scalar_mode = 0;
    } else if (c.kind != Flavour::Cpd) {
        if (f->reversed && f->sharded())  // the totals over all shards' query ranges are in place: this shard's rows of them
            hipLaunchKernelGGL(reversal_local_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, ctx->stream, M, m->row_begin, m->perm,
                               m->M_total, f->revsum, &f->st->sigma2, f->robs, f->rwin);
        if (f->reversed)  // one observation per template vertex: mean of its accepted targets, weight count / sigma2
            launch_obs_points(ctx, m, f->st, f->robs, f->rwin, f->weight, f->evec, f->lm_mask);
        else if (c.kind == Flavour::IcpSurface)  // only the weight-1 pairs are observed (ICP.scala:50): weight 0 drops the row
            launch_obs_points(ctx, m, f->st, f->surf_cp, f->surf_win, f->weight, f->evec, f->lm_mask, f->zero_counts);
        else if (f->n_lm != 0)  // (without landmarks the observation is formed inside the right-hand-side pass of run_phase)
            launch_obs_icp(ctx, m, f->st, tgt, f->nn_idx, f->lm_mask, f->weight, f->evec);
        fa.scalar_mode = 0;
    } else {
        launch_cpd_den_finalize(ctx, tgt, &f->st->sigma2, c.cpd.w, m->M_total, s.seg0, f->inv_den, f->Pt1, f->tile_bad, f->part,
                                f->scalars, f->colsum_chunks > 0 ? f->ws : nullptr, f->colsum_chunks);
        f->colsum_chunks = 0;
        // observations (correspondence point, uncertainty) come out of the row-statistics reduction; the scalar sums are
        // finished by the phase-1 finalize kernel
        CpdObsArgs ob;
        memset(&ob, 0, sizeof(ob));
        ob.ref = m->ref;
        ob.mean = m->mean;
        ob.sigma2 = &f->st->sigma2;
        ob.R = f->st->R;
        ob.center = f->st->center;
        ob.t = f->st->t;
        ob.lambda = c.cpd.lambda;
        ob.lm_mask = f->lm_mask;
        ob.weight = f->weight;
        ob.evec = f->evec;
        launch_cpd_rowstats(ctx, fit, tgt, &f->st->sigma2, f->absmax, f->inv_den, f->tboxes, f->tile_bad, f->ws, f->P1,
                            f->PX, f->part, f->scalars, nullptr, 0, &ob, false);
        fa.scalar_mode = 1;
        fa.part = f->part;
        fa.scalars_local = f->scalars;
        fa.contribute_xpx = m->row_begin == 0 ? 1 : 0;
    }
}

// for the right-hand-side sweep behind phase1_gram: the Gram pass left its partials already / the gate it carries (ZeroGate{}: none)
struct GramOutcome {
    bool rhs_done;
    ZeroGate rhs_gate;
};

// The weighted Gram matrix Q^T W Q of the local rows, as slab partials in gram_ws and/or a scaled copy of the model's moment; both are
// added up by the phase-1 finalize kernel, whose Gram fields of `fa` this fills.  The contract as it stands, per case:
//   scaled moment    point-cloud ICP without landmarks: every row has the weight 1 / sigma2.  No launch.  mom holds the total over
//                    ALL shards: the shard that owns row 0 contributes it (scaled_contribute), the others contribute zero.
//   gated downdate   forward surface ICP, gram_downdate == 1, or by size (gram_downdate < 0 and M >= kGramDowndateMinRows, M the rows of
//                    THIS shard): the moment (shard of row 0) minus this shard's zero-weight rows, slabs in gram_ws.  By size, the
//                    choice is made again on the device: the downdate and the right-hand-side sweep carry the gate `few`, a weighted
//                    pass launched behind them carries `many` and writes its slabs (alt_nslabs) and right-hand-side partials over
//                    the same gram_ws / sweep_ws (at rp >= 128 its ungated row expansion writes behind the WIDE plan's slab count).
//                    The gate sums THIS shard's zero_counts against THIS shard's M: the shards of one update may decide differently.
//   weighted pass    everything else -- always for the pairs flavour, whose weights are the caller's: each shard contributes the pass over its own rows; the pass may leave the right-hand-side
//                    partials as well (rhs_done).
//   compact pass     the weighted pass of a coordinate-separable model (use_compact): the three Gram blocks and right-hand sides from the
//                    compact basis, scattered into the same dense G / rhs by the finalize kernel (rhs_done).
GramOutcome phase1_gram(gingr_fitter *f, const Correspondence &c, double *gram_ws, double *sweep_ws, Phase1FinalizeArgs &fa) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    const int32_t rp = m->rp;
    GramOutcome out{false, ZeroGate{}};
    if (uniform_weights(c, f->reversed, f->n_lm)) {
        // (ICP.scala:90-92; written by the phase-1 finalize kernel: one launch less than a copy kernel of its own)
        fa.nslabs = 0;
        fa.scaled_src = m->mom + MomentLayout{rp}.stot();
        fa.sigma2 = &f->st->sigma2;
        fa.scaled_contribute = m->row_begin == 0 ? 1 : 0;
    } else if (zero_one_weights(c, f->reversed) &&
               (ctx->gram_downdate == 1 || (ctx->gram_downdate < 0 && M >= kGramDowndateMinRows))) {
        // surface correspondence: an accepted pair has the weight 1 / sigma2, a rejected one (and a vertex a landmark overrides) 0
        // (ICP.scala:50,90-92) -- the weighted Gram is the model's moment minus the rows of the zero-weight vertices, scaled.
        // One pass over THOSE rows (0.2 % of them at 41k x 82k) instead of the MFMA pass over the whole basis (44 us); the
        // right-hand side takes the sweep of run_phase.  By size (the default) the observation launch counted the zero-weight
        // vertices; with more than one in eight of them (open targets, partial overlap: ClosestPointRegistrator.scala:84-91) the
        // downdate and the sweep leave at once and the weighted pass behind them does the work, as without the option.
        const bool gated = ctx->gram_downdate != 1;
        ZeroGate few{f->zero_counts, (int32_t)ceil_div(M, 256), 0, M}, many = few;
        many.run_if_many = 1;
        fa.gram_partial = gram_ws;
        fa.nslabs = launch_gram_downdate(ctx, m->Q0, M, rp, f->weight, gram_ws, gated ? &few : nullptr);
        fa.scaled_src = m->mom + MomentLayout{rp}.stot();
        fa.sigma2 = &f->st->sigma2;
        fa.scaled_contribute = m->row_begin == 0 ? 1 : 0;
        if (gated) {
            bool alt_rhs = false;
            fa.alt_nslabs = launch_gram(ctx, m->Q0, M, rp, f->weight, gram_ws, nullptr, f->evec, sweep_ws, &alt_rhs, &many);
            fa.gate = many;
            out.rhs_gate = few;
        }
    } else if (use_compact(f, c)) {
        fa.gram_partial = gram_ws;
        fa.nslabs = launch_gram_compact(ctx, m->Qc, M, f->weight, f->evec, gram_ws);
        fa.sep_map = m->sep_map;
        out.rhs_done = true;
    } else {
        fa.gram_partial = gram_ws;
        fa.nslabs = launch_gram(ctx, m->Q0, M, rp, f->weight, gram_ws, nullptr, f->evec, sweep_ws, &out.rhs_done);
    }
    return out;
}

// ---- phase 2: the replicated algebra -- posterior solve, post-solve (commit or failure status) -- and the new fit of the local rows
void phase2_solve_and_commit(gingr_fitter *f, const Correspondence &c, const Segments &s) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int32_t r = m->r, rp = m->rp;
    // the posterior mean of the uniform-weight case comes from the model's eigen-decomposition (no factorisation); a sampled
    // proposal needs the Cholesky factor itself (its square root of the covariance is part of the parity contract)
    const bool eig = uniform_weights(c, f->reversed, f->n_lm) && !f->zrand_active && m->eig_ready;
    if (eig)
        launch_posterior_solve_eig(ctx, r, rp, m->eigV, m->eigL, &f->st->sigma2, s.rhs, f->acoef, f->st);
    else if (f->zrand_active && f->allow_alt && f->post_stage == 2 && f->nf_valid[f->live] && m->M == m->M_total && !f->partial_out)
        // the log-density query that first met this state left the factor of I + G and the posterior coefficients behind
        launch_posterior_sample_cached(ctx, r, rp, f->nfac[f->live], f->fxbuf[f->live] + (int64_t)rp * rp, f->zrand, f->acoef, f->st);
    else if (use_compact(f, c))
        launch_posterior_solve_separable(ctx, m, s.G, s.rhs, f->acoef, f->st);
    else
        launch_posterior_solve(ctx, r, rp, s.G, s.rhs, f->zrand_active ? f->zrand : nullptr, f->work, f->acoef, f->st);
    launch_post_matvecs(ctx, m, f->alpha, f->acoef, f->zbuf);
    PostSolveArgs a;
    memset(&a, 0, sizeof(a));
    a.r = r;
    a.rp = rp;
    a.pvec = m->pvec;
    a.zbuf = f->zbuf;
    a.alpha = f->alpha;
    a.scalars = s.sc8;
    a.is_icp = post_solve_sigma2_rule(c);  // sigma2 of the next state: CPD's sums / ICP's schedule / kept (the caller's updateSigma2)
    if (is_icp_schedule(c)) {
        a.icp_step = (c.icp.initial_sigma - c.icp.end_sigma) / (double)c.icp.max_iterations;  // ICP.scala:65
        a.icp_end = c.icp.end_sigma;
    }
    a.step = f->step_length;
    a.global_transform = f->global_transform;
    a.state = f->st;
    a.retry = f->retry;
    a.zero_slot = f->absmax + 1;
    a.probabilistic = f->zrand_active ? 1 : 0;
    a.stop_threshold = f->stop_threshold;
    launch_post_solve(ctx, a);
    refresh_fit(f, use_compact(f, c));
}

int run_phase(gingr_fitter *f, const Correspondence &c, int phase) {
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    const int64_t M = m->M;
    const int32_t rp = m->rp;
    if (f->seg_swapped && !f->allow_alt) {  // this entry point works on the exchange buffer itself: the live segment moves back
        const int64_t seg = (int64_t)rp * rp + rp + 8;
        hipLaunchKernelGGL(swap_segments_kernel, dim3((unsigned)ceil_div(seg, 256)), dim3(256), 0, ctx->stream, f->xch + f->off[1], f->alt_seg,
                           seg, 0);
        f->seg_swapped = false;
        f->alt_stage = 0;  // (what was parked there is given up)
        f->fx_valid[f->live ^ 1] = f->nf_valid[f->live ^ 1] = false;
    }
    Segments s;
    s.seg0 = f->xch + f->off[0];
    s.G = f->seg1_live();
    s.rhs = s.G + (int64_t)rp * rp;
    s.sc8 = s.rhs + rp;
    double *wbase = f->partial_out ? f->partial_out : f->xch;
    s.seg0w = wbase + f->off[0];
    s.Gw = f->partial_out ? wbase + f->off[1] : s.G;
    s.rhsw = s.Gw + (int64_t)rp * rp;
    s.sc8w = s.rhsw + rp;
    const Cloud fit = cloud_of(f->fit, M);
    const Cloud tgt = cloud_of(f->target, f->N);
    if (phase == GINGR_PHASE_GATHER) {  // sharded surface ICP: this shard's rows of the fit into the full-fit buffer (gingr_fitter::fullfit)
        if (!f->sharded()) return GINGR_OK;
        if (!f->fullfit) return gingr_set_error(ctx, GINGR_ERR_STATE, "gather phase: no meshes set (gingr_fitter_set_meshes)");
        hipLaunchKernelGGL(fit_contribution_kernel, dim3((unsigned)ceil_div(m->M_total, 256)), dim3(256), 0, ctx->stream, f->fit, m->iperm, M,
                           m->row_begin, m->M_total, f->partial_fullfit ? f->partial_fullfit : f->fullfit);
        return check_launch(ctx);
    }
    // the template mesh of the surface tests: the fit itself, or -- on a row shard -- the gathered fit of all shards (original order)
    const Cloud meshc = f->sharded() && f->fullfit ? cloud_of(f->fullfit, m->M_total) : fit;
    if (memo_enter(f, c, phase)) return GINGR_OK;
    switch (phase) {
        case 0:
            if (c.kind == Flavour::Pairs)
                break;  // the correspondences are the caller's: nothing to compute, nothing to exchange
            if (reversed_icp(c, f->reversed))
                GINGR_TRY(phase0_reversed(f, c, fit, tgt, meshc));
            else if (c.kind == Flavour::IcpSurface)
                phase0_surface(f, fit, tgt, meshc);
            else if (c.kind == Flavour::IcpCloud)
                phase0_nearest_vertex(f, fit, tgt);
            else
                phase0_cpd_colsums(f, s, fit, tgt);
            break;
        case 1: {
            Phase1FinalizeArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.rp = rp;
            fa.G = s.Gw;
            fa.rhs = s.rhsw;
            fa.sc8 = s.sc8w;
            phase1_observations(f, c, s, fit, tgt, fa);
            double *gram_ws = f->ws, *sweep_ws = f->ws + gram_ws_doubles(M, rp);
            const GramOutcome gram = phase1_gram(f, c, gram_ws, sweep_ws, fa);
            fa.sweep_partial = sweep_ws;
            if (gram.rhs_done) {  // the Gram pass left the right-hand-side partials, one row per slab
                fa.sweep_blocks = fa.nslabs;
            } else {
                SweepArgs a = base_args(f);
                a.evec = f->evec;
                a.partial = sweep_ws;
                a.no_reduce = 1;
                a.gate = gram.rhs_gate;
                if (uniform_weights(c, f->reversed, f->n_lm)) {  // point-cloud ICP: observation + Q^T e in one pass
                    a.state = f->st;
                    a.icp_idx = f->nn_idx;
                    a.tx = tgt.x, a.ty = tgt.y, a.tz = tgt.z;
                    a.n_targets = tgt.n;
                    a.lm_mask = f->lm_mask;
                    a.weight_out = f->weight, a.evec_out = f->evec;
                    launch_sweep(ctx, SWEEP_RHS_ICP, a);
                } else {
                    launch_sweep(ctx, SWEEP_RHS, a);
                }
                fa.sweep_blocks = sweep_num_blocks(M);
            }
            launch_phase1_finalize(ctx, fa);
            if (c.kind == Flavour::Pairs && f->n_dense > 0)  // the dense covariance list: its own pass, added before the segment is handed out
                launch_gram_cov(ctx, m, f->st, f->dobs, f->dprec, f->lm_mask, f->dense_ws.as<double>(), s.Gw, s.rhsw);
            if (c.kind == Flavour::Pairs && f->n_pc > 0)  // one launch over [covariance pairs | landmarks]: a defined summation order
                launch_landmarks(ctx, m, f->st, f->n_cat, f->cat_pid.as<int32_t>(), f->cat_xyz.as<double>(), f->cat_cov.as<double>(),
                                 s.Gw, s.rhsw);
            else
                launch_landmarks(ctx, m, f->st, f->n_lm, f->lm_pid, f->lm_xyz, f->lm_cov, s.Gw, s.rhsw);
            break;
        }
        case 2:
            phase2_solve_and_commit(f, c, s);
            break;
        default:
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "phase %d out of range", phase);
    }
    return check_launch(ctx);
}

}  // namespace

// One phase of one flavour (GINGR_PHASE_GATHER included); the caller has checked the descriptor (check_correspondence)
int fitter_run_phase(gingr_fitter *f, const Correspondence &c, int phase) { return run_phase(f, c, phase); }

// The launches of the forward surface correspondence alone, for a caller that turns their results into pairs of its own
// (fitter_pairs.hip: gingr_fitter_set_pairs_plane_async).  The correspondence arrays belong to the current state afterwards.
void fitter_surface_scan(gingr_fitter *f) {
    const Cloud fit = cloud_of(f->fit, f->m->M);
    phase0_surface(f, fit, cloud_of(f->target, f->N), fit);
    f->corr_stale = false;
}

void fitter_cloud_scan(gingr_fitter *f) {
    phase0_nearest_vertex(f, cloud_of(f->fit, f->m->M), cloud_of(f->target, f->N));
    f->corr_stale = false;
}

// The posterior inputs of the current state -- correspondences, Gram, right-hand side -- for a query that leaves the state as it is:
// phases 0 and 1, which may bring a parked memo slot back (allow_alt)
int fitter_posterior_inputs(gingr_fitter *f, const Correspondence &c) {
    f->allow_alt = true;
    int rc = GINGR_OK;
    for (int ph = 0; ph < 2 && rc == GINGR_OK; ++ph) rc = run_phase(f, c, ph);
    f->allow_alt = false;
    return rc;
}

// n_iterations single-shard updates of one flavour, each timed as one step
int fitter_update(gingr_fitter *f, const Correspondence &c, int32_t n_iterations) {
    GINGR_TRY(check_correspondence(f, c));
    if (f->sharded()) {
        static const char *const text[4] = {
            "update_cpd_async: sharded model needs the phase API + exchange", "update_icp_async: sharded model needs the phase API + exchange",
            "update_icp_surface_async: a row shard needs the sharded update (gingr_fitter_update_sharded_async / _rccl_async / the device group)",
            "update_pairs_async: a row shard needs the sharded update (gingr_fitter_update_sharded_async)"};
        return gingr_set_error(f->ctx, GINGR_ERR_STATE, "%s", text[(int)c.kind]);
    }
    for (int32_t it = 0; it < n_iterations; ++it) {
        TimerScope ts(f->ctx, 3);
        for (int ph = 0; ph < GINGR_NUM_PHASES; ++ph) GINGR_TRY(run_phase(f, c, ph));
    }
    return GINGR_OK;
}

static int checked_phase(gingr_fitter *f, const Correspondence &c, int32_t phase) {
    GINGR_TRY(check_correspondence(f, c));
    return run_phase(f, c, phase);
}

extern "C" {

int gingr_fitter_cpd_phase_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t phase) {
    return checked_phase(f, abi_correspondence(0, p, nullptr), phase);
}
int gingr_fitter_icp_phase_async(gingr_fitter *f, const gingr_icp_params *p, int32_t phase) {
    return checked_phase(f, abi_correspondence(1, nullptr, p), phase);
}
int gingr_fitter_icp_surface_phase_async(gingr_fitter *f, const gingr_icp_params *p, int32_t phase) {
    return checked_phase(f, abi_correspondence(2, nullptr, p), phase);
}
int gingr_fitter_pairs_phase_async(gingr_fitter *f, int32_t phase) { return checked_phase(f, abi_correspondence(3, nullptr, nullptr), phase); }

int gingr_fitter_update_cpd_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t n_iterations) {
    return fitter_update(f, abi_correspondence(0, p, nullptr), n_iterations);
}
int gingr_fitter_update_icp_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations) {
    return fitter_update(f, abi_correspondence(1, nullptr, p), n_iterations);
}
int gingr_fitter_update_icp_surface_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations) {
    return fitter_update(f, abi_correspondence(2, nullptr, p), n_iterations);
}
int gingr_fitter_update_pairs_async(gingr_fitter *f, int32_t n_iterations) {
    return fitter_update(f, abi_correspondence(3, nullptr, nullptr), n_iterations);
}

}  // extern "C"

// The row-sharded update of any flavour, deterministic (z == nullptr) or with a sampled proposal (z: rank standard normals, one
// iteration): per iteration [surface: gather phase, all-reduce of the full fit], phase 0, [CPD: all-reduce of the column sums],
// phase 1, all-reduce of the Gram bundle, phase 2.  The posterior solve, the sample a + L^-T z and everything behind them are
// replicated r x r algebra, so z is the same on every shard and nothing else is exchanged.
// gather (nullable): does the whole gather of the fit itself (stage, all-gather, unpack: rccl_exchange.hip) and returns 0; a positive
// value means "not possible here" and the zero-padded all-reduce through `reduce` is used instead
int gather_fit(gingr_fitter *f, const Correspondence &c, gingr_allreduce_fn reduce, void *user, fitter_gather_fn gather, const char *who) {
    gingr_ctx *ctx = f->ctx;
    if (gather) {
        const int g = gather(user, f);
        if (g == 0) return GINGR_OK;
        if (g < 0) return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: the all-gather of the fit failed", who);
    }
    GINGR_TRY(run_phase(f, c, GINGR_PHASE_GATHER));
    if (reduce(user, GINGR_SEGMENT_FULLFIT, f->fullfit, 3 * f->m->M_total) != 0)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "%s: the all-reduce callback failed (full fit)", who);
    return GINGR_OK;
}

int fitter_sharded_update(gingr_fitter *f, const Correspondence &c, int32_t n_iterations, const double *z, gingr_allreduce_fn reduce,
                          void *user, fitter_gather_fn gather, bool split_native) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (n_iterations < 0 || !reduce || correspondence_error(c) == CorrespondenceError::BadFlavour)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sharded update: bad arguments");
    GINGR_TRY(check_correspondence(f, c));
    if (f->partial_out) return gingr_set_error(ctx, GINGR_ERR_STATE, "sharded update: this fitter belongs to a device group");
    if (z && n_iterations != 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "sharded update: a sampled proposal is one iteration");
    if (z) GINGR_TRY(fitter_upload_zrand(f, z));
    f->zrand_active = z != nullptr;
    int rc = GINGR_OK;
    // GINGR_OPT_SPLIT_EXCHANGE: pass 1 in two halves of the target tiles; the all-reduce of the first half runs on the context's second
    // stream (ordered by events, same communicator) while the second half computes, so only the second half's all-reduce is exposed
    bool split = split_native && c.kind == Flavour::Cpd && f->sharded() && f->N >= 8192;
    // (the halves take twice the chunks of the whole pass)
    if (split && (int64_t)2 * cpd_colsum_chunks(f->m->M, f->N) * f->N > f->ws_doubles) split = false;
    if (split && !ctx->side_stream) {
        if (hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->split_ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->split_ev[1], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            split = false;
        }
    }
    for (int32_t it = 0; it < n_iterations && rc == GINGR_OK; ++it) {
        TimerScope ts(ctx, 3);
        if (needs_gathered_fit(c, f->reversed) && f->sharded()) rc = gather_fit(f, c, reduce, user, gather, "sharded update");
        for (int ph = 0; ph < GINGR_NUM_PHASES && rc == GINGR_OK; ++ph) {
            if (ph == 0 && split) {
                const int64_t NA = split_cut(f->N);
                double *seg0 = f->xch + f->off[0];
                f->split_half = 1;
                rc = run_phase(f, c, 0);
                {
                    TimerScope tx(ctx, 6);
                    if (!rc && (hipEventRecord(ctx->split_ev[0], ctx->stream) != hipSuccess ||
                                hipStreamWaitEvent(ctx->side_stream, ctx->split_ev[0], 0) != hipSuccess))
                        rc = gingr_set_error(ctx, GINGR_ERR_HIP, "sharded update: event ordering of the split exchange failed");
                    if (!rc) {
                        ctx->exchange_stream = ctx->side_stream;
                        const int xr = reduce(user, 0, seg0, NA);
                        ctx->exchange_stream = nullptr;
                        if (xr != 0) rc = gingr_set_error(ctx, GINGR_ERR_STATE, "sharded update: the all-reduce callback failed (segment 0, first half)");
                    }
                    if (!rc && hipEventRecord(ctx->split_ev[1], ctx->side_stream) != hipSuccess)
                        rc = gingr_set_error(ctx, GINGR_ERR_HIP, "sharded update: event ordering of the split exchange failed");
                }
                f->split_half = 2;
                if (!rc) rc = run_phase(f, c, 0);
                f->split_half = 0;
                {
                    TimerScope tx(ctx, 6);
                    if (!rc && reduce(user, 0, seg0 + NA, f->N - NA) != 0)
                        rc = gingr_set_error(ctx, GINGR_ERR_STATE, "sharded update: the all-reduce callback failed (segment 0, second half)");
                    if (!rc && hipStreamWaitEvent(ctx->stream, ctx->split_ev[1], 0) != hipSuccess)
                        rc = gingr_set_error(ctx, GINGR_ERR_HIP, "sharded update: event ordering of the split exchange failed");
                }
                continue;
            }
            rc = run_phase(f, c, ph);
            if (!rc && ph < GINGR_NUM_SEGMENTS && (ph != 0 || exchanges_segment0(c))) {
                TimerScope tx(ctx, 6 + ph);  // the exchange of segment ph as this shard sees it (includes waiting for the peers)
                if (reduce(user, ph, f->xch + f->off[ph], f->cnt[ph]) != 0)
                    rc = gingr_set_error(ctx, GINGR_ERR_STATE, "sharded update: the all-reduce callback failed (segment %d)", ph);
            }
            if (!rc && ph == 0 && exchanges_reversal_sums(c, f->reversed) && f->sharded() &&
                reduce(user, GINGR_SEGMENT_REVSUM, f->revsum, 4 * f->m->M_total) != 0)
                rc = gingr_set_error(ctx, GINGR_ERR_STATE, "sharded update: the all-reduce callback failed (reversal sums)");
        }
    }
    f->zrand_active = false;
    return rc;
}

extern "C" {

int gingr_fitter_update_cpd_sharded_async(gingr_fitter *f, const gingr_cpd_params *p, int32_t n_iterations, gingr_allreduce_fn reduce,
                                          void *user) {
    return fitter_sharded_update(f, abi_correspondence(0, p, nullptr), n_iterations, nullptr, reduce, user);
}

int gingr_fitter_update_icp_sharded_async(gingr_fitter *f, const gingr_icp_params *p, int32_t n_iterations, gingr_allreduce_fn reduce,
                                          void *user) {
    return fitter_sharded_update(f, abi_correspondence(1, nullptr, p), n_iterations, nullptr, reduce, user);
}

int gingr_fitter_update_sharded_async(gingr_fitter *f, int32_t flavour, const gingr_cpd_params *cp, const gingr_icp_params *ip,
                                      int32_t n_iterations, const double *z, gingr_allreduce_fn reduce, void *user) {
    return fitter_sharded_update(f, abi_correspondence(flavour, cp, ip), n_iterations, z, reduce, user);
}

int gingr_fitter_gather_stage(gingr_fitter *f, int32_t world, int32_t rank, void **send_ptr, void **recv_ptr, int64_t *count_per_rank) {
    if (!f || !send_ptr || !recv_ptr || !count_per_rank) return GINGR_ERR_BAD_ARGUMENT;
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    const gingr_model *m = f->m;
    if (!f->fullfit) return gingr_set_error(ctx, GINGR_ERR_STATE, "gather_stage: not a row shard with meshes (gingr_fitter_set_meshes)");
    if (world < 1 || rank < 0 || rank >= world) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "gather_stage: need 0 <= rank < world");
    const int64_t Mt = m->M_total, base = Mt / world, extra = Mt % world;
    const int64_t b = rank * base + (rank < extra ? rank : extra), e = b + base + (rank < extra ? 1 : 0);
    if (b != m->row_begin || e - b != m->M)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "gather_stage: rows [%lld, %lld) are not shard %d of the balanced partition over %d shards",
                               (long long)m->row_begin, (long long)(m->row_begin + m->M), (int)rank, (int)world);
    const int64_t chunk = ceil_div(Mt, world);
    if (!f->gstage || f->gstage_world != world) {
        dev_free(f->gstage);
        f->gstage = nullptr;
        GINGR_TRY(dev_alloc(ctx, &f->gstage, (size_t)world * 3 * chunk));
        HIP_TRY(ctx, hipMemsetAsync(f->gstage, 0, (size_t)world * 3 * chunk * sizeof(double), ctx->stream));
        f->gstage_world = world;
    }
    double *mine = f->gstage + (int64_t)rank * 3 * chunk;
    hipLaunchKernelGGL(fit_to_stage_kernel, dim3((unsigned)ceil_div(m->M, 256)), dim3(256), 0, ctx->stream, f->fit, m->iperm, m->M, chunk, mine);
    *send_ptr = mine;
    *recv_ptr = f->gstage;
    *count_per_rank = 3 * chunk;
    return check_launch(ctx);
}

int gingr_fitter_gather_finish(gingr_fitter *f, int32_t world) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!f->fullfit || !f->gstage || f->gstage_world != world)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "gather_finish: no gather staged for %d shards (gingr_fitter_gather_stage)", (int)world);
    const int64_t Mt = f->m->M_total;
    hipLaunchKernelGGL(stage_to_fullfit_kernel, dim3((unsigned)ceil_div(Mt, 256)), dim3(256), 0, ctx->stream, f->gstage, (int)world, ceil_div(Mt, world),
                       Mt, f->fullfit);
    return check_launch(ctx);
}

int gingr_fitter_reversal_exchange(gingr_fitter *f, void **dev_ptr, int64_t *count) {
    if (!f || !dev_ptr || !count) return GINGR_ERR_BAD_ARGUMENT;
    if (!f->revsum)
        return gingr_set_error(f->ctx, GINGR_ERR_STATE, "reversal_exchange: not a row shard with the reversed direction set (gingr_fitter_set_correspondence_direction)");
    *dev_ptr = f->revsum;
    *count = 4 * f->m->M_total;
    return GINGR_OK;
}

int gingr_fitter_fullfit_exchange(gingr_fitter *f, void **dev_ptr, int64_t *count) {
    if (!f || !dev_ptr || !count) return GINGR_ERR_BAD_ARGUMENT;
    if (!f->fullfit) return gingr_set_error(f->ctx, GINGR_ERR_STATE, "fullfit_exchange: not a row shard with meshes (gingr_fitter_set_meshes)");
    *dev_ptr = f->fullfit;
    *count = 3 * f->m->M_total;
    return GINGR_OK;
}

}  // extern "C"
