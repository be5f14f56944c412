// Surface ICP of the fitter: mesh set-up (gingr_fitter_set_meshes), surface method and correspondence direction, the surface getters,
// and the surface distance statistics with the two stateless gingr_mesh_* entries (C ABI in include/gingr_hip.h).
#include "fitter.h"

#include <algorithm>

namespace {

// dst[d][i] = src[d][q0 + i]: a compact copy of the planes of an SoA array for the index range [q0, q0 + n)
__global__ __launch_bounds__(256) void soa_range_kernel(const double *__restrict__ src, int64_t stride, int64_t q0, int64_t n, double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) dst[d * n + i] = src[d * stride + q0 + i];
}

// out [n] = 1 at map[v] (map == nullptr: at v) for every vertex v on an edge with exactly one adjacent triangle
// (TriangleMesh3DOperations.pointIsOnBoundary), 0 elsewhere
void mark_boundary(int64_t T, const int32_t *tri, const int32_t *map, int64_t n, std::vector<int32_t> &out) {
    out.assign((size_t)n, 0);
    std::vector<uint64_t> edges;
    edges.reserve((size_t)3 * T);
    for (int64_t t = 0; t < T; ++t)
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)tri[3 * t + k], b = (uint64_t)tri[3 * t + (k + 1) % 3];
            edges.push_back((a < b ? a : b) << 32 | (a < b ? b : a));
        }
    std::sort(edges.begin(), edges.end());
    for (size_t i = 0; i < edges.size();) {
        size_t j = i;
        while (j < edges.size() && edges[j] == edges[i]) ++j;
        if (j - i == 1)
            for (const uint64_t v : {edges[i] >> 32, edges[i] & 0xffffffffu}) out[(size_t)(map ? map[v] : (int32_t)v)] = 1;
        i = j;
    }
}

}  // namespace

void free_meshes(gingr_fitter *f) {
    void *rptrs[] = {f->mtri_orig, f->mboundary, f->rcp, f->rd2, f->rnnd2, f->rw01, f->robs, f->rwin, f->rnn, f->rpre, f->rhit,
                     f->rkeys, f->rvals, f->rskeys, f->rsvals, f->rsort, f->radj_ptr, f->radj_tri, f->rmbnd, f->rmvn, f->rfboxes,
                     f->rtvn_loc, f->revsum, f->rws, f->gperm, f->gsorted, f->rnn_pos, f->rtri_pos};
    for (void *p : rptrs) dev_free(p);
    f->radj_ptr = f->radj_tri = f->rmbnd = nullptr;
    f->rmvn = f->rfboxes = f->rtvn_loc = f->revsum = f->gsorted = nullptr;
    f->gperm = f->rnn_pos = f->rtri_pos = nullptr;
    f->rnn_warm = f->rtri_warm = false;
    f->gather_agreed = -1;  // (new meshes: the ranks agree again)
    f->rq0 = f->rqn = 0;
    f->rws = nullptr;
    f->mtri_orig = f->mboundary = f->rnn = f->rpre = f->rhit = f->rkeys = f->rvals = f->rskeys = f->rsvals = nullptr;
    f->rcp = f->rd2 = f->rnnd2 = f->rw01 = f->robs = f->rwin = nullptr;
    f->rsort = nullptr;
    f->rsort_bytes = 0;
    f->reversed = false;
    void *ptrs[] = {f->mtri, f->ttri, f->ttri_orig, f->madj_ptr, f->madj_tri, f->tadj_ptr, f->tadj_tri, f->mcn, f->tcn, f->mvn,
                    f->tvn, f->mtboxes, f->ttboxes, f->tboundary, f->surf_cp, f->surf_d2, f->surf_w01, f->surf_win, f->surf_nnd2,
                    f->surf_nn, f->surf_pre, f->surf_hit, f->surf_tri_pos, f->mtribox, f->ttribox};
    for (void *p : ptrs) dev_free(p);
    f->mtri = f->ttri = f->ttri_orig = f->madj_ptr = f->madj_tri = f->tadj_ptr = f->tadj_tri = f->tboundary = nullptr;
    f->mcn = f->tcn = f->mvn = f->tvn = f->mtboxes = f->ttboxes = f->mtribox = f->ttribox = nullptr;
    f->surf_cp = f->surf_d2 = f->surf_w01 = f->surf_win = f->surf_nnd2 = nullptr;
    f->surf_nn = f->surf_pre = f->surf_hit = f->surf_tri_pos = nullptr;
    f->surf_tri_warm = f->surf_nn_warm = false;
    tri_grid_free(&f->ttgrid);
    mov_grid_free(&f->mgrid);
    f->Tm = f->Tt = 0;
}

extern "C" {

// ------------------------------------------------------------------------------------------ ICP, surface correspondence
int gingr_fitter_set_meshes(gingr_fitter *f, int64_t n_model_tri, const int32_t *model_tri, int64_t n_target_tri,
                            const int32_t *target_tri) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    f->forget_posteriors();  // the posterior memos describe other inputs
    gingr_ctx *ctx = f->ctx;
    if (!f->target) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_meshes: no target set (gingr_fitter_set_target)");
    if (n_model_tri < 1 || n_target_tri < 1 || !model_tri || !target_tri)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_meshes: need at least one triangle per mesh");
    // A row shard takes the triangles of the WHOLE template (vertex ids of the full model): its queries are its own rows, but the
    // tests against the template itself -- vertex normals, self-intersection -- see all of it, through the gathered fit
    // (gingr_fitter::fullfit, original point order).  A single shard indexes its own fit (device order).
    const bool sharded = f->sharded();
    const int64_t M = f->m->M, N = f->N, Mt = f->m->M_total, rb = f->m->row_begin;
    for (int64_t k = 0; k < 3 * n_model_tri; ++k)
        if (model_tri[k] < 0 || model_tri[k] >= Mt) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_meshes: model vertex id out of range");
    for (int64_t k = 0; k < 3 * n_target_tri; ++k)
        if (target_tri[k] < 0 || target_tri[k] >= N) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "set_meshes: target vertex id out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    free_meshes(f);
    // device vertex positions of the two clouds (orig -> device) and their coordinates in device order
    std::vector<int32_t> tinv((size_t)N);
    for (int64_t s2 = 0; s2 < N; ++s2) tinv[(size_t)f->h_tperm[(size_t)s2]] = (int32_t)s2;
    std::vector<double> mpos((size_t)3 * M), mmean((size_t)3 * M), tpos((size_t)3 * N);
    HIP_TRY(ctx, hipMemcpy(mpos.data(), f->m->ref, mpos.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(mmean.data(), f->m->mean, mmean.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(tpos.data(), f->target, tpos.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < mpos.size(); ++k) mpos[k] += mmean[k];
    struct Built {
        std::vector<int32_t> tri, orig, adj_ptr, adj_tri;
    };
    // coord(v, d): coordinate d of vertex v; mesh_pos(v): its position in the cloud the triangles index; adj_slot(v): its slot in the
    // vertex -> triangles lists (n_adj slots) or -1 for a vertex this fitter does not own
    auto build = [&](int64_t T, const int32_t *tri, auto coord, auto mesh_pos, auto adj_slot, int64_t n_adj, Built &b) {
        std::vector<double> cen((size_t)3 * T);
        for (int64_t t = 0; t < T; ++t)
            for (int d = 0; d < 3; ++d) {
                double c = 0.0;
                for (int k = 0; k < 3; ++k) c += coord(tri[3 * t + k], d);
                cen[(size_t)3 * t + d] = c / 3.0;
            }
        kd_leaf_order(cen.data(), T, b.orig);  // orig[s] = original index of the triangle at device position s
        std::vector<int32_t> tpos2((size_t)T);
        b.tri.resize((size_t)3 * T);
        for (int64_t s2 = 0; s2 < T; ++s2) {
            const int32_t t = b.orig[(size_t)s2];
            tpos2[(size_t)t] = (int32_t)s2;
            for (int k = 0; k < 3; ++k) b.tri[(size_t)3 * s2 + k] = mesh_pos(tri[3 * t + k]);
        }
        // vertex -> triangles, in ascending ORIGINAL triangle index (the order the normals are averaged in)
        std::vector<int32_t> cnt((size_t)n_adj + 1, 0);
        int64_t total = 0;
        for (int64_t k = 0; k < 3 * T; ++k) {
            const int32_t sl = adj_slot(tri[k]);
            if (sl >= 0) cnt[(size_t)sl + 1]++, ++total;
        }
        for (int64_t v = 0; v < n_adj; ++v) cnt[(size_t)v + 1] += cnt[(size_t)v];
        b.adj_ptr = cnt;
        b.adj_tri.resize((size_t)(total > 0 ? total : 1));
        std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
        for (int64_t t = 0; t < T; ++t)
            for (int k = 0; k < 3; ++k) {
                const int32_t sl = adj_slot(tri[3 * t + k]);
                if (sl >= 0) b.adj_tri[(size_t)fill[(size_t)sl]++] = tpos2[(size_t)t];
            }
    };
    Built bm, bt;
    const std::vector<int32_t> &hip = f->m->hiperm;
    if (sharded) {
        const std::vector<double> &full = f->m->h_full_pts;
        if ((int64_t)full.size() != 3 * Mt) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_meshes: the shard holds no copy of the full mean shape");
        build(n_model_tri, model_tri, [&](int32_t v, int d) { return full[(size_t)3 * v + d]; }, [&](int32_t v) { return v; },
              [&](int32_t v) { return (v >= rb && v < rb + M) ? hip[(size_t)(v - rb)] : -1; }, M, bm);
    } else {
        build(n_model_tri, model_tri, [&](int32_t v, int d) { return mpos[(size_t)d * M + hip[(size_t)v]]; }, [&](int32_t v) { return hip[(size_t)v]; },
              [&](int32_t v) { return hip[(size_t)v]; }, M, bm);
    }
    build(n_target_tri, target_tri, [&](int32_t v, int d) { return tpos[(size_t)d * N + tinv[(size_t)v]]; }, [&](int32_t v) { return tinv[(size_t)v]; },
          [&](int32_t v) { return tinv[(size_t)v]; }, N, bt);
    // boundary vertices of the target, and of the model (reversed direction: the rejection rules run on the template side)
    std::vector<int32_t> bnd, mbnd((size_t)M, 0);
    mark_boundary(n_target_tri, target_tri, tinv.data(), N, bnd);
    if (!sharded) mark_boundary(n_model_tri, model_tri, hip.data(), M, mbnd);
    // (row shard) the whole template's vertex -> triangle lists and boundary flags in original vertex order: the reversed
    // correspondence direction tests the template vertex nearest to a match, which may belong to any shard
    Built bfull;
    std::vector<int32_t> mbnd_full;
    if (sharded) {
        const std::vector<double> &full = f->m->h_full_pts;
        build(n_model_tri, model_tri, [&](int32_t v, int d) { return full[(size_t)3 * v + d]; }, [&](int32_t v) { return v; },
              [&](int32_t v) { return v; }, Mt, bfull);
        mark_boundary(n_model_tri, model_tri, nullptr, Mt, mbnd_full);
    }
    f->Tm = n_model_tri;
    f->Tt = n_target_tri;
    const int64_t ntm = ceil_div(f->Tm, 256), ntt = ceil_div(f->Tt, 256);
    int rc;
    if ((rc = dev_alloc(ctx, &f->mtri, (size_t)3 * f->Tm)) || (rc = dev_alloc(ctx, &f->ttri, (size_t)3 * f->Tt)) ||
        (rc = dev_alloc(ctx, &f->ttri_orig, (size_t)f->Tt)) || (rc = dev_alloc(ctx, &f->madj_ptr, (size_t)M + 1)) ||
        (rc = dev_alloc(ctx, &f->madj_tri, bm.adj_tri.size())) || (rc = dev_alloc(ctx, &f->tadj_ptr, (size_t)N + 1)) ||
        (rc = dev_alloc(ctx, &f->tadj_tri, (size_t)3 * f->Tt)) || (rc = dev_alloc(ctx, &f->mcn, (size_t)3 * f->Tm)) ||
        (rc = dev_alloc(ctx, &f->tcn, (size_t)3 * f->Tt)) || (rc = dev_alloc(ctx, &f->mvn, (size_t)3 * M)) ||
        (rc = dev_alloc(ctx, &f->tvn, (size_t)3 * N)) || (rc = dev_alloc(ctx, &f->mtboxes, (size_t)30 * ntm + 6 * (ntm / 16 + 1))) ||
        (rc = dev_alloc(ctx, &f->ttboxes, (size_t)30 * ntt + 6 * (ntt / 16 + 1))) || (rc = dev_alloc(ctx, &f->tboundary, (size_t)N)) ||
        (rc = dev_alloc(ctx, &f->surf_cp, (size_t)3 * M)) || (rc = dev_alloc(ctx, &f->surf_d2, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->surf_w01, (size_t)M)) || (rc = dev_alloc(ctx, &f->surf_win, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->surf_nnd2, (size_t)M)) || (rc = dev_alloc(ctx, &f->surf_nn, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->surf_pre, (size_t)M)) || (rc = dev_alloc(ctx, &f->surf_hit, (size_t)M)) ||
        (rc = dev_alloc(ctx, &f->surf_tri_pos, (size_t)M)) || (rc = dev_alloc(ctx, &f->mtribox, (size_t)6 * f->Tm)) ||
        (rc = dev_alloc(ctx, &f->ttribox, (size_t)6 * f->Tt)) ||
        (rc = dev_alloc(ctx, &f->mtri_orig, (size_t)f->Tm)) || (rc = dev_alloc(ctx, &f->mboundary, (size_t)M)))
        return rc;
    auto up = [&](int32_t *dst, const std::vector<int32_t> &src) {
        return hipMemcpy(dst, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    };
    HIP_TRY(ctx, up(f->mtri, bm.tri));
    HIP_TRY(ctx, up(f->ttri, bt.tri));
    HIP_TRY(ctx, up(f->ttri_orig, bt.orig));
    HIP_TRY(ctx, up(f->madj_ptr, bm.adj_ptr));
    HIP_TRY(ctx, up(f->madj_tri, bm.adj_tri));
    HIP_TRY(ctx, up(f->tadj_ptr, bt.adj_ptr));
    HIP_TRY(ctx, up(f->tadj_tri, bt.adj_tri));
    HIP_TRY(ctx, up(f->tboundary, bnd));
    HIP_TRY(ctx, up(f->mtri_orig, bm.orig));
    HIP_TRY(ctx, up(f->mboundary, mbnd));
    if (sharded && !f->fullfit) {
        GINGR_TRY(dev_alloc(ctx, &f->fullfit, (size_t)3 * Mt));
        HIP_TRY(ctx, hipMemsetAsync(f->fullfit, 0, (size_t)3 * Mt * sizeof(double), ctx->stream));
    }
    if (sharded) {
        if ((rc = dev_alloc(ctx, &f->radj_ptr, (size_t)Mt + 1)) || (rc = dev_alloc(ctx, &f->radj_tri, bfull.adj_tri.size())) ||
            (rc = dev_alloc(ctx, &f->rmbnd, (size_t)Mt)) || (rc = dev_alloc(ctx, &f->rmvn, (size_t)3 * Mt)) ||
            (rc = dev_alloc(ctx, &f->rfboxes, (size_t)ceil_div(Mt, 256) * 30)))
            return rc;
        HIP_TRY(ctx, up(f->radj_ptr, bfull.adj_ptr));
        HIP_TRY(ctx, up(f->radj_tri, bfull.adj_tri));
        HIP_TRY(ctx, up(f->rmbnd, mbnd_full));
    }
    // static target side: cell normals, vertex normals, triangle tile boxes
    const Cloud tgt = cloud_of(f->target, N);
    launch_cell_normals(ctx, tgt, f->ttri, f->Tt, f->tcn);
    launch_vertex_normals(ctx, f->tadj_ptr, f->tadj_tri, f->tcn, f->Tt, N, f->tvn);
    launch_tri_tile_bbox(ctx, tgt, f->ttri, f->Tt, f->ttboxes, f->ttribox);
    GINGR_TRY(check_launch(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the target triangles do not move: bin them once (the surface ICP's warm-started closest-point search)
    GINGR_TRY(tri_grid_build(ctx, tpos.data(), N, bt.tri.data(), bt.orig.data(), n_target_tri, M, &f->ttgrid));
    // the template's triangles move: their grid is rebuilt on the device every iteration (self-intersection test); buffers only here
    GINGR_TRY(mov_grid_alloc(ctx, n_model_tri, M, &f->mgrid));
    return GINGR_OK;
}

int gingr_fitter_set_surface_method(gingr_fitter *f, int32_t method) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    if (method != 0 && method != 1) return gingr_set_error(f->ctx, GINGR_ERR_BAD_ARGUMENT, "set_surface_method: 0 or 1");
    f->surface_method = method;
    return GINGR_OK;
}

int gingr_fitter_set_correspondence_direction(gingr_fitter *f, int32_t reversed) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (!reversed) {
        f->reversed = false;
        return GINGR_OK;
    }
    if (!f->target) return gingr_set_error(ctx, GINGR_ERR_STATE, "set_correspondence_direction: no target set");
    if (f->sharded() && !f->radj_ptr)
        return gingr_set_error(ctx, GINGR_ERR_STATE, "set_correspondence_direction: a row shard needs the meshes first (gingr_fitter_set_meshes: "
                                                     "the reversed direction works on the gathered template)");
    if (f->sharded() && !f->revsum) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int64_t Mt = f->m->M_total, N = f->N;
        // this shard's range of the target queries: the same fraction of the (replicated) target as its rows are of the template --
        // the row ranges tile [0, M_total), so the query ranges tile [0, N), whatever the number of shards
        const int64_t q0 = (int64_t)((__int128)N * f->m->row_begin / Mt), q1 = (int64_t)((__int128)N * (f->m->row_begin + f->m->M) / Mt);
        f->rq0 = q0;
        f->rqn = q1 - q0;
        int rc;
        if ((rc = dev_alloc(ctx, &f->revsum, (size_t)4 * Mt)) || (rc = dev_alloc(ctx, &f->rtvn_loc, (size_t)3 * (f->rqn > 0 ? f->rqn : 1)))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(f->revsum, 0, (size_t)4 * Mt * sizeof(double), ctx->stream));
        if (f->tvn && f->rqn > 0)
            hipLaunchKernelGGL(soa_range_kernel, dim3((unsigned)ceil_div(f->rqn, 256)), dim3(256), 0, ctx->stream, f->tvn, N, q0, f->rqn, f->rtvn_loc);
        HIP_TRY(ctx, hipMalloc(&f->rws, (size_t)nn_ws_bytes(f->N, Mt)));
    }
    if (!f->rnn) {  // buffers per target vertex + the sort workspace, once per target
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int64_t M = f->m->M, N = f->N;
        int rc;
        if ((rc = dev_alloc(ctx, &f->rcp, (size_t)3 * N)) || (rc = dev_alloc(ctx, &f->rd2, (size_t)N)) ||
            (rc = dev_alloc(ctx, &f->rnnd2, (size_t)N)) || (rc = dev_alloc(ctx, &f->rw01, (size_t)N)) ||
            (rc = dev_alloc(ctx, &f->robs, (size_t)3 * M)) || (rc = dev_alloc(ctx, &f->rwin, (size_t)M)) ||
            (rc = dev_alloc(ctx, &f->rnn, (size_t)N)) || (rc = dev_alloc(ctx, &f->rpre, (size_t)N)) ||
            (rc = dev_alloc(ctx, &f->rhit, (size_t)N)) || (rc = dev_alloc(ctx, &f->rkeys, (size_t)N)) ||
            (rc = dev_alloc(ctx, &f->rvals, (size_t)N)) || (rc = dev_alloc(ctx, &f->rskeys, (size_t)N)) ||
            (rc = dev_alloc(ctx, &f->rsvals, (size_t)N)) || (rc = dev_alloc(ctx, &f->rtri_pos, (size_t)N)))
            return rc;
        f->rtri_warm = false;
        f->rsort_bytes = reversal_sort_temp_bytes(N);
        HIP_TRY(ctx, hipMalloc(&f->rsort, f->rsort_bytes ? f->rsort_bytes : 8));
    }
    f->reversed = true;
    return GINGR_OK;
}

int gingr_fitter_get_reversed_correspondence(gingr_fitter *f, int32_t *template_id, double *w) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (f->corr_stale)  // see gingr_fitter::alt_seg
        return gingr_set_error(ctx, GINGR_ERR_STATE, "get_reversed_correspondence: a probabilistic query brought another state's posterior back; the correspondences on the device are not this state's -- run an update or a phase first");
    if (!f->rnn) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_reversed_correspondence: direction not reversed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t N = f->N;
    // a row shard scanned ITS range of the target queries only (device positions [rq0, rq0 + rqn)): the others come back as
    // (-1, 0) -- the shards' answers are disjoint and together cover the target
    const int64_t q0 = f->sharded() ? f->rq0 : 0, nq = f->sharded() ? f->rqn : N;
    std::vector<int32_t> hid((size_t)(nq > 0 ? nq : 1));
    std::vector<double> hw((size_t)(nq > 0 ? nq : 1));
    if (nq > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(hid.data(), f->rnn, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(hw.data(), f->rw01 + q0, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t s2 = 0; s2 < N; ++s2) {  // device target position -> original target id; device model row -> original vertex id
        const int32_t j = f->h_tperm[(size_t)s2];
        const bool mine = s2 >= q0 && s2 < q0 + nq;
        const int32_t row = mine ? hid[(size_t)(s2 - q0)] : -1;
        if (template_id)  // (a row shard searched the gathered template: original vertex ids already)
            template_id[j] = f->sharded() ? ((row >= 0 && row < f->m->M_total) ? row : -1)
                                          : ((row >= 0 && row < f->m->M) ? f->m->hperm[(size_t)row] : -1);
        if (w) w[j] = mine ? hw[(size_t)(s2 - q0)] : 0.0;
    }
    return GINGR_OK;
}

int gingr_fitter_get_surface_correspondence(gingr_fitter *f, double *cp_xyz, double *w) {
    if (!f) return GINGR_ERR_BAD_ARGUMENT;
    gingr_ctx *ctx = f->ctx;
    if (f->corr_stale)  // see gingr_fitter::alt_seg
        return gingr_set_error(ctx, GINGR_ERR_STATE, "get_surface_correspondence: a probabilistic query brought another state's posterior back; the correspondences on the device are not this state's -- run an update or a phase first");
    if (!f->surf_cp) return gingr_set_error(ctx, GINGR_ERR_STATE, "get_surface_correspondence: no meshes set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t M = f->m->M;
    if (cp_xyz) {
        launch_soa_to_aos(ctx, f->surf_cp, M, reinterpret_cast<double *>(f->aos), f->m->perm);
        HIP_TRY(ctx, hipMemcpyAsync(cp_xyz, f->aos, (size_t)3 * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<double> hw((size_t)M);
    HIP_TRY(ctx, hipMemcpyAsync(hw.data(), f->surf_w01, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (w)
        for (int64_t s2 = 0; s2 < M; ++s2) w[f->m->hperm[(size_t)s2]] = hw[(size_t)s2];
    return GINGR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ surface distance statistics
namespace {

// out4 = {sum d, max d, count, sum log N(d; 0, sdev)} of d = |q - closest point of the mesh (v, tri)| over the queries q.
// `nn_orig` / `nn_boxes` / `boundary` (all three or none): the boundary-aware variant.  `scratch` holds what the kernels write.
int run_distance_stats(gingr_ctx *ctx, Cloud q, Cloud v, const int32_t *tri, const int32_t *tri_orig, int64_t T, const double *tboxes,
                       const int32_t *q_orig, int64_t q_limit, const int32_t *v_orig, const double *v_boxes,
                       const int32_t *boundary, double sdev, StatScratch &sc, double out4[4], double *pinned4 = nullptr,
                       const double *tribox = nullptr, gingr_fitter *spin_on = nullptr) {
    const int64_t K = q.n;
    HIP_TRY(ctx, ensure(sc.cp, (size_t)3 * K * sizeof(double)));
    HIP_TRY(ctx, ensure(sc.d2, (size_t)K * sizeof(double)));
    HIP_TRY(ctx, ensure(sc.part, (size_t)distance_stats_ws_doubles() * sizeof(double)));
    HIP_TRY(ctx, ensure(sc.out, 4 * sizeof(double)));
    HIP_TRY(ctx, ensure(sc.pos, (size_t)K * sizeof(int32_t)));
    const bool warm = sc.pos_K == K && sc.pos_T == T && sc.pos_tri == tri;
    launch_surface_closest_point(ctx, q, v, tri, tri_orig, T, tboxes, sc.cp.as<double>(), sc.d2.as<double>(), nullptr, sc.pos.as<int32_t>(),
                                 warm, tribox);
    sc.pos_K = K, sc.pos_T = T, sc.pos_tri = tri;
    if (boundary) {
        HIP_TRY(ctx, ensure(sc.nn, (size_t)K * sizeof(int32_t)));
        HIP_TRY(ctx, ensure(sc.nnd2, (size_t)K * sizeof(double)));
        HIP_TRY(ctx, ensure(sc.ws, (size_t)nn_ws_bytes(K, v.n)));
        launch_nn(ctx, cloud_of(sc.cp.as<double>(), K), v, v_orig, v_boxes, sc.ws.p, sc.nn.as<int32_t>(), sc.nnd2.as<double>());
    }
    launch_distance_stats(ctx, K, sc.d2.as<double>(), q_orig, q_limit, boundary ? sc.nn.as<int32_t>() : nullptr, boundary, sdev,
                          sc.part.as<double>(), sc.out.as<double>());
    GINGR_TRY(check_launch(ctx));
    if (spin_on && pinned4) {  // (the fitter's pinned buffer: pull_small)
        GINGR_TRY(pull_small(spin_on, sc.out.as<double>(), 4, pinned4));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(pinned4 ? pinned4 : out4, sc.out.p, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (pinned4) memcpy(out4, pinned4, 4 * sizeof(double));
    return GINGR_OK;
}

}  // namespace

// spatial orders of a stateless mesh query: queries and vertices (device position -> original; vinv: original -> position) and
// triangles by centroid (torder), with `tri` their vertex positions in that order (declared in surface.h: surface_metrics.hip plans
// its shared topology with it)
void mesh_orders(int64_t n_points, const double *points, int64_t n_vertices, const double *vertices, int64_t n_triangles,
                 const int32_t *triangles, std::vector<int32_t> &qorder, std::vector<int32_t> &vorder, std::vector<int32_t> &torder,
                 std::vector<int32_t> &vinv, std::vector<int32_t> &tri) {
    kd_leaf_order(points, n_points, qorder);
    kd_leaf_order(vertices, n_vertices, vorder);
    vinv.resize((size_t)n_vertices);
    for (int64_t s2 = 0; s2 < n_vertices; ++s2) vinv[(size_t)vorder[(size_t)s2]] = (int32_t)s2;
    std::vector<double> cen((size_t)3 * n_triangles);
    for (int64_t t = 0; t < n_triangles; ++t)
        for (int d = 0; d < 3; ++d) {
            double c = 0.0;
            for (int k = 0; k < 3; ++k) c += vertices[(size_t)3 * triangles[3 * t + k] + d];
            cen[(size_t)3 * t + d] = c / 3.0;
        }
    kd_leaf_order(cen.data(), n_triangles, torder);
    tri.resize((size_t)3 * n_triangles);
    for (int64_t s2 = 0; s2 < n_triangles; ++s2)
        for (int k = 0; k < 3; ++k) tri[(size_t)3 * s2 + k] = vinv[(size_t)triangles[(size_t)3 * torder[(size_t)s2] + k]];
}

namespace {

// SoA planes of host points taken in the order `order` (device position -> input index)
void gather_soa(const double *xyz, const std::vector<int32_t> &order, std::vector<double> &soa) {
    const size_t n = order.size();
    soa.resize(3 * n);
    for (size_t s2 = 0; s2 < n; ++s2)
        for (int d = 0; d < 3; ++d) soa[(size_t)d * n + s2] = xyz[(size_t)3 * order[s2] + d];
}

}  // namespace

extern "C" {

int gingr_fitter_surface_distance_stats(gingr_fitter *f, int32_t direction, int64_t n_points, const double *points,
                                        int32_t boundary_aware, double sdev, double out[4]) {
    GINGR_TRY(check_ready(f));
    gingr_ctx *ctx = f->ctx;
    if (!out || (direction != 0 && direction != 1) || n_points < 0 || !(sdev >= 0.0))
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "surface_distance_stats: bad argument");
    if (!f->Tm || !f->Tt) return gingr_set_error(ctx, GINGR_ERR_STATE, "surface_distance_stats: no meshes set (gingr_fitter_set_meshes)");
    const gingr_model *m = f->m;
    const int64_t M = m->M, N = f->N;
    const Cloud fit = cloud_of(f->fit, M), tgt = cloud_of(f->target, N);
    if (!f->stat_scratch) f->stat_scratch = new StatScratch;
    StatScratch &sc = *f->stat_scratch;
    if (direction == 0) {
        // the first n_points vertices of the current fit (original numbering; 0 = all) against the target surface
        if (points) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "surface_distance_stats: model -> target takes no point list");
        if (n_points > M) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "surface_distance_stats: more points than model vertices");
        const bool all = n_points == 0 || n_points == M;
        return run_distance_stats(ctx, fit, tgt, f->ttri, f->ttri_orig, f->Tt, f->ttboxes, all ? nullptr : m->perm, n_points, f->tperm,
                                  f->tboxes, boundary_aware ? f->tboundary : nullptr, sdev, sc, out, f->pin, f->ttribox, f);
    }
    // `points` (null: every target vertex) against the surface of the current fit
    launch_tri_tile_bbox(ctx, fit, f->mtri, f->Tm, f->mtboxes, f->mtribox);
    if (boundary_aware) launch_tile_bbox(ctx, fit, f->fboxes);
    const int32_t *bnd = boundary_aware ? f->mboundary : nullptr;
    if (!points)
        return run_distance_stats(ctx, tgt, fit, f->mtri, f->mtri_orig, f->Tm, f->mtboxes, nullptr, 0, m->perm, f->fboxes, bnd, sdev, sc,
                                  out, f->pin, f->mtribox, f);
    if (n_points < 1) return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "surface_distance_stats: empty point list");
    std::vector<int32_t> order;
    kd_leaf_order(points, n_points, order);
    std::vector<double> soa;
    gather_soa(points, order, soa);
    DevBuf q;
    HIP_TRY(ctx, q.alloc(soa.size() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(q.p, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return run_distance_stats(ctx, cloud_of(q.as<double>(), n_points), fit, f->mtri, f->mtri_orig, f->Tm, f->mtboxes, nullptr, 0, m->perm,
                              f->fboxes, bnd, sdev, sc, out);
}

int gingr_mesh_distance_stats(gingr_ctx *ctx, int64_t n_points, const double *points, int64_t n_vertices, const double *vertices,
                              int64_t n_triangles, const int32_t *triangles, int32_t boundary_aware, double sdev, double out[4]) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!points || !vertices || !triangles || !out || n_points < 1 || n_vertices < 1 || n_triangles < 1 || !(sdev >= 0.0) ||
        n_vertices > INT32_MAX || n_triangles > INT32_MAX || n_points > INT32_MAX)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_distance_stats: bad argument");
    for (int64_t k = 0; k < 3 * n_triangles; ++k)
        if (triangles[k] < 0 || triangles[k] >= n_vertices)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_distance_stats: vertex id out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> qorder, vorder, torder, vinv, tri;
    mesh_orders(n_points, points, n_vertices, vertices, n_triangles, triangles, qorder, vorder, torder, vinv, tri);
    std::vector<int32_t> bnd;
    if (boundary_aware) mark_boundary(n_triangles, triangles, vinv.data(), n_vertices, bnd);
    std::vector<double> qsoa, vsoa;
    gather_soa(points, qorder, qsoa);
    gather_soa(vertices, vorder, vsoa);
    const int64_t ntiles = ceil_div(n_triangles, 256), nvt = ceil_div(n_vertices, 256);
    DevBuf dq, dv, dtri, dorig, dtb, dvorig, dvb, dbnd;
    HIP_TRY(ctx, dq.alloc(qsoa.size() * sizeof(double)));
    HIP_TRY(ctx, dv.alloc(vsoa.size() * sizeof(double)));
    HIP_TRY(ctx, dtri.alloc(tri.size() * sizeof(int32_t)));
    HIP_TRY(ctx, dorig.alloc(torder.size() * sizeof(int32_t)));
    HIP_TRY(ctx, dtb.alloc((size_t)30 * ntiles * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(dq.p, qsoa.data(), qsoa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dv.p, vsoa.data(), vsoa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dtri.p, tri.data(), tri.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dorig.p, torder.data(), torder.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Cloud q = cloud_of(dq.as<double>(), n_points), v = cloud_of(dv.as<double>(), n_vertices);
    launch_tri_tile_bbox(ctx, v, dtri.as<int32_t>(), n_triangles, dtb.as<double>());
    if (boundary_aware) {
        HIP_TRY(ctx, dvorig.alloc(vorder.size() * sizeof(int32_t)));
        HIP_TRY(ctx, dvb.alloc((size_t)30 * nvt * sizeof(double)));
        HIP_TRY(ctx, dbnd.alloc(bnd.size() * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(dvorig.p, vorder.data(), vorder.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dbnd.p, bnd.data(), bnd.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        launch_tile_bbox(ctx, v, dvb.as<double>());
    }
    StatScratch sc;
    return run_distance_stats(ctx, q, v, dtri.as<int32_t>(), dorig.as<int32_t>(), n_triangles, dtb.as<double>(), nullptr, 0,
                              boundary_aware ? dvorig.as<int32_t>() : nullptr, boundary_aware ? dvb.as<double>() : nullptr,
                              boundary_aware ? dbnd.as<int32_t>() : nullptr, sdev, sc, out);
}

int gingr_mesh_closest_points(gingr_ctx *ctx, int64_t n_points, const double *points, int64_t n_vertices, const double *vertices,
                              int64_t n_triangles, const int32_t *triangles, double *cp_xyz, double *d2, int32_t *tri_id,
                              double *bary) {
    if (!ctx) return GINGR_ERR_BAD_ARGUMENT;
    if (!points || !vertices || !triangles || n_points < 1 || n_vertices < 1 || n_triangles < 1 || n_vertices > INT32_MAX ||
        n_triangles > INT32_MAX || n_points > INT32_MAX)
        return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_closest_points: bad argument");
    for (int64_t k = 0; k < 3 * n_triangles; ++k)
        if (triangles[k] < 0 || triangles[k] >= n_vertices)
            return gingr_set_error(ctx, GINGR_ERR_BAD_ARGUMENT, "mesh_closest_points: vertex id out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> qorder, vorder, torder, vinv, tri;
    mesh_orders(n_points, points, n_vertices, vertices, n_triangles, triangles, qorder, vorder, torder, vinv, tri);
    std::vector<int32_t> tri_by_orig((size_t)3 * n_triangles);
    for (int64_t k = 0; k < 3 * n_triangles; ++k) tri_by_orig[(size_t)k] = vinv[(size_t)triangles[(size_t)k]];
    std::vector<double> qsoa, vsoa;
    gather_soa(points, qorder, qsoa);
    gather_soa(vertices, vorder, vsoa);
    const int64_t ntiles = ceil_div(n_triangles, 256);
    DevBuf dq, dv, dtri, dorig, dtb, dcp, dd2, dtid, dtbo, dbary;
    HIP_TRY(ctx, dq.alloc(qsoa.size() * sizeof(double)));
    HIP_TRY(ctx, dv.alloc(vsoa.size() * sizeof(double)));
    HIP_TRY(ctx, dtri.alloc(tri.size() * sizeof(int32_t)));
    HIP_TRY(ctx, dtbo.alloc(tri.size() * sizeof(int32_t)));
    HIP_TRY(ctx, dorig.alloc(torder.size() * sizeof(int32_t)));
    HIP_TRY(ctx, dtb.alloc((size_t)30 * ntiles * sizeof(double)));
    HIP_TRY(ctx, dcp.alloc((size_t)3 * n_points * sizeof(double)));
    HIP_TRY(ctx, dd2.alloc((size_t)n_points * sizeof(double)));
    HIP_TRY(ctx, dtid.alloc((size_t)n_points * sizeof(int32_t)));
    HIP_TRY(ctx, dbary.alloc((size_t)3 * n_points * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(dq.p, qsoa.data(), qsoa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dv.p, vsoa.data(), vsoa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dtri.p, tri.data(), tri.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dtbo.p, tri_by_orig.data(), tri.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dorig.p, torder.data(), torder.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Cloud q = cloud_of(dq.as<double>(), n_points), v = cloud_of(dv.as<double>(), n_vertices);
    launch_tri_tile_bbox(ctx, v, dtri.as<int32_t>(), n_triangles, dtb.as<double>());
    launch_surface_closest_point(ctx, q, v, dtri.as<int32_t>(), dorig.as<int32_t>(), n_triangles, dtb.as<double>(), dcp.as<double>(),
                                 dd2.as<double>(), dtid.as<int32_t>());
    launch_barycentric(ctx, q, v, dtbo.as<int32_t>(), dtid.as<int32_t>(), dbary.as<double>());
    GINGR_TRY(check_launch(ctx));
    std::vector<double> hcp((size_t)3 * n_points), hd2((size_t)n_points), hb((size_t)3 * n_points);
    std::vector<int32_t> ht((size_t)n_points);
    HIP_TRY(ctx, hipMemcpyAsync(hcp.data(), dcp.p, hcp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hd2.data(), dd2.p, hd2.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hb.data(), dbary.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ht.data(), dtid.p, ht.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t s2 = 0; s2 < n_points; ++s2) {  // device position -> input index
        const size_t o = (size_t)qorder[(size_t)s2];
        if (cp_xyz)
            for (int d = 0; d < 3; ++d) cp_xyz[3 * o + d] = hcp[(size_t)d * n_points + s2];
        if (d2) d2[o] = hd2[(size_t)s2];
        if (tri_id) tri_id[o] = ht[(size_t)s2];
        if (bary)
            for (int d = 0; d < 3; ++d) bary[3 * o + d] = hb[(size_t)3 * s2 + d];
    }
    return GINGR_OK;
}

}  // extern "C"
