// The uniform grid over the (fixed) target triangles, host side: the binning is tri_grid_plan (tri_grid_plan.h, plain C++); this
// file owns the device copies.
#include "surface.h"

void tri_grid_free(TriGrid *g) {
    if (g->cell_start) (void)hipFree(g->cell_start);
    if (g->boxes) (void)hipFree(g->boxes);
    if (g->recs) (void)hipFree(g->recs);
    if (g->flag) (void)hipFree(g->flag);
    if (g->nflag) (void)hipFree(g->nflag);
    *g = TriGrid{};
}

// vsoa: host, the mesh vertices as SoA planes [3][n] in DEVICE order; tri: host, [3 T] vertex positions in the (spatially sorted)
// triangle order of the device.  Synchronous.  No grid (g->ready false) where the plan has none: the callers keep the tile scan.
int tri_grid_build(gingr_ctx *ctx, const double *vsoa, int64_t n, const int32_t *tri, const int32_t *tri_orig, int64_t T, int64_t max_queries,
                   TriGrid *g) {
    tri_grid_free(g);
    if (max_queries < 1) return GINGR_OK;
    TriGridPlan p;
    tri_grid_plan(vsoa, n, tri, tri_orig, T, &p);
    if (!p.ready) return GINGR_OK;
    HIP_TRY(ctx, hipMalloc(&g->boxes, p.boxes.size() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(g->boxes, p.boxes.data(), p.boxes.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMalloc(&g->recs, p.recs.size() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(g->recs, p.recs.data(), p.recs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMalloc(&g->cell_start, p.start.size() * sizeof(int32_t)));
    HIP_TRY(ctx, hipMalloc(&g->flag, (size_t)max_queries));
    HIP_TRY(ctx, hipMalloc(&g->nflag, 2 * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(g->cell_start, p.start.data(), p.start.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(g->flag, 0, (size_t)max_queries, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(g->nflag, 0, 2 * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int d = 0; d < 3; ++d) g->v.lo[d] = p.lo[d], g->v.g[d] = p.g[d], g->v.span[d] = p.span[d];
    g->v.h = p.h;
    g->v.inv_h = p.inv_h;
    g->v.cell_start = g->cell_start;
    g->v.boxes = g->boxes;
    g->v.recs = g->recs;
    g->v.n_listed = (int32_t)p.n_listed;
    g->v.n_big = (int32_t)p.n_big;
    g->max_queries = max_queries;
    g->list_entries = p.n_listed + p.n_big;
    g->ready = true;
    return GINGR_OK;
}
