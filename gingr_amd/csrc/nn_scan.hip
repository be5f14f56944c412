// Exact brute-force nearest neighbour for gfx950 (MI355X): the pruned tile scan and the all-pairs scan of small clouds.
//
// Reference loop replaced (G/ = src/main/scala/gingr/):
//   nn           : findClosestPoint per fit vertex        G/api/registration/utils/ClosestPointRegistrator.scala:139-145
//
// Exact, lowest index on ties: the distances are norm2_exact (box_device.h), the reference's own float64 expression.
#include "common.h"
#include "box_device.h"
#include "cpd_plan.h"

namespace {

// A workgroup of four waves serves 64 consecutive queries (spatially compact when the fitter keeps clouds in k-d leaf order):
// every wave holds the same queries and scans ONE 64-point quarter of each staged target tile, visited only if that quarter's box
// is not farther from a lane's query than the lane's best so far.  Tiles are found with the lanes testing 64 tile boxes at a time
// against the queries' box; the tiles at the smallest gap come first, then the four waves share their best distances (the bound
// only) and the remaining tiles are visited under that bound -- exact pruning: the result is the same as the full scan including
// the lowest-original-index tie rule (a NaN box or query never prunes).
constexpr int kNNBlock = 256;    // threads per workgroup (kNNThreads = 64 queries, cpd_plan.h)

// COUNT (diagnostics, gingr_ctx_nn_counting): *tests += the distance tests the launch really executed (64 lanes x the entries of every
// scanned quarter), one integer atomic per wave at its end -- the denominator of the kernel's roofline figure after pruning.
template <bool COUNT>
__global__ __launch_bounds__(kNNBlock) void nn_kernel(Cloud q, Cloud tgt, const int32_t *__restrict__ orig,
                                                      const double *__restrict__ tgt_boxes, int64_t cols_per_chunk,
                                                      double *__restrict__ pd2, int32_t *__restrict__ pidx,
                                                      int32_t *__restrict__ porig, const int32_t *warm /* may alias idx_out */,
                                                      unsigned long long *tests, const uint8_t *__restrict__ mask,
                                                      const int32_t *__restrict__ nmask, int32_t *idx_out,
                                                      double *__restrict__ d2_out) {
    // masked launch (the queries the grid search of nn_grid.hip left over): nothing to do at all, or nothing for these 64 queries
    if (nmask && *nmask == 0) return;
    if (mask) {
        const int64_t iq = (int64_t)blockIdx.x * kNNThreads + (threadIdx.x & 63);
        if (!__any(iq < q.n && mask[iq] != 0)) return;  // the four waves hold the same queries: a workgroup-uniform exit
    }
    unsigned long long scanned = 0;  // wave-uniform
    __shared__ P4 tile[kTile];
    __shared__ double sbest[4][kNNThreads], sorig[4][kNNThreads];
    __shared__ int32_t sidx[4][kNNThreads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kNNThreads + lane;
    const bool ok = i < q.n;
    const double qx = ok ? q.x[i] : 0.0, qy = ok ? q.y[i] : 0.0, qz = ok ? q.z[i] : 0.0;
    double best = __builtin_huge_val(), bo = __builtin_huge_val();  // best distance and the ORIGINAL index that holds it
    double bound = __builtin_huge_val();                            // best of all four waves after the first sweep
    int32_t bi = -1;
    // Warm start (nullable): the position of the target this query matched LAST time (an ICP iteration moves the queries a little).
    // Its distance, computed with the arithmetic of the scan, is a valid candidate and prunes from the first tile on; the result is
    // the same exact minimum with the same tie rule (a tile holding an equally close target has a gap <= the bound and is visited).
    if (warm && ok) {
        const int32_t p = warm[i];
        if (p >= 0 && p < tgt.n) {
            const double d2 = norm2_exact(tgt.x[p] - qx, tgt.y[p] - qy, tgt.z[p] - qz);
            if (d2 == d2) {  // a NaN query keeps the cold-start behaviour
                best = d2;
                bo = (double)(orig ? orig[p] : p);
                bi = p;
            }
        }
    }
    const int64_t j0 = (int64_t)blockIdx.y * cols_per_chunk;
    const int64_t j1 = min(tgt.n, j0 + cols_per_chunk);
    const int t0 = (int)(j0 / kTile), nt = (int)((j1 - j0 + kTile - 1) / kTile);
    const double *qboxes = tgt_boxes ? tgt_boxes + ((tgt.n + kTile - 1) / kTile) * 6 : nullptr;
    const Box wb = wave_box(ok, qx, qy, qz);  // the queries' bounding box (invalid lanes excluded)
    double gmin = __builtin_huge_val();
    if (tgt_boxes) {
        for (int t = lane; t < nt; t += 64) gmin = fmin(gmin, box_gap2(wb, tgt_boxes + (int64_t)(t0 + t) * 6));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gmin = fmin(gmin, __shfl_xor(gmin, off));
        gmin = uniform_d(gmin);
    }
    for (int phase = 0; phase < 2; ++phase) {
        if (!tgt_boxes && phase == 1) break;  // no boxes: the first sweep visits everything
        double bmax = ok ? fmin(best, bound) : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, off));
        bmax = uniform_d(bmax) * (1.0 + 1e-12);  // identical in the four waves in the second sweep (bound is shared)
        for (int tc = 0; tc < nt; tc += 64) {
            const int tl = tc + lane;
            bool take = tl < nt;
            if (tgt_boxes && take) {
                const double g = box_gap2(wb, tgt_boxes + (int64_t)(t0 + tl) * 6);
                // a NaN box gives g = NaN: taken in the first sweep
                take = phase == 0 ? !(g > gmin) : (g > gmin && !(g > bmax));
            }
            unsigned long long cand = __ballot(take);  // workgroup-uniform: same queries, same gmin / bound in every wave
            while (cand) {
                const int t = tc + __builtin_ctzll(cand);
                cand &= cand - 1;
                const int64_t jb = j0 + (int64_t)t * kTile, q0 = jb + 64 * wave;
                bool need = ok && q0 < j1;
                if (qboxes) {
                    const double *bx = qboxes + ((int64_t)(t0 + t) * 4 + wave) * 6;
                    const double gx = fmax(fmax(bx[0] - qx, qx - bx[3]), 0.0), gy = fmax(fmax(bx[1] - qy, qy - bx[4]), 0.0),
                                 gz = fmax(fmax(bx[2] - qz, qz - bx[5]), 0.0);
                    const double pd = __builtin_fma(gz, gz, __builtin_fma(gy, gy, gx * gx));
                    need = need && !(pd > fmin(best, bound) * (1.0 + 1e-12));
                }
                const bool wave_needs = __any(need);
                if (!__syncthreads_or(wave_needs)) continue;
                {
                    const int64_t j = jb + threadIdx.x;
                    if (j < j1) tile[threadIdx.x] = P4{tgt.x[j], tgt.y[j], tgt.z[j], (double)(orig ? orig[j] : (int32_t)j)};
                }
                __syncthreads();
                if (wave_needs) {
                    const int cnt = (int)min((int64_t)64, j1 - q0);
                    if (COUNT) scanned += (unsigned long long)cnt * 64ull;
#pragma unroll 4
                    for (int jj = 0; jj < cnt; ++jj) {
                        const P4 p = tile[64 * wave + jj];
                        const double d2 = norm2_exact(p.x - qx, p.y - qy, p.z - qz);
                        // strictly closer, or exactly as close with a lower original index: "lowest index wins" independent of
                        // the (spatially sorted) device order and of the visiting order
                        if (d2 < best || (d2 == best && p.w < bo)) {
                            best = d2;
                            bo = p.w;
                            bi = (int32_t)(q0 + jj);
                        }
                    }
                }
                __syncthreads();  // the tile is restaged by the next visited tile
            }
        }
        if (phase == 0 && tgt_boxes) {  // share the distance bound of the first sweep
            sbest[wave][lane] = best;
            __syncthreads();
            bound = fmin(fmin(sbest[0][lane], sbest[1][lane]), fmin(sbest[2][lane], sbest[3][lane]));
            __syncthreads();
        }
    }
    // combine the four waves: smallest distance, ties -> lowest original index
    sbest[wave][lane] = best;
    sorig[wave][lane] = bo;
    sidx[wave][lane] = bi;
    __syncthreads();
    if (wave == 0 && ok) {
        int w = 0;
        for (int k = 1; k < 4; ++k)
            if (sbest[k][lane] < sbest[w][lane] || (sbest[k][lane] == sbest[w][lane] && sorig[k][lane] < sorig[w][lane])) w = k;
        const double wo = sorig[w][lane];
        if (idx_out) {  // masked launch over ONE chunk: this is the answer (no reduction kernel follows); unflagged queries stay as they are
            if (mask[i]) idx_out[i] = sidx[w][lane], d2_out[i] = sbest[w][lane];
        } else {
            pd2[(int64_t)blockIdx.y * q.n + i] = sbest[w][lane];
            pidx[(int64_t)blockIdx.y * q.n + i] = sidx[w][lane];
            porig[(int64_t)blockIdx.y * q.n + i] = (int32_t)(wo < 2147483648.0 ? wo : -1.0);
        }
    }
    if (COUNT && lane == 0 && scanned) atomicAdd(tests, scanned);
}

__global__ void nn_reduce_kernel(const double *__restrict__ pd2, const int32_t *__restrict__ pidx,
                                 const int32_t *__restrict__ porig, int nchunks, int64_t M, int32_t *__restrict__ idx,
                                 double *__restrict__ d2, const uint8_t *__restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (mask && !mask[i]) return;  // answered by the grid search; the scan's partials may not even exist
    double best = pd2[i];
    int32_t bi = pidx[i], bo = porig[i];
    for (int c = 1; c < nchunks; ++c) {
        const double v = pd2[(int64_t)c * M + i];
        const int32_t o = porig[(int64_t)c * M + i];
        if (v < best || (v == best && o >= 0 && (bo < 0 || o < bo))) {
            best = v;
            bi = pidx[(int64_t)c * M + i];
            bo = o;
        }
    }
    idx[i] = bi;
    d2[i] = best;
}

// ---- small problems (the stateless gingr_nn of a few thousand points each; BASELINE config 2): all pairs, no boxes, no tiles.
// Pass 1: a workgroup = 512 queries (two per lane) x one slice of the targets in the CALLER's order; the whole slice goes to LDS with
// every load in flight at once, then every lane walks it with wave-uniform (broadcast) LDS reads.  Per pair the separately rounded
// expression of norm2_exact (3 subtractions, 3 products, 2 sums) and ONE minimum -- 9 instructions; which target it was is not
// tracked (a compare, a select and a move per pair for an answer 1 / nslices of the slices contribute to).
// Pass 2: sixteen lanes per query pick the first slice that holds the overall minimum (ascending slices, strict <) and search THAT
// slice again for the first target at exactly this distance (same expression, same bits): the lowest index on ties, as the full scan.
// A NaN distance never wins (v_min returns the other operand); a query with no finite distance keeps index -1, distance +inf.
__global__ __launch_bounds__(256) void nn_small_kernel(Cloud q, const double *__restrict__ tx, const double *__restrict__ ty,
                                                       const double *__restrict__ tz, int32_t n_targets, int32_t slice_len,
                                                       double *__restrict__ pd2) {
    extern __shared__ double sh[];  // [3][slice_len]
    const int tid = threadIdx.x;
    const int32_t j0 = (int32_t)blockIdx.y * slice_len, n = min(slice_len, n_targets - j0);
    double *sx = sh, *sy = sh + slice_len, *sz = sh + 2 * slice_len;
    for (int32_t k = tid; k < n; k += 256) sx[k] = tx[j0 + k], sy[k] = ty[j0 + k], sz[k] = tz[j0 + k];
    const int64_t ia = (int64_t)blockIdx.x * 512 + tid, ib = ia + 256;
    const bool oka = ia < q.n, okb = ib < q.n;
    const double ax = oka ? q.x[ia] : 0.0, ay = oka ? q.y[ia] : 0.0, az = oka ? q.z[ia] : 0.0;
    const double bx = okb ? q.x[ib] : 0.0, by = okb ? q.y[ib] : 0.0, bz = okb ? q.z[ib] : 0.0;
    __syncthreads();
    double besta = __builtin_huge_val(), bestb = __builtin_huge_val();
    int32_t j = 0;
    for (; j + 4 <= n; j += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x = sx[j + k], y = sy[j + k], z = sz[j + k];
            besta = fmin(besta, norm2_exact(x - ax, y - ay, z - az));
            bestb = fmin(bestb, norm2_exact(x - bx, y - by, z - bz));
        }
    }
    for (; j < n; ++j) {
        const double x = sx[j], y = sy[j], z = sz[j];
        besta = fmin(besta, norm2_exact(x - ax, y - ay, z - az));
        bestb = fmin(bestb, norm2_exact(x - bx, y - by, z - bz));
    }
    if (oka) pd2[(int64_t)blockIdx.y * q.n + ia] = besta;
    if (okb) pd2[(int64_t)blockIdx.y * q.n + ib] = bestb;
}

__global__ void nn_small_count_kernel(unsigned long long *tests, unsigned long long n) { *tests += n; }

__global__ __launch_bounds__(256) void nn_small_reduce_kernel(Cloud q, const double *__restrict__ tx, const double *__restrict__ ty,
                                                              const double *__restrict__ tz, int32_t n_targets, int32_t slice_len,
                                                              const double *__restrict__ pd2, int nslices, int32_t *__restrict__ idx,
                                                              double *__restrict__ d2) {
    const int l = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4), M = q.n;
    const bool ok = i < M;
    double best = __builtin_huge_val();
    int32_t bs = INT32_MAX;  // the first slice that holds `best`
    if (ok)
        for (int c = l; c < nslices; c += 16) {
            const double v = pd2[(int64_t)c * M + i];
            if (v < best) best = v, bs = c;
        }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const double v = __shfl_xor(best, off);
        const int32_t o = __shfl_xor(bs, off);
        if (v < best || (v == best && o < bs)) best = v, bs = o;
    }
    int32_t bi = INT32_MAX;
    if (ok && bs != INT32_MAX) {  // (best < +inf) the first target of slice bs at exactly this distance
        const double qx = q.x[i], qy = q.y[i], qz = q.z[i];
        const int32_t j0 = bs * slice_len, j1 = min(j0 + slice_len, n_targets);
        for (int32_t j = j0 + l; j < j1; j += 16)
            if (norm2_exact(tx[j] - qx, ty[j] - qy, tz[j] - qz) == best) {
                bi = j;
                break;
            }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) bi = min(bi, __shfl_xor(bi, off));
    if (ok && l == 0) {
        idx[i] = bi == INT32_MAX ? -1 : bi;
        d2[i] = best;
    }
}

}  // namespace

int64_t nn_ws_bytes(int64_t M, int64_t N) {
    int nch;
    int64_t len;
    plan_nn(M, N, false, &nch, &len);  // the unpruned plan has the most chunks
    return (int64_t)nch * M * (sizeof(double) + 2 * sizeof(int32_t));
}

void launch_nn(gingr_ctx *ctx, Cloud query, Cloud target, const int32_t *target_orig, const double *tgt_boxes, void *ws,
               int32_t *idx, double *d2, const int32_t *warm, const uint8_t *mask, const int32_t *nmask) {
    int nch;
    int64_t len;
    const bool pruned = ctx->cull && tgt_boxes != nullptr;
    plan_nn(query.n, target.n, pruned, &nch, &len);
    // masked (the leftovers of the grid search, normally none): one chunk from 4096 queries on, and then the scan kernel writes the
    // answers itself -- one launch that exits at once instead of two
    if (mask && pruned && query.n >= 4096) nch = 1, len = round_up(target.n, kTile);
    const bool direct = mask && nch == 1;
    double *pd2 = reinterpret_cast<double *>(ws);
    int32_t *pidx = reinterpret_cast<int32_t *>(pd2 + (int64_t)nch * query.n);
    int32_t *porig = pidx + (int64_t)nch * query.n;
    dim3 grid((unsigned)ceil_div(query.n, kNNThreads), (unsigned)nch);
    {
        TimerScope ts(ctx, 8);
        if (ctx->nn_tests)
            hipLaunchKernelGGL(nn_kernel<true>, grid, dim3(kNNBlock), 0, ctx->stream, query, target, target_orig,
                               pruned ? tgt_boxes : (const double *)nullptr, len, pd2, pidx, porig, warm, ctx->nn_tests, mask, nmask,
                               direct ? idx : (int32_t *)nullptr, direct ? d2 : (double *)nullptr);
        else
            hipLaunchKernelGGL(nn_kernel<false>, grid, dim3(kNNBlock), 0, ctx->stream, query, target, target_orig,
                               pruned ? tgt_boxes : (const double *)nullptr, len, pd2, pidx, porig, warm, (unsigned long long *)nullptr,
                               mask, nmask, direct ? idx : (int32_t *)nullptr, direct ? d2 : (double *)nullptr);
    }
    if (direct) return;
    hipLaunchKernelGGL(nn_reduce_kernel, dim3((unsigned)ceil_div(query.n, 256)), dim3(256), 0, ctx->stream, pd2, pidx, porig,
                       nch, query.n, idx, d2, mask);
}

// all pairs of two small clouds in the caller's order (see nn_small_kernel); ws: nn_small_ws_bytes(M, N)
bool nn_small_applies(int64_t M, int64_t N) { return M >= 1 && N >= 1 && N <= INT32_MAX / 2 && M * N <= (int64_t)1 << 26; }
int64_t nn_small_ws_bytes(int64_t M, int64_t N) { return (int64_t)nn_small_slices(M, N) * M * sizeof(double); }
void launch_nn_small(gingr_ctx *ctx, Cloud query, Cloud target, void *ws, int32_t *idx, double *d2) {
    const int ns = nn_small_slices(query.n, target.n);
    const int32_t len = (int32_t)ceil_div(target.n, ns);
    const int nslices = (int)ceil_div(target.n, len);
    double *pd2 = reinterpret_cast<double *>(ws);
    TimerScope ts(ctx, 8);  // (both launches: the slices mean nothing before they are combined)
    hipLaunchKernelGGL(nn_small_kernel, dim3((unsigned)ceil_div(query.n, 512), (unsigned)nslices), dim3(256), (size_t)3 * len * sizeof(double),
                       ctx->stream, query, target.x, target.y, target.z, (int32_t)target.n, len, pd2);
    hipLaunchKernelGGL(nn_small_reduce_kernel, dim3((unsigned)ceil_div(query.n, 16)), dim3(256), 0, ctx->stream, query, target.x, target.y,
                       target.z, (int32_t)target.n, len, pd2, nslices, idx, d2);
    if (ctx->nn_tests)  // diagnostics (gingr_ctx_nn_counting): every lane of every wave tests every target
        hipLaunchKernelGGL(nn_small_count_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->nn_tests,
                           (unsigned long long)round_up(query.n, 64) * (unsigned long long)target.n);
}
