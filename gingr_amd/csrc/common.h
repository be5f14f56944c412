// Internal definitions shared by the translation units of libgingr_hip.so (gfx950 only).
#pragma once
#include <cstdlib>

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gingr_hip.h"
#include "host_device.h"

#define GINGR_TIMERS 30

struct gingr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    char err[512] = {0};
    // timing hooks (bench roofline): per-kernel event pairs recorded on `stream`
    bool timing = false;
    struct Span {
        hipEvent_t a, b;
        int which;
    };
    std::vector<Span> spans;     // recorded, not yet resolved
    std::vector<hipEvent_t> pool;  // recycled events
    double t_ms[GINGR_TIMERS] = {0};
    int64_t t_n[GINGR_TIMERS] = {0};
    // exact-zero tile culling of the CPD passes and exact pruning of the closest-point scans (cpd_pairs.hip, nn_scan.hip); gingr_ctx_set_option
    // (GINGR_OPT_CULL, 0) disables both (results must stay bit-identical: the culling test compares the two)
    int cull = 1;
    // GINGR_OPT_TRI_GRID: closest surface point over the target's triangle grid (surface.hip) in front of the tile scan: 0 never, 1 from
    // kTriGridMinTriangles target triangles on (default), 2 always.  Bit-identical results either way.
    int tri_grid = 1;
    int nn_grid = 1;  // GINGR_OPT_NN_GRID: closest point over the target's uniform grid (nn_grid.hip); 0 = the tile scan alone; 2 = gingr_nn too
    // Culling regime of the CPD passes as the DEVICE last saw it (0 plain, 1 quarter-tile culling pays): pinned host word the
    // all-pairs kernels write, read -- unsynchronised, possibly a few launches stale -- when the next launch picks its kernel
    // variant.  Both variants compute bit-identical results, so a stale value only costs time.  Null: always the plain variant.
    int32_t *regime_host = nullptr, *regime_dev = nullptr;
    int fine_override = -1;  // GINGR_OPT_FINE_CULL 0|1 pins the variant (tests: both must give bit-identical results); -1: by regime
    // diagnostics (gingr_ctx_nn_counting): device counter of the distance tests the nearest-neighbour launches really execute; null = off
    unsigned long long *nn_tests = nullptr;
    // native RCCL exchange (rccl_exchange.hip): the communicator of this rank, owned by the context; null = none
    void *rccl_comm = nullptr;
    int32_t rccl_world = 0, rccl_rank = 0;
    // GINGR_OPT_SPLIT_EXCHANGE: the column-sum exchange in two halves, the first on a second stream of the context behind the first
    // half of pass 1 (fitter_phases.hip: fitter_sharded_update).  side_stream / the events are created on first use; exchange_stream is
    // where the native all-reduce is enqueued right now (nullptr = the context's stream).
    int split_exchange = 0;
    int gram_downdate = -1;  // GINGR_OPT_GRAM_DOWNDATE: 0 / 1 weights of the surface ICP -> the model's moment minus the rejected rows (fitter_phases.hip: phase1_gram); -1: by size
    int separable = -1;  // GINGR_OPT_SEPARABLE: -1 the compact passes of a coordinate-separable model where they apply (fitter_phases.hip: use_compact); 0 never
    int decimate_batch = 16;  // GINGR_OPT_DECIMATE_BATCH: bisection steps of gingr_mesh_decimate enqueued per read-back of its control block
    hipStream_t side_stream = nullptr, exchange_stream = nullptr;
    hipEvent_t split_ev[2] = {nullptr, nullptr};
    // scratch kept across calls (grown on demand, never shrunk) so steady-state updates do not allocate
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
};

int gingr_set_error(gingr_ctx *ctx, int code, const char *fmt, ...);
void gingr_ctx_rccl_release(gingr_ctx *ctx);  // rccl_exchange.hip: destroys the context's communicator, if any

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess)                                                                               \
            return gingr_set_error((ctx), GINGR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                   __FILE__, __LINE__);                                                      \
    } while (0)

#define GINGR_TRY(expr)          \
    do {                         \
        int s__ = (expr);        \
        if (s__ != GINGR_OK) return s__; \
    } while (0)

// While a handle is being built: a failed HIP call clears the runtime's sticky error (a refused allocation must not surface again in the
// next call's launch check), leaves its text as the message and returns fail(code) -- `fail` destroys the half-built handle.
#define HANDLE_TRY(ctx, fail, expr)                                                              \
    do {                                                                                         \
        if ((expr) != hipSuccess) {                                                              \
            (void)hipGetLastError();                                                             \
            return fail(gingr_set_error((ctx), GINGR_ERR_HIP, "%s: %s", __func__, #expr));       \
        }                                                                                        \
    } while (0)

// did the launches so far go through?
inline int check_launch(gingr_ctx *ctx) {
    HIP_TRY(ctx, hipGetLastError());
    return GINGR_OK;
}

// RAII device buffer for the stateless operators
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n) {
        release();
        bytes = n;
        const hipError_t e = hipMalloc(&p, n ? n : 8);
        static const bool poison = getenv("GINGR_DEBUG_POISON") != nullptr;  // (diagnostic: see dev_alloc, fitter.h)
        if (e == hipSuccess && poison) {
            (void)hipMemset(p, 0xFF, n ? n : 8);
            (void)hipDeviceSynchronize();
        }
        return e;
    }
    template <typename T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};

// Raise a kernel's dynamic-LDS limit -- ONCE per device, function and size, under a lock.  hipFuncSetAttribute in front of every launch
// (rounds 1-5) is a race in a device group, where one host thread per shard launches the same kernels: a launch that overlaps another
// thread's hipFuncSetAttribute on the same function can be rejected, nothing runs, and the consumer reads the previous iteration's
// partials (a 0.2 % flake of the three-shard rank-150 tests, unmasked by tools/experiments/stress_group2.py).
void set_dynamic_lds(const void *func, int bytes);
template <typename K>
inline void set_dynamic_lds(K *kern, size_t bytes) {
    set_dynamic_lds(reinterpret_cast<const void *>(kern), (int)bytes);
}

struct TimerScope {
    gingr_ctx *ctx;
    int which;
    hipEvent_t a = nullptr, b = nullptr;
    TimerScope(gingr_ctx *c, int w);
    void stop();
    ~TimerScope();
};

// All launchers are asynchronous on the context's stream.
// Points on the device are SoA: x[n], y[n], z[n] contiguous planes of one allocation (plane stride = n).
struct Cloud {
    const double *x, *y, *z;
    int64_t n;
};

// ---------------------------------------------------------------------------- cpd_pairs.hip (the two all-pairs passes of CPD)
// workspace sizes (in doubles) the launchers need
int64_t cpd_colsum_ws_doubles(int64_t M, int64_t N);
int64_t cpd_rowstats_ws_doubles(int64_t M, int64_t N);
// den_partial[N] = sum_{i in fit} exp(-|x_j - y_i|^2 / (2 sigma2))   (no outlier constant)
// aux (GINGR_AUX doubles on the device): [2..4] centroid of the target cloud (launch_cloud_centroid); [0] / [1] largest
// |coordinate - centroid| of the target / fit cloud (launch_cloud_absmax).  From them the kernels decide, wave-uniformly,
// (a) whether the exponent argument needs clamping and (b) whether the cheaper norm-expansion form of c|x-y|^2 is
// accurate enough (cpd_pairs.hip: use_expansion).
#define GINGR_AUX 8
// returns the number of chunk partials left in ws ([chunk][N]); den_partial == nullptr skips their reduction (the caller passes
// ws and the count to launch_cpd_den_finalize, which then adds them up itself: single shard, one launch less)
// forced_chunks > 0: exactly that many chunks of the streamed rows, balanced to a quarter (a half of a split column-sum pass keeps
// the launch's workgroup count by taking twice the chunks of the whole pass)
int launch_cpd_colsum(gingr_ctx *ctx, Cloud fit, Cloud target, const double *sigma2_dev, const double *aux,
                      const double *fit_boxes, double *ws, double *den_partial, int forced_chunks = 0);
int cpd_colsum_chunks(int64_t M, int64_t N);  // chunks of the planner's own choice
// den[j] += c; inv_den[j] = 1/den[j]; Pt1[j] = (den[j]-c)/den[j]; xPx block partials -> part[0..256)
// M_total enters the outlier constant c = w/(1-w) (2 pi sigma2)^1.5 M_total/N.  part: GINGR_SCALAR_PART doubles.
// tile_bad[tile] (nullable) is set when a 1/den of the tile is not finite: such tiles are never culled.
#define GINGR_SCALAR_PART 1024
void launch_cpd_den_finalize(gingr_ctx *ctx, Cloud target, const double *sigma2_dev, double w, int64_t M_total,
                             double *den, double *inv_den, double *Pt1, int32_t *tile_bad, double *part,
                             double *scalars_dev, const double *chunk_partial = nullptr, int nchunks = 0);
// CPD observations fused into the row-statistics reduction (rowstats_reduce_kernel): pointers into the model / state
struct CpdObsArgs {
    const double *ref, *mean;       // SoA planes of the local rows
    const double *sigma2;           // device scalars of the state: sigma2, R (row-major 3x3), center, translation
    const double *R, *center, *t;
    double lambda;
    const int32_t *lm_mask;         // nullable
    double *weight, *evec;          // out: [M], SoA [3][M]; weight == nullptr: no observations
};
// the four block-partial arrays (GINGR_SCALAR_BLOCKS entries each) the CPD passes leave in `part`: slot 0 xPx (den_finalize),
// 1 Np, 2 trPXY, 3 yPy (rowstats_reduce); scalar index of slot q: {1, 0, 2, 3}[q]
#define GINGR_SCALAR_BLOCKS 256
// P1[i], PX (SoA planes px,py,pz of stride M) for the local rows; Np/xPx/trPXY/yPy sums into scalars_dev[0..3]
// xch8 (nullable): the 8 scalars of the exchange segment {Np, xPx (only when contribute_xpx), trPXY, yPy, 0...}
void launch_cpd_rowstats(gingr_ctx *ctx, Cloud fit, Cloud target, const double *sigma2_dev, const double *aux,
                         const double *inv_den, const double *tgt_boxes, const int32_t *tile_bad, double *ws, double *P1,
                         double *PX_soa, double *part, double *scalars_dev, double *xch8 = nullptr, int contribute_xpx = 1,
                         const CpdObsArgs *obs = nullptr, bool finish_scalars = true);
// ---------------------------------------------------------------------------- nn_scan.hip (exact nearest neighbour)
int64_t nn_ws_bytes(int64_t M, int64_t N);
// all pairs of two small clouds, both in the caller's order: one launch of ~4 000 single-wave workgroups + the combination of their
// slices (nn_scan.hip: nn_small_kernel); the stateless gingr_nn uses it where it applies
bool nn_small_applies(int64_t M, int64_t N);
int64_t nn_small_ws_bytes(int64_t M, int64_t N);
void launch_nn_small(gingr_ctx *ctx, Cloud query, Cloud target, void *ws, int32_t *idx, double *d2);
// idx[i] = POSITION (in the device order of `target`) of the nearest target; exact ties are broken by the lowest ORIGINAL
// index, taken from target_orig[position] (nullptr: the device order is the original order).
// tgt_boxes (nullable): bounding boxes of the 256-point target tiles (launch_tile_bbox) for exact nearest-first pruning.
// mask / nmask (nullable, device): only queries with mask[i] != 0 are answered (idx / d2 of the others are left alone) and the
// launch is a no-op when *nmask == 0 (launch_nn_grid leaves both behind: NNGrid::flag, NNGrid::cur_nflag()).
void launch_nn(gingr_ctx *ctx, Cloud query, Cloud target, const int32_t *target_orig, const double *tgt_boxes, void *ws,
               int32_t *idx, double *d2, const int32_t *warm = nullptr, const uint8_t *mask = nullptr,
               const int32_t *nmask = nullptr);
// ---------------------------------------------------------------------------- nn_grid.hip (closest point over a uniform grid)
struct GridPoint {  // one target, in cell order: coordinates, original index (tie rule), position in the device order of the cloud
    double x, y, z;
    int32_t orig, pos;
};
struct NNGridDev {  // what the kernel needs, by value
    double lo[3];
    double h, inv_h;
    int32_t g[3];
    const int32_t *cell_start;  // [g0 g1 g2 + 1], x fastest
    const GridPoint *pts;       // [n]
    int32_t brute_n;            // n when the cloud is small enough for uncertified queries to scan all of it in the kernel, else 0
};
struct NNGrid {  // owner
    NNGridDev v{};
    int32_t *cell_start = nullptr;
    void *pts = nullptr;
    uint8_t *flag = nullptr;   // [max_queries]: queries the grid could not certify (launch_nn_grid writes every entry)
    // how many of them: two counters used alternately -- a search counts into one and clears the other for the next search, so the
    // masked scan that follows only reads (no reset kernel, no reset by a kernel that others still read)
    int32_t *nflag = nullptr;
    int parity = 0;
    int64_t n = 0, max_queries = 0;
    bool ready = false;
    const int32_t *cur_nflag() const { return nflag + parity; }  // the counter of the LAST launch_nn_grid
};
int nn_grid_build(gingr_ctx *ctx, const double *target_xyz, int64_t N, const int32_t *perm, int64_t max_queries, NNGrid *g);
void nn_grid_free(NNGrid *g);
bool launch_nn_grid(gingr_ctx *ctx, Cloud query, Cloud target, const int32_t *target_orig, NNGrid &g, const int32_t *warm,
                    int32_t *idx, double *d2);
// ---------------------------------------------------------------------------- cloud_knn.hip (k nearest neighbours, normals)
// gingr_cloud_normals on a cloud that lies on the device (SoA; orig: device position -> the caller's index, nullable = the same): the
// normal of the point at position t goes to normals[t * point_stride + axis * axis_stride], its variation (nullable) to variation[t].
// viewpoint: host, nullable.  Synchronises.
int cloud_normals_device(gingr_ctx *ctx, Cloud c, const int32_t *orig, int32_t k, const double *viewpoint, double *normals, int64_t point_stride,
                         int64_t axis_stride, double *variation, gingr_cloud_knn_info *info, const char *who);
// gingr_cloud_knn on a cloud that lies on the device in the caller's order (SoA): idx / d2 [N][k] on the device, d2 nullable, row t the
// list of the point at position t.  Checks k.  Synchronises; the lists stay on the device (feature_align.hip reads them there).
int cloud_knn_device(gingr_ctx *ctx, Cloud c, int32_t k, int32_t *idx, double *d2, gingr_cloud_knn_info *info, const char *who);
// ---------------------------------------------------------------------------- cloud_ops.hip (per-cloud kernels, layouts, k-d order)
void launch_cloud_centroid(gingr_ctx *ctx, Cloud c, double *out3);
void launch_cloud_absmax(gingr_ctx *ctx, Cloud c, const double *ctr, double *slot);
// boxes[tile] = {lo[3], hi[3]} of every 256-point tile of a cloud: input of the exact-zero tile culling
// with absmax_slot != nullptr also *absmax_slot = max |coordinate - ctr| (same value launch_cloud_absmax produces); the slot
// must have been zeroed by an earlier launch on the stream
void launch_tile_bbox(gingr_ctx *ctx, Cloud c, double *boxes, const double *ctr = nullptr, double *absmax_slot = nullptr);
void launch_gauss_block(gingr_ctx *ctx, Cloud A, Cloud B, double sigma, double scaling, double *out);
// sum over all pairs of |a_i - b_j|^2 (computeInitialSigma2, CPD.scala:81-90); ws: sumsq_pairs_ws_doubles(A.n) doubles
int64_t sumsq_pairs_ws_doubles(int64_t nA);
void launch_sumsq_pairs(gingr_ctx *ctx, Cloud A, Cloud B, double *ws, double *out_scalar);

// interleaved xyz (n*3) <-> SoA planes; perm (nullable) maps device position -> original index:
// soa[s] = aos[perm[s]] resp. aos[perm[s]] = soa[s]
void launch_aos_to_soa(gingr_ctx *ctx, const double *aos, int64_t n, double *soa, const int32_t *perm = nullptr);
void launch_soa_to_aos(gingr_ctx *ctx, const double *soa, int64_t n, double *aos, const int32_t *perm = nullptr);
// host xyz -> stage -> SoA planes on the device, and the way back; stage: 3 n doubles on the device.  Both return a status and
// synchronise (the staging buffer is free again, a downloaded cloud is there)
int upload_cloud(gingr_ctx *ctx, double *stage, const double *xyz, int64_t n, double *soa, const int32_t *perm = nullptr);
int download_cloud(gingr_ctx *ctx, double *stage, const double *soa, int64_t n, double *xyz, const int32_t *perm = nullptr);
// *out = factor sum_ij |a_i - b_j|^2 / (3 nB nA), the first variance of the CPD family (RigidCPD.initializeGaussianKernel, :46-57;
// BCPD: factor = gamma); ws as for launch_sumsq_pairs, slot: one double on the device, which keeps the sum.  Synchronises.
int first_variance(gingr_ctx *ctx, Cloud A, Cloud B, double factor, double *ws, double *slot, double *out);
// The end of an iterate call: the launch check, then the handle's `words` (<= 2) flag words come back (synchronises).  Where word
// `decides` holds a code the words are cleared and the code is returned, with "<name>: system not positive definite" for
// GINGR_ERR_NOT_SPD and "<name>: non-finite result" otherwise.
int finish_iterate(gingr_ctx *ctx, int32_t *flags, int words, int decides, const char *name);
// out[perm[s]] = in[s]  (perm nullable = copy)
void launch_scatter(gingr_ctx *ctx, const double *in, int64_t n, const int32_t *perm, double *out);
// spatial (balanced k-d tree, leaf = one 256-point tile) order of interleaved points: perm[s] = original index of the
// point stored at device position s
void kd_leaf_order(const double *xyz, int64_t n, std::vector<int32_t> &perm);
