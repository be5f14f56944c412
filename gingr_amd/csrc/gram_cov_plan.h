// Planning of the 3 x 3-weighted Gram pass (gp_gram_cov.hip): G += sum_i Q_i^T W_i Q_i, rhs += sum_i Q_i^T W_i v_i over the M local
// vertices of a rank-rp basis.  Plain C++ (compiled for the host alone by tests/test_pairs_cov_gram_host.py).
//
// The vertices are cut into slabs of whole K-steps; a workgroup takes one slab through one 64 x 64 patch of the upper triangle of G
// and leaves the patch in the slab's partial, and the workgroups of patch row 0 leave the slab's part of the right-hand side behind it.
// The reducer adds the slabs in a fixed order (eight interleaved groups, then a tree): nothing here depends on anything but (M, rp).
#pragma once

#include "host_device.h"

namespace gram_cov_plan {

constexpr int kPatch = 64;                // columns of a patch: 4 x 4 MFMA tiles of 16 x 16
constexpr int kWaves = 4;                 // waves of a workgroup; they interleave the K-steps of the slab
constexpr int kStepVerts = 4;             // vertices of one K-step: twelve basis rows, three v_mfma_f64_16x16x4_f64 per tile
constexpr int64_t kSlabQuantum = kWaves * kStepVerts;  // a slab holds whole rounds of the four waves
constexpr int64_t kMinSlabVerts = 64;     // below this a slab's rp x rp partial costs more than the rows it summarises
constexpr int kWantWorkgroups = 768;      // ~3 workgroups of 4 waves per CU over all patches
constexpr int kMaxSlabs = 768;            // what the reducer is sized for (one patch: one slab per wanted workgroup)
constexpr int kMaxRp = 512;

// one instance for every rank; the name a rank reaches (reported by tools/bench_pairs_cov.py)
enum class Instance { Patch64 = 0 };

struct Plan {
    int64_t M = 0;
    int rp = 0;
    int nbp = 0, npatch = 0;  // patches per side / upper-triangle patches (pa <= pb)
    int nslabs = 0;
    int64_t verts_per_slab = 0;
    Instance instance = Instance::Patch64;

    int64_t slab_begin(int s) const { return (int64_t)s * verts_per_slab; }
    int64_t slab_end(int s) const { return (int64_t)(s + 1) * verts_per_slab < M ? (int64_t)(s + 1) * verts_per_slab : M; }
    int64_t partial_stride() const { return (int64_t)rp * rp + rp; }  // [rp * rp] patch entries, then [rp] right-hand side
    int64_t partial_doubles() const { return (int64_t)nslabs * partial_stride(); }
    int64_t factor_doubles() const { return 9 * M; }  // per vertex: the six entries of C_i (W_i = C_i^T C_i) and W_i v_i, planes [9][M]
    int64_t workspace_doubles() const { return partial_doubles() + factor_doubles(); }
};

// rp: a multiple of 16 in 16 .. 512; M >= 1
inline Plan make_plan(int64_t M, int rp) {
    Plan p;
    p.M = M;
    p.rp = rp;
    p.nbp = (rp + kPatch - 1) / kPatch;
    p.npatch = p.nbp * (p.nbp + 1) / 2;
    int64_t want = kWantWorkgroups / p.npatch;
    const int64_t most = ceil_div(M, kMinSlabVerts);
    if (want > most) want = most;
    if (want > kMaxSlabs) want = kMaxSlabs;
    if (want < 1) want = 1;
    p.verts_per_slab = round_up(ceil_div(M, want), kSlabQuantum);
    p.nslabs = (int)ceil_div(M, p.verts_per_slab);
    return p;
}

}  // namespace gram_cov_plan
