// Host-side bookkeeping of the kernel extension (model_extend.hip): which pivots of a GPMM build belong to which coordinate, and how
// the extension pass cuts its work.  Plain C++ (no HIP, no context).
#pragma once

#include <cstdint>
#include <vector>

namespace model_extend_plan {

constexpr int kWaveRows = 16;    // new points per wave = rows of one float64 MFMA tile
constexpr int kWaves = 4;        // waves per workgroup, each with 16 points of its own
constexpr int kChunkTiles = 4;   // 16-column tiles of the result a wave keeps in registers (3 x 4 accumulator tiles)
constexpr int kChunkCols = 16 * kChunkTiles;
constexpr int kPivotStep = 4;    // pivots per MFMA step: lists and coefficient rows are padded to a multiple of it

inline int32_t padded(int32_t n) { return (n + kPivotStep - 1) / kPivotStep * kPivotStep; }
inline int chunks(int32_t rp) { return (rp + kChunkCols - 1) / kChunkCols; }
inline int64_t point_blocks(int64_t points) { return (points + kWaveRows * kWaves - 1) / (kWaveRows * kWaves); }

// The pivots of coordinate d in pivot order: ord[d][j] = ordinal in the build's pivot sequence, ids[d][j] = point of the reference.
//   shared kernel (scalar factorisation over the points): pivot i is point pivots[i]; coordinate d uses the leading cnt[d] of them
//   generic factorisation over the (point, coordinate) entries: pivot i is entry pivots[i] = 3 point + coordinate
struct Lists {
    std::vector<int32_t> ord[3], ids[3];
};

inline Lists pivot_lists(const int32_t *pivots, int32_t n, bool generic, const int32_t cnt[3]) {
    Lists l;
    for (int32_t i = 0; i < n; ++i) {
        if (generic) {
            const int d = pivots[i] % 3;
            l.ord[d].push_back(i);
            l.ids[d].push_back(pivots[i] / 3);
        } else {
            for (int d = 0; d < 3; ++d)
                if (i < cnt[d]) {
                    l.ord[d].push_back(i);
                    l.ids[d].push_back(pivots[i]);
                }
        }
    }
    return l;
}

}  // namespace model_extend_plan
