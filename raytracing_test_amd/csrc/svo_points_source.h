// svo_points_source.h — the emitter's source over a sparse list of voxels (svo_build_points.hip).  What the list leaves
// after its duplicates, its empty ids and the tree's view are resolved is held as sorted arrays of occupied cells, one
// pair per level: level 0 the stored voxels with their ids, level k = 1..levels the aligned 4^k cells that hold any,
// each with its class — a palette id when all 64 children carry that one id, P_MIXED otherwise.  A cell that is absent
// is empty.  A cell's key has 6 bits per tree level above it, the emitter's slot bits z<<4 | y<<2 | x with the top level
// first: key order is the emitter's breadth-first child order, and a cell's parent is key >> 6.  Seven levels make 42
// bits; keys are 64-bit throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svo_build_emit.h"

namespace {

constexpr uint32_t P_MIXED = 0xFFFFu;  // 16-bit class words (ids are below 65535)

// the key of voxel (x, y, z) of a tree `levels` deep; the key of the 4^k cell holding it is voxel_key >> 6k
__host__ __device__ __forceinline__ uint64_t voxel_key(uint32_t x, uint32_t y, uint32_t z, int32_t levels) {
    uint64_t key = 0;
    for (int d = 0; d < levels; d++) {
        const uint32_t sh = (uint32_t)(2 * (levels - 1 - d));
        key = (key << 6) | (uint64_t)((((z >> sh) & 3u) << 4) | (((y >> sh) & 3u) << 2) | ((x >> sh) & 3u));
    }
    return key;
}

struct PointSource {
    const uint64_t* key[kMaxPyr];  // level k = 0..levels: the occupied cells' keys, ascending, each once
    const uint16_t* cls[kMaxPyr];  // their classes (level 0: the voxels' ids)
    int64_t n[kMaxPyr];
    int32_t levels;

    // index of `key` among level k's cells, -1: absent
    __device__ __forceinline__ int64_t find(int k, uint64_t want) const {
        const uint64_t* a = key[k];
        int64_t lo = 0, hi = n[k];
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        return (lo < n[k] && a[lo] == want) ? lo : -1;
    }
    __device__ uint32_t classify(int32_t x0, int32_t y0, int32_t z0, int32_t, int k) const {
        const int64_t i = find(k, voxel_key((uint32_t)x0, (uint32_t)y0, (uint32_t)z0, levels) >> (6 * k));
        if (i < 0) return G_EMPTY;
        const uint32_t c = cls[k][i];
        return c == P_MIXED ? G_MIXED : c;
    }
    __device__ uint32_t voxel(int32_t x, int32_t y, int32_t z) const {
        const int64_t i = find(0, voxel_key((uint32_t)x, (uint32_t)y, (uint32_t)z, levels));
        return i < 0 ? G_EMPTY : (uint32_t)cls[0][i];
    }
};

}  // namespace
