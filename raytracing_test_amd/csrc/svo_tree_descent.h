// svo_tree_descent.h — svo_tree_get_block's descent over a resident tree's arrays in HBM, for the kernels that re-emit
// such a tree: the patches (svo_patch_cells.h: the old content where the patch does not decide) and the compaction
// (svo_compact.hip: the voxels of the old bricks), and for the lookup of scattered voxels (svo_build_points.hip:
// svo_tree_get_blocks_gpu).  T holds the arrays and the depth: T.nodes, T.mats, T.levels.
// Every node and material index is widened to 64 bits before it addresses memory.
#pragma once

#include <hip/hip_runtime.h>

#include "svo_build_emit.h"

namespace {

template <class T>
__device__ uint32_t old_voxel(const T& P, uint32_t wx, uint32_t wy, uint32_t wz) {
    uint64_t ni = 0;
    for (int d = 0; d < P.levels; d++) {
        const Node n = P.nodes[ni];
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) return node_material(n.info);
        if (kind == K_BRICK) {
            const uint32_t v = ((wz & 3u) << 4) | ((wy & 3u) << 2) | (wx & 3u);
            if (!((n.mask >> v) & 1ull)) return G_EMPTY;
            return (n.info & K_UNIFORM) ? node_material(n.info) : P.mats[(uint64_t)n.ref + (uint64_t)__popcll(n.mask & ((1ull << v) - 1ull))];
        }
        const uint32_t sh = (uint32_t)(2 * (P.levels - 1 - d));
        const uint32_t sl = (((wz >> sh) & 3u) << 4) | (((wy >> sh) & 3u) << 2) | ((wx >> sh) & 3u);
        if (!((n.mask >> sl) & 1ull)) return G_EMPTY;
        ni = (uint64_t)n.ref + (uint64_t)__popcll(n.mask & ((1ull << sl) - 1ull));
    }
    return G_EMPTY;
}

}  // namespace
