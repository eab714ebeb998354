// svo_diff_pair.h — the pair logic of svo_tree_diff_gpu (svo_diff_voxels.hip), shared by its kernels and the host: no HIP,
// so it also builds with g++ and runs on a CPU (tests/sanitize/diff_voxels_plan_sanitize.cpp).  The diff walks two trees
// of equal levels side by side; an item is one aligned region with a *side* per tree.  A side is a Node: either a copy of
// the record a descent of that tree reads at the region, or, below a K_SOLID ancestor or an unset slot, the synthesised
// "uniform id u" (diff_uniform: kind K_SOLID, material u, u = 0 for empty), which is never read from memory.  A real
// record is uniform too when it is K_SOLID or stores nothing (mask 0, whatever its kind); a full one-material brick that
// stayed a brick is not: it is read voxel by voxel for what it stores.
#pragma once

#include <stdint.h>

#include "svo_common.h"

namespace svo {

SVO_HD uint32_t diff_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// the side "every voxel of the region holds id u" (u = 0: the region is empty)
SVO_HD Node diff_uniform(uint32_t u) { return Node{u ? ~0ull : 0ull, 0u, K_SOLID | (u << 16)}; }

// does the side hold one id throughout?  *u: that id.  brick_depth: the region is a brick's (depth levels - 1), where the
// only record with content of its own is a brick; above it, an interior record.  A record of the other kind does not occur
// in a tree the library built and counts as empty, so that neither its ref nor its mask is ever followed.
SVO_HD bool diff_side_uniform(const Node& s, bool brick_depth, uint32_t* u) {
    const uint32_t kind = node_kind(s.info);
    if (kind == K_SOLID) {
        *u = node_material(s.info);
        return true;
    }
    *u = 0;
    return s.mask == 0ull || kind != (brick_depth ? K_BRICK : K_INTERIOR);
}

// the classification "both uniform": such a pair is never an item of a list; its total is 0 or its clipped volume
SVO_HD bool diff_both_uniform(const Node& a, const Node& b, bool brick_depth, uint32_t* ua, uint32_t* ub) {
    const bool fa = diff_side_uniform(a, brick_depth, ua), fb = diff_side_uniform(b, brick_depth, ub);
    return fa && fb;
}

// the child slots a side above brick depth may differ from emptiness in: all 64 below a uniform non-empty side
SVO_HD uint64_t diff_slot_mask(const Node& s) {
    uint32_t u;
    if (diff_side_uniform(s, false, &u)) return u ? ~0ull : 0ull;
    return s.mask;
}

// the state of child slot sl of a side that stands above brick depth; nodes: that side's tree
SVO_HD Node diff_child(const Node& s, const Node* nodes, uint32_t sl) {
    uint32_t u;
    if (diff_side_uniform(s, false, &u)) return diff_uniform(u);
    if (!((s.mask >> sl) & 1ull)) return diff_uniform(0u);
    return nodes[(uint64_t)s.ref + (uint64_t)diff_popc(s.mask & ((1ull << sl) - 1ull))];
}

// the id of voxel v of a side at brick depth; mats: that side's tree
SVO_HD uint32_t diff_voxel_id(const Node& s, const uint16_t* mats, uint32_t v) {
    uint32_t u;
    if (diff_side_uniform(s, true, &u)) return u;
    if (!((s.mask >> v) & 1ull)) return 0u;
    if (s.info & K_UNIFORM) return node_material(s.info);
    return (uint32_t)mats[(uint64_t)s.ref + (uint64_t)diff_popc(s.mask & ((1ull << v) - 1ull))];
}

}  // namespace svo
