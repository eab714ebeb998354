// svo_lookup.h — where the ray's voxel lies in the tree: the parent kept in registers and the per-lane path in LDS
// (Parent, Path), the two node-addressing classes (BufNodes, WideNodes), the region lookup (lookup<OPT>) and a brick
// voxel's material.  Used by trace() in svo_trace.h and by the shading and AO code of svo_shade.h.
#pragma once

#include "svo_boxes.h"
#include "svo_exact.h"
#include "svo_stats.h"

// Region lookup of a wrapped voxel: SOLID hit, an empty child cell (returns its shift), or the
// brick holding the voxel (mask / ref / info returned).  tetrahexa_tree.cpp:124-152 on the
// breadth-first layout.
enum : uint32_t { R_EMPTY = 0u, R_BRICK = 1u, R_SOLID = 2u, R_CEIL = 3u };
// Hit.info of a shading ray that left the loop early (ESCAPE): a miss whose remaining steps are all in empty voxels
// (never written to a hit record: escaping is off when records are requested)
constexpr uint32_t ESC_BIT = 1u << 19;

// The interior node whose child region holds the ray's current cell, kept in registers: a move to
// a sibling region reads the cached child mask (no load when the sibling is empty) and restarts
// the descent at most one level down; leaving the parent's region restarts at the root, whose top
// levels are staged in LDS.
// per-lane path of the last descent in LDS
struct Path {
    // [depth][mask low, mask high, first child][lane] dwords: one address per depth (the three
    // words at +0, +256, +512 bytes: ds_write2st64 / ds_read2st64 and one more)
    uint32_t* __restrict__ w;
    __device__ __forceinline__ void put(int32_t d, uint64_t mask, uint32_t ref) const {
        uint32_t* e = w + d * (3 * kBlock);
        e[0] = (uint32_t)mask;
        e[kBlock] = (uint32_t)(mask >> 32);
        e[2 * kBlock] = ref;
    }
    __device__ __forceinline__ uint64_t mask(int32_t d) const {
        const uint32_t* e = w + d * (3 * kBlock);
        return (uint64_t)e[0] | ((uint64_t)e[kBlock] << 32);
    }
    __device__ __forceinline__ uint32_t ref(int32_t d) const { return w[d * (3 * kBlock) + 2 * kBlock]; }
};

struct Parent {
    uint64_t mask;
    uint32_t ref;
    uint32_t sh;  // child shift: a child region is 2^sh voxels wide, the parent's 2^(sh+2)
};

// Node reads.  Trees of up to kNarrowNodes nodes (4 GiB) read through a buffer resource with 32-bit
// byte offsets (one shift per load, and buffer loads are never merged with the LDS path); larger
// trees — the builders accept up to 2^32 nodes, 64 GiB — through 64-bit global addresses.  The host
// picks the instance per tree (svo_cast.hip: node_addressing), so no index can wrap or fall outside
// the resource and read zeros (an empty node) silently.
// Loads take "one past" indices: ni1 = node index + 1 = first child + rank + 1, which is the popcount
// of the child mask shifted so the child's own bit stays in (slot_top: no further shift), and the
// bases sit one node before the array.
constexpr uint64_t kNarrowNodes = 1ull << 28;  // below it, ni1 << 4 stays below 2^32

struct BufNodes {
    __amdgpu_buffer_rsrc_t rsrc;
    const Node* __restrict__ base;
    __device__ __forceinline__ explicit BufNodes(const Node* p)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<Node*>(p - 1), (short)0, (int)0xFFFFFFFFu, (int)0x00020000)), base(p) {}
    __device__ __forceinline__ Node root() const { return base[0]; }  // (uniform: a scalar load)
    __device__ __forceinline__ Node load(uint32_t ni) const {  // node ni - 1
        const uint32_t off = ni << 4;
        Node n;
        n.mask = ((uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0)) |
                 ((uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4, 0, 0) << 32);
        n.ref = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 8, 0, 0);
        n.info = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 12, 0, 0);
        return n;
    }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct WideNodes {
    const __attribute__((address_space(1))) u32x4* p;
    const Node* __restrict__ base;
    __device__ __forceinline__ explicit WideNodes(const Node* q) : p((const __attribute__((address_space(1))) u32x4*)(q - 1)), base(q) {}
    __device__ __forceinline__ Node root() const { return base[0]; }  // (uniform: a scalar load)
    __device__ __forceinline__ Node load(uint32_t ni) const {  // node ni - 1
        const u32x4 v = p[ni];  // 64-bit address: base + (u64)ni * 16
        Node n;
        n.mask = (uint64_t)v.x | ((uint64_t)v.y << 32);
        n.ref = v.z;
        n.info = v.w;
        return n;
    }
};

// lookup()'s compile-time options, one word (lookup<OPT>)
enum : uint32_t {
    L_STATS = 1u << 0,  // count into st (diagnostics)
    // the levels above the bricks hold interior nodes or SOLID regions only; a SOLID region ends the ray, so the parent
    // may be overwritten by it, and those levels need no leaf branch and no copies of the loaded node (the shading
    // pass, whose callers read the final parent's regions, keeps the general loop)
    L_SPLIT = 1u << 1,
    // (AO instances: ao_count_plan reads the final parent's shift only) a SOLID region above the bricks leaves the shift
    // of its own parent, so no path entry at or below the SOLID node is read back
    L_PSH = 1u << 2,
};
template <uint32_t OPT, class Mem>
__device__ __forceinline__ uint32_t lookup(const CastParams& P, const Mem& mem, const Path& path,
                                           const uint32_t w[3], uint32_t moved, Parent& par, uint32_t& sh_out, uint64_t& bmask,
                                           uint32_t& bref, uint32_t& binfo, Stats& st) {
    static_assert((OPT & ~(L_STATS | L_SPLIT | L_PSH)) == 0u, "lookup: unknown option");
    constexpr bool STATS = (OPT & L_STATS) != 0u, SPLIT = (OPT & L_SPLIT) != 0u, PSH = (OPT & L_PSH) != 0u;
    uint32_t ni = 0u;
    int32_t dd = 0;
    if (STATS) st.lookups++;
    {
        // the previous voxel lies in the parent's region (every move starts inside it), so the
        // bits in which the last step changed the stepped coordinate tell whether the ray left it
        const uint32_t diff = moved;
        if (diff >= (4u << par.sh)) {  // a bit at or above the parent region's size changed
            // left the parent's region: the deepest node of the last descent whose region also
            // holds this cell (depth levels-1-floor(h/2), h = highest differing bit) becomes the
            // parent, read back from the per-lane path in LDS
            const int32_t da = P.levels - 1 - (int32_t)((31u - (uint32_t)__builtin_clz(diff)) >> 1);  // (diff != 0)
            par.mask = path.mask(da);
            par.ref = path.ref(da);
            par.sh = (uint32_t)(2 * (P.levels - 1 - da));
            if (STATS) {
                st.path_starts++;
                if (da == 0) st.root_starts++;  // (back to the root, which stands in the path at depth 0: svo_trace.h)
            }
        }
        sh_out = par.sh;
        const uint64_t t = slot_top(par.mask, child_slot(w[0], w[1], w[2], par.sh));
        if ((int64_t)t >= 0) {
            if (STATS) st.cache_empty++;
            return R_EMPTY;
        }
        ni = popc_add(t, par.ref);  // (one past: BufNodes)
        dd = P.levels - (int32_t)(par.sh >> 1);  // depth of that child
        if (STATS && dd == 0) st.root_starts++;
    }
    // descend (one exit: no per-exit register copies)
    uint32_t res = R_EMPTY;
    if (SPLIT) {
        // Node ni - 1 occupies the cell and is not loaded yet.  Across the back-edge go ni, dd and one flag: dd counts
        // only the levels whose child is pending (occupied, under an interior node), so a lane leaves the loop with
        // dd == levels - 1 exactly when its brick-level node is pending (also a lane that starts there), and the
        // other lanes' outcome is read after the loop from the last node they loaded (binfo; par.sh is its shift).
        const int32_t dl = P.levels - 1;
        bool more = dd < dl;
        while (more) {
            if (STATS) {
                st.wv_descents += wave_lead();
                st.loads++;
            }
            const Node n = mem.load(ni);
            const uint32_t sh = (uint32_t)(2 * (dl - dd));
            path.put(dd, n.mask, n.ref);
            par.mask = n.mask;
            par.ref = n.ref;
            binfo = n.info;
            const uint64_t t = slot_top(n.mask, child_slot(w[0], w[1], w[2], sh));
            const bool solid = (n.info & K_KIND_MASK) == K_SOLID;
            par.sh = PSH && solid ? sh + 2u : sh;
            ni = popc_add(t, n.ref);
            const bool pend = (int64_t)t < 0 && !solid;
            dd += pend ? 1 : 0;
            more = pend && dd < dl;
        }
        // ended above the bricks: a SOLID region, or an empty child cell of the last node (shift par.sh; sh_out is read
        // for R_EMPTY only).  (Taken on every lane: the brick level's lanes overwrite it.)
        sh_out = par.sh;
        res = (binfo & K_KIND_MASK) == K_SOLID ? R_SOLID : R_EMPTY;
        if (dd == dl) {  // the brick level: a BRICK or SOLID leaf
            if (STATS) {
                st.wv_descents += wave_lead();
                st.loads++;
            }
            const Node n = mem.load(ni);
            bmask = n.mask;
            bref = n.ref;
            binfo = n.info;
            sh_out = 2u;
            res = (n.info & K_KIND_MASK) == K_SOLID ? R_SOLID : R_BRICK;
        }
        return res;
    }
    bool more = dd < P.levels;
    while (more) {
        if (STATS) {
            st.wv_descents += wave_lead();
            st.loads++;
        }
        const Node n = mem.load(ni);
        const uint32_t kind = n.info & K_KIND_MASK;
        // (read only for BRICK / SOLID results: written on every load, so the previous values need
        // no copies around it)
        bmask = n.mask;
        bref = n.ref;
        binfo = n.info;
        if (kind == K_INTERIOR) {
            const uint32_t sh = (uint32_t)(2 * (P.levels - 1 - dd));
            path.put(dd, n.mask, n.ref);
            par.mask = n.mask;
            par.ref = n.ref;
            par.sh = sh;
            const uint64_t t = slot_top(n.mask, child_slot(w[0], w[1], w[2], sh));
            const bool occ = (int64_t)t < 0;
            ni = popc_add(t, n.ref);
            dd++;
            more = occ && dd < P.levels;
            sh_out = occ ? 0u : sh;  // (occupied at the last level only in a malformed tree: one voxel)
        } else {
            sh_out = 2u;
            res = kind == K_SOLID ? R_SOLID : R_BRICK;
            more = false;
        }
    }
    return res;
}

__device__ __forceinline__ uint32_t brick_material(const uint16_t* mats, uint64_t mask, uint32_t ref, uint32_t info, uint32_t v) {
    return (info & K_UNIFORM) ? (info >> 16) : (uint32_t)mats[ref + (uint32_t)__popcll(mask & ((1ull << v) - 1ull))];
}

__device__ __forceinline__ void wrap3(const Ray& R, uint32_t wm, uint32_t w[3]) {
    w[0] = (uint32_t)R.r[0] & wm;
    w[1] = (uint32_t)R.r[1] & wm;
    w[2] = (uint32_t)R.r[2] & wm;
}
