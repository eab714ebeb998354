// svo_patch_cells.h — the one descent by which every patch changes a resident tree on the device (svo_patch_volume.hip:
// a dense box; svo_patch_points.hip: a sparse list of edits; svo_patch_shapes.hip: boxes and balls; svo_patch_tree.hip: a
// box of another tree).  Level-synchronous from the anchor: one wavefront per item (a region that is re-emitted), lane =
// child slot (voxel at the brick level), ballots for the masks, exclusive scans (hipCUB) for child-block and material-run
// offsets, a count pass and a write pass per level, then a brick pass (k_brick_count / k_brick_write's rules over the
// composite voxels), all into scratch; commit_cells puts the result into the tree (svo_patch_commit.h).  A child slot
// becomes nothing, a K_SOLID record, the old record copied (it keeps its subtree), or an item of the next level: a new
// child block at the tail.  Re-emitted interior regions are not re-collapsed, and a brick that would store no voxel
// clears its slot bit instead, so no K_BRICK record with mask 0 exists.
// The patch is a class P, passed to the kernels by value:
//   P.nodes, P.nbase    the resident tree's records (read only: the patch is written to scratch); scratch record s >= 1
//                       becomes node nbase + s - 1 of the tree
//   P::Item             an item of a level's list: `node`, the place of its record among the scratch records (0 is the
//                       anchor's), and `old`, `kind`, what the tree held there (svo_plan.h P_NODE / P_UNIFORM / P_EMPTY:
//                       a node index or a material); then whatever else the patch's own functions need
//   child_of(P, it, on, sl, cs, k)   what slot sl of item `it` becomes (children cs = 4^k voxels wide, k >= 1; on: the old
//                       record of a P_NODE item): a struct with `what` (CH_*) and `a`, plus what next_item needs
//   next_item(P, it, c, sl, cs, node)   the next level's item of a CH_NEXT child c, its record at scratch index `node`
//   brick_voxel(P, it, v)            the composite voxel v (z<<4 | y<<2 | x) of a brick item
//   superseded(P, it, on, c, sl)     optional, called by every lane of the count pass: the patch counts there what it
//                       supersedes (the patches that do not define it count on the host)
// and descend_cells takes the first item (the anchor's) from the caller.
// The cell-asking patches (all but the points patch) share one Item (coordinates), one child_of, next_item and
// brick_voxel, written here over two questions:
//   P.relation(x, y, z, cs, k, &id)   the cell of cs = 4^k voxels (k >= 1) against the patch: svo_shape_cell.h's numbers
//   P.voxel(x, y, z, &id)             true when the patch decides the voxel, *id then what it stores
//   P.mats, P.levels                  with P.nodes what old_voxel reads (svo_tree_descent.h) where the patch does not decide
//   P::kFull                          whether relation() ever answers SHAPE_FULL
//   * an OUT cell keeps its record and its subtree (below a K_SOLID region: a synthesised K_SOLID, below an empty one
//     nothing);
//   * an IN cell is one K_SOLID record of the id at whatever level it sits, or a clear slot bit for id 0: nothing is read
//     for it;
//   * a CUT cell is re-emitted one level down, carrying only what the tree held: every child asks the patch anew.  A cut
//     brick is classified from its 64 composite voxels (the patch's, else the old tree's);
//   * a FULL cell is re-emitted one level down as though the tree held nothing there (P_EMPTY): the patch decides every
//     voxel of it, so nothing of the old tree is read for it or below it, and a FULL brick stores a voxel.
// Every node and material index is widened to 64 bits before it addresses memory.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_patch_commit.h"
#include "svo_plan.h"
#include "svo_shape_cell.h"
#include "svo_tree_descent.h"

namespace {

// what a child slot of an item becomes
enum : uint32_t { CH_NONE = 0u, CH_SOLID = 1u, CH_COPY = 2u, CH_NEXT = 3u };

// the old record of an item (nothing is read for one that holds none)
template <class P>
__device__ __forceinline__ Node old_record(const P& T, const typename P::Item& it) {
    return it.kind == P_NODE ? T.nodes[(uint64_t)it.old] : Node{0ull, 0u, K_INTERIOR};
}

// the patches that count what they supersede on the host define no hook of their own
template <class P, class C>
__device__ __forceinline__ void superseded(const P&, const typename P::Item&, const Node&, const C&, uint32_t) {}

// ---- the cell-asking patches' item and functions

// a cut cell of one level's list: its first voxel, where its record goes and what the tree held there
struct Item {
    int32_t x0, y0, z0;
    uint32_t node, old, kind;
};

// the composite: the patch's id where it decides the voxel, the old tree's elsewhere (svo_tree_descent.h)
template <class P>
__device__ __forceinline__ uint32_t comp_voxel(const P& T, int32_t x, int32_t y, int32_t z) {
    uint32_t id;
    return T.voxel(x, y, z, &id) ? id : old_voxel(T, (uint32_t)x, (uint32_t)y, (uint32_t)z);
}

struct Child {
    uint32_t what;
    uint32_t a;  // CH_SOLID: the material; CH_COPY: the old record's index; CH_NEXT: the next item's `old`
    uint32_t b;  // CH_NEXT: the next item's kind
};

template <class P>
__device__ Child child_of(const P& T, const Item& it, const Node& on, uint32_t sl, int32_t cs, int k) {
    const int32_t x = it.x0 + (int32_t)(sl & 3u) * cs, y = it.y0 + (int32_t)((sl >> 2) & 3u) * cs, z = it.z0 + (int32_t)(sl >> 4) * cs;
    uint32_t id;
    const uint32_t rel = T.relation(x, y, z, cs, k, &id);
    if (rel == SHAPE_IN) return id ? Child{CH_SOLID, id, 0u} : Child{CH_NONE, 0u, 0u};
    if constexpr (P::kFull)
        if (rel == SHAPE_FULL) return Child{CH_NEXT, 0u, P_EMPTY};
    // what the child held
    uint32_t okind = it.kind, old = it.old;
    uint64_t om = it.kind == P_UNIFORM ? ~0ull : 0ull;  // (k == 1) the voxels the old child stored
    if (it.kind == P_NODE) {
        okind = P_EMPTY;
        if ((on.mask >> sl) & 1ull) {
            old = on.ref + (uint32_t)__popcll(on.mask & ((1ull << sl) - 1ull));
            if (rel == SHAPE_OUT) return Child{CH_COPY, old, 0u};
            const Node oc = T.nodes[(uint64_t)old];
            okind = P_NODE;
            om = oc.mask;
            if (node_kind(oc.info) == K_SOLID) {
                okind = P_UNIFORM;
                old = node_material(oc.info);
                om = ~0ull;
            }
        }
    }
    if (rel == SHAPE_OUT) return okind == P_UNIFORM ? Child{CH_SOLID, old, 0u} : Child{CH_NONE, 0u, 0u};
    if (k == 1) {  // a cut brick: absent unless a composite voxel is stored (the patch's id, else what om says the tree held)
        bool any = false;
        for (uint32_t v = 0; v < 64u && !any; v++) {
            uint32_t vid;
            const bool hit = T.voxel(x + (int32_t)(v & 3u), y + (int32_t)((v >> 2) & 3u), z + (int32_t)(v >> 4), &vid);
            any = hit ? vid != 0u : (bool)((om >> v) & 1ull);
        }
        if (!any) return Child{CH_NONE, 0u, 0u};
    }
    return Child{CH_NEXT, old, okind};
}

template <class P>
__device__ __forceinline__ Item next_item(const P&, Item it, Child c, uint32_t sl, int32_t cs, uint32_t node) {
    return Item{it.x0 + (int32_t)(sl & 3u) * cs, it.y0 + (int32_t)((sl >> 2) & 3u) * cs, it.z0 + (int32_t)(sl >> 4) * cs, node, c.a, c.b};
}

template <class P>
__device__ __forceinline__ uint32_t brick_voxel(const P& T, const Item& it, uint32_t v) {
    return comp_voxel(T, it.x0 + (int32_t)(v & 3u), it.y0 + (int32_t)((v >> 2) & 3u), it.z0 + (int32_t)(v >> 4));
}

// ---- the kernels, over any patch

// one wavefront per item, lane = child slot: the children that exist and those that go on to the next level's list
template <class P>
__global__ void k_cells_count(P T, const typename P::Item* cur, int64_t r0, int64_t n, int32_t cs, int k, uint32_t* nkid, uint32_t* nnext) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together
    const typename P::Item it = cur[r];
    const Node on = old_record(T, it);
    const auto c = child_of(T, it, on, sl, cs, k);
    const uint64_t kid = __ballot(c.what != CH_NONE), nx = __ballot(c.what == CH_NEXT);
    if (sl == 0) {
        nkid[r] = (uint32_t)__popcll(kid);
        nnext[r] = (uint32_t)__popcll(nx);
    }
    superseded(T, it, on, c, sl);
}

// second pass: the item's INTERIOR record, its SOLID and copied children, the next level's items.  base: the scratch
// index of this level's first child record
template <class P>
__global__ void k_cells_write(P T, const typename P::Item* cur, int64_t r0, int64_t n, int32_t cs, int k, const uint64_t* koff,
                              const uint64_t* noff, uint64_t base, Node* out, typename P::Item* next) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const typename P::Item it = cur[r];
    const auto c = child_of(T, it, old_record(T, it), sl, cs, k);
    const uint64_t kid = __ballot(c.what != CH_NONE), nx = __ballot(c.what == CH_NEXT);
    const uint64_t below = (1ull << sl) - 1ull;
    const uint64_t kpos = base + koff[r] + (uint64_t)__popcll(kid & below);
    if (c.what == CH_NEXT) {
        next[noff[r] + (uint64_t)__popcll(nx & below)] = next_item(T, it, c, sl, cs, (uint32_t)kpos);
    } else if (c.what == CH_SOLID) {
        out[kpos] = Node{~0ull, 0u, K_SOLID | (c.a << 16)};
    } else if (c.what == CH_COPY) {
        out[kpos] = T.nodes[(uint64_t)c.a];
    }
    if (sl == 0) out[it.node] = Node{kid, (uint32_t)(T.nbase + base + koff[r] - 1ull), K_INTERIOR};
}

// bricks, by k_brick_count / k_brick_write's rules over the composite voxels (every item stores at least one)
template <class P>
__global__ void k_cells_brick_count(P T, const typename P::Item* cur, int64_t r0, int64_t n, uint32_t* nmat) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const uint32_t c = brick_voxel(T, cur[r], v);
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    if (v == 0) nmat[r] = uni ? 0u : (uint32_t)__popcll(solid);
}

// mbase: the tree's material index of mats[0]
template <class P>
__global__ void k_cells_brick_write(P T, const typename P::Item* cur, int64_t r0, int64_t n, const uint64_t* moff, uint64_t mbase, Node* out,
                                    uint16_t* mats) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const typename P::Item it = cur[r];
    const uint32_t c = brick_voxel(T, it, v);
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    const uint32_t first = (uint32_t)__shfl((int)c, (int)__builtin_ctzll(solid | (1ull << 63)));
    if (!uni && c != G_EMPTY) mats[moff[r] + (uint64_t)__popcll(solid & ((1ull << v) - 1ull))] = (uint16_t)c;
    if (v == 0) out[it.node] = uni ? Node{solid, 0u, K_BRICK | K_UNIFORM | (first << 16)} : Node{solid, (uint32_t)(mbase + moff[r]), K_BRICK};
}

// A finished descent in scratch (pool's): out[0] the anchor's new record, out[1 .. used) the node tail, mats[0 .. n_mats)
// the material tail
struct CellsTail {
    Node* out = nullptr;
    uint64_t used = 1;
    uint16_t* mats = nullptr;
    uint64_t n_mats = 0;
};

// the anchor as the cell-asking patches' first item
inline Item anchor_item(const PatchAnchor& a) { return Item{a.o[0], a.o[1], a.o[2], 0u, a.old, a.kind}; }

// The level loop, from the anchor down to the bricks of a tree L levels deep.  first: the anchor's item (node 0), at
// `depth`.  lone_root: the whole extent is one uniform region, and the root is this record without children (nothing
// descends).  mbase: the tree's material index of the tail's first entry.  tmp holds the scans' temporaries, which the
// caller frees after the device has finished.
template <class P>
int descend_cells(const P& T, const char* who, int32_t L, int32_t depth, const typename P::Item& first, const Node* lone_root, uint64_t mbase,
                  Pool& pool, std::vector<void*>& tmp, CellsTail* tail) {
    using Item = typename P::Item;
    // scratch records: [0] the anchor's, [1 ..) the appended tail; grown per level (capacity doubling, device copies)
    uint64_t cap = 1 << 12, used = 1, n_mats = 0;
    Node* out;
    int rc = pool.alloc(&out, cap);
    if (rc) return rc;
    auto reserve = [&](uint64_t need) -> int {
        if (need <= cap) return SVO_OK;
        uint64_t nc = cap;
        while (nc < need) nc *= 2;
        Node* nn;
        int r2 = pool.alloc(&nn, nc);
        if (r2) return r2;
        HIP_TRY(hipMemcpy(nn, out, used * sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
        pool.release(out);
        (void)hipFree(out);
        out = nn;
        cap = nc;
        return SVO_OK;
    };
    uint16_t* mats = nullptr;

    int64_t ncur = 1;
    if (lone_root) {
        HIP_TRY(hipMemcpy(out, lone_root, sizeof(Node), hipMemcpyHostToDevice), SVO_EDEVICE);
        ncur = 0;
    }
    Item* cur;
    rc = pool.alloc(&cur, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(cur, &first, sizeof(Item), hipMemcpyHostToDevice), SVO_EDEVICE);
    for (int d = depth; d < L && ncur > 0; d++) {
        const int32_t cs = 1 << (2 * (L - d - 1));
        if (d == L - 1) {
            uint32_t* nmat;
            uint64_t* moff;
            rc = pool.alloc(&nmat, ncur);
            if (!rc) rc = pool.alloc(&moff, ncur);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_cells_brick_count<P>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, nmat);
            });
            if (rc) return rc;
            rc = scan(nmat, moff, ncur, &n_mats, tmp);
            if (rc) return rc;
            if (mbase + n_mats > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 material entries");
            rc = pool.alloc(&mats, n_mats + 1);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_cells_brick_write<P>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, moff, mbase, out, mats);
            });
            if (rc) return rc;
            break;
        }
        uint32_t *nkid, *nnext;
        uint64_t *koff, *noff, nk = 0, nn = 0;
        rc = pool.alloc(&nkid, ncur);
        if (!rc) rc = pool.alloc(&nnext, ncur);
        if (!rc) rc = pool.alloc(&koff, ncur);
        if (!rc) rc = pool.alloc(&noff, ncur);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_cells_count<P>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, cs, L - d - 1, nkid, nnext);
        });
        if (rc) return rc;
        rc = scan(nkid, koff, ncur, &nk, tmp);
        if (!rc) rc = scan(nnext, noff, ncur, &nn, tmp);
        if (rc) return rc;
        if (T.nbase + used - 1 + nk > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 nodes");
        rc = reserve(used + nk);
        if (rc) return rc;
        Item* next;
        rc = pool.alloc(&next, nn);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_cells_write<P>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, cs, L - d - 1, koff, noff, used, out, next);
        });
        if (rc) return rc;
        used += nk;
        cur = next;
        ncur = (int64_t)nn;
    }
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    *tail = CellsTail{out, used, mats, n_mats};
    return SVO_OK;
}

// The finished descent put into the tree (svo_patch_commit.h), with what follows a commit: the garbage counts (gnodes /
// gmats superseded, counted by a host walk or by the patch's hook; a restart leaves none), the tree's top row, the ceilings over `rects` (room for them is reserved in
// svo_tree.ceil_dirty by the caller) and svo_tree_patch_times' three figures (clock0: after the entry synchronisation;
// clock1: after the descent).
inline int commit_cells(svo_tree* t, const char* who, const CellsTail& tail, const PatchAnchor& anchor, uint64_t nbase, uint64_t mbase,
                        uint64_t gnodes, uint64_t gmats, const std::vector<std::array<int64_t, 4>>& rects,
                        std::chrono::steady_clock::time_point clock0, std::chrono::steady_clock::time_point clock1) {
    // the totals are known and nothing of the tree has changed yet: room, then the tail, then the anchor's record
    int rc = commit_patch(t, who, PatchTail{tail.out, tail.used - 1, tail.mats, tail.n_mats, anchor.node, nbase, mbase, anchor.whole});
    if (rc) return rc;
    if (anchor.whole) {
        t->garbage_nodes = t->garbage_mats = 0;
    } else {
        t->garbage_nodes += gnodes;
        t->garbage_mats += gmats;
    }
    const auto clock2 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(t->top_mu);
        t->top_valid = false;
    }
    t->dev_top_y = tree_top_y(t);
    for (const auto& r : rects) t->ceil_dirty.push_back(r);
    rc = sync_ceilings(t);
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    t->patch_ms[0] = ms(clock0, clock1);
    t->patch_ms[1] = ms(clock1, clock2);
    t->patch_ms[2] = ms(clock2, std::chrono::steady_clock::now());
    return rc;
}

}  // namespace
