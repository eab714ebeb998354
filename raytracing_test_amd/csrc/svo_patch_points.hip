// svo_patch_points.hip — svo_tree_patch_points_gpu: a resident tree is changed, on the device, by a sparse list of voxel
// edits (x, y, z, id) in HBM, applied in list order; a last entry of id 0 erases its voxel.  The cost follows the number of
// edits, never the extent's volume or the tree's size:
//   * keys and sort: svo_build_points_gpu's key pass (which checks ids and coordinates) and its stable radix sort of
//     (key, id) (svo_point_keys.h);
//   * edit list E: the last entry of every run of equal keys, whatever its id, with ids the tree's view does not hold
//     turned into 0, compacted to a sorted list of distinct keys;
//   * anchor: the deepest interior record of the host image whose region holds every edit (svo_plan.cpp points_anchor),
//     from the digits E's first and last key have in common: two 8-byte reads back;
//   * descent: svo_patch_cells.h's, shared with the other patches (its kernels, level loop and commit), with this file's
//     own item, child_of, next_item, brick_voxel and superseded hook.  An item is a region with what it held (svo_plan.h P_NODE / P_UNIFORM / P_EMPTY), its range
//     [e0, e1) of E and the place of its new record.  A child is touched when E holds a key under it (a binary search on
//     that level's digit inside the item's range).  An untouched child is the old record copied, a synthesised K_SOLID
//     below a uniform region, or nothing; a touched one goes on to the next level's list, and at the brick level it is
//     absent when ((om & ~em) | en) == 0 — om the old child's voxel mask, em the edited voxels, en the edits that store
//     something — so no K_BRICK record with mask 0 exists;
//   * bricks: k_brick_count / k_brick_write's rules, lane = voxel; the composite voxel is the edit where E has one, else
//     the old brick's, read from the old record directly;
//   * garbage is counted where the old records are read, in the count pass: the old child block of every P_NODE item, the
//     material run of every touched old non-uniform brick (atomics on two scratch words, read back after the descent);
//   * commit: commit_cells — everything is in scratch and the ids are checked before the tree is touched;
//   * ceilings: the distinct 16 x 16-column blocks E touches come back (8 B each), are merged into rectangles on the host
//     (svo_plan.cpp ceil_block_rects) and recomputed exactly by sync_ceilings.
// Scratch: 24 B per point for the sort, 4 + 8 B per point for the flags and offsets of the compaction, 10 B per edit for
// E, 16 B per edit for the column blocks and their sort, one item (20 B) and four scan words (24 B) per touched region and
// level — at most one region per edit per level — and the scratch records (16 B per appended node, capacity doubling).
// Nothing is sized by the extent or by the tree.  Every node and material index is widened to 64 bits before it addresses
// memory.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_args.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_patch_cells.h"
#include "svo_point_keys.h"

using namespace svo;

namespace {

// sorted entries: 1 for the last entry of a voxel, whatever its id
__global__ void k_edit_last(const uint64_t* keys, int64_t n, uint32_t* keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = (i + 1 == n || keys[i + 1] != keys[i]) ? 1u : 0u;
}

// the kept entries compacted into E; an id the tree's view does not hold becomes 0 (bit 0 of the table is clear)
__global__ void k_edit_compact(const uint64_t* keys, const uint16_t* vals, const uint32_t* keep, const uint64_t* off, int64_t n,
                               const uint32_t* in_view, uint64_t* ekeys, uint16_t* evals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint32_t id = vals[i];
    ekeys[off[i]] = keys[i];
    evals[off[i]] = ((in_view[id >> 5] >> (id & 31u)) & 1u) ? (uint16_t)id : (uint16_t)0;
}

// the 16 x 16-column block of every edit, as (bz << 32) | bx: x and z are the low and high 2 bits of every 6-bit digit
__global__ void k_edit_blocks(const uint64_t* ekeys, int64_t n, int32_t levels, uint64_t* blocks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = ekeys[i];
    uint64_t x = 0, z = 0;
    for (int d = 0; d < levels; d++) {
        const uint64_t dg = (key >> (6 * (levels - 1 - d))) & 63ull;
        x = (x << 2) | (dg & 3ull);
        z = (z << 2) | (dg >> 4);
    }
    blocks[i] = ((z >> (2 * kCeilK0)) << 32) | (x >> (2 * kCeilK0));
}

__global__ void k_block_heads(const uint64_t* blocks, int64_t n, uint32_t* head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || blocks[i - 1] != blocks[i]) ? 1u : 0u;
}

__global__ void k_block_compact(const uint64_t* blocks, const uint32_t* head, const uint64_t* off, int64_t n, uint64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    out[off[i]] = blocks[i];
}

// a region of one level's list: its record's place among the scratch records (0 is the anchor's), what it held (svo_plan.h
// P_*: `old` is a node index or a material), and its edits E[e0 .. e1) (n < 2^31)
struct EditItem {
    uint32_t node, old, kind, e0, e1;
};

// the patch as svo_patch_cells.h's kernels ask it
struct DevEdits {
    const uint64_t* ekeys;  // E: distinct keys, ascending
    const uint16_t* evals;  // their resolved ids (0: erase)
    const Node* nodes;      // the resident tree (read only: the patch is written to scratch)
    const uint16_t* mats;
    uint64_t nbase;         // scratch record s >= 1 becomes node nbase + s - 1 of the tree
    unsigned long long* garbage;  // [0] node records, [1] material entries superseded
    using Item = EditItem;
};

// the first entry of E[e0 .. e1) whose digit (key >> sh) & 63 is not below dg; the range shares every digit above
__device__ __forceinline__ uint32_t digit_lower(const uint64_t* ekeys, uint32_t e0, uint32_t e1, int sh, uint32_t dg) {
    uint32_t lo = e0, hi = e1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)((ekeys[mid] >> sh) & 63ull) < dg) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// what a child slot of an item becomes
struct EditChild {
    uint32_t what;
    uint32_t a;       // CH_SOLID: the material; CH_COPY: the old record's index; CH_NEXT: the next item's `old`
    uint32_t b;       // CH_NEXT: the next item's kind
    uint32_t e0, e1;  // CH_NEXT: the child's edits
    uint32_t gmats;   // material entries of a touched old non-uniform brick (superseded whatever the child becomes)
};

// slot sl of item `it`, whose children are 4^k voxels wide (k >= 1; k == 1: bricks); on = the old record of a P_NODE item
__device__ EditChild child_of(const DevEdits& P, const EditItem& it, const Node& on, uint32_t sl, int32_t, int k) {
    const uint32_t c0 = digit_lower(P.ekeys, it.e0, it.e1, 6 * k, sl), c1 = digit_lower(P.ekeys, c0, it.e1, 6 * k, sl + 1u);
    const bool touched = c1 > c0;
    // what the child held
    uint32_t okind = it.kind, old = it.old;
    uint64_t om = it.kind == P_UNIFORM ? ~0ull : 0ull;  // (k == 1) the old child's voxel mask
    uint32_t gmats = 0;
    if (it.kind == P_NODE) {
        okind = P_EMPTY;
        if ((on.mask >> sl) & 1ull) {
            old = on.ref + (uint32_t)__popcll(on.mask & ((1ull << sl) - 1ull));
            if (!touched) return EditChild{CH_COPY, old, 0u, 0u, 0u, 0u};
            const Node oc = P.nodes[(uint64_t)old];
            okind = P_NODE;
            om = oc.mask;
            if (node_kind(oc.info) == K_SOLID) {
                okind = P_UNIFORM;
                old = node_material(oc.info);
                om = ~0ull;
            } else if (node_kind(oc.info) == K_BRICK && !(oc.info & K_UNIFORM)) {
                gmats = (uint32_t)__popcll(oc.mask);
            }
        }
    }
    if (!touched) return okind == P_UNIFORM ? EditChild{CH_SOLID, old, 0u, 0u, 0u, 0u} : EditChild{CH_NONE, 0u, 0u, 0u, 0u, 0u};
    if (k == 1) {  // a touched brick: absent unless a composite voxel is stored (at most 64 entries of E)
        uint64_t em = 0, en = 0;
        for (uint32_t e = c0; e < c1; e++) {
            const uint64_t bit = 1ull << (P.ekeys[e] & 63ull);
            em |= bit;
            if (P.evals[e] != 0) en |= bit;
        }
        if (((om & ~em) | en) == 0ull) return EditChild{CH_NONE, 0u, 0u, 0u, 0u, gmats};
    }
    return EditChild{CH_NEXT, old, okind, c0, c1, gmats};
}

__device__ __forceinline__ EditItem next_item(const DevEdits&, EditItem, EditChild c, uint32_t, int32_t, uint32_t node) {
    return EditItem{node, c.a, c.b, c.e0, c.e1};
}

// the sum of v over the wavefront's 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}

// the records an item supersedes, counted where the old records are read (the count pass): its old child block, and the
// material runs of its touched old bricks
__device__ __forceinline__ void superseded(const DevEdits& P, const EditItem& it, const Node& on, const EditChild& c, uint32_t sl) {
    const uint32_t gm = wave_sum(c.gmats);
    if (sl == 0) {
        if (it.kind == P_NODE && on.mask) atomicAdd(P.garbage, (unsigned long long)__popcll(on.mask));
        if (gm) atomicAdd(P.garbage + 1, (unsigned long long)gm);
    }
}

// voxel v of a brick item: the edit when E has one, else what the brick held
__device__ uint32_t brick_voxel(const DevEdits& P, const EditItem& it, uint32_t v) {
    const uint32_t e = digit_lower(P.ekeys, it.e0, it.e1, 0, v);
    if (e < it.e1 && (uint32_t)(P.ekeys[e] & 63ull) == v) return P.evals[e];
    if (it.kind == P_UNIFORM) return it.old;
    if (it.kind != P_NODE) return G_EMPTY;
    const Node ob = P.nodes[(uint64_t)it.old];  // a K_BRICK record (a K_SOLID child came as P_UNIFORM)
    if (!((ob.mask >> v) & 1ull)) return G_EMPTY;
    return (ob.info & K_UNIFORM) ? node_material(ob.info) : P.mats[(uint64_t)ob.ref + (uint64_t)__popcll(ob.mask & ((1ull << v) - 1ull))];
}

}  // namespace

extern "C" int svo_tree_patch_points_gpu(svo_tree* t, const int32_t* xyz, const uint16_t* ids, int64_t n) {
    const char* who = "svo_tree_patch_points_gpu";
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_points_gpu: NULL tree");
    if (n < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_points_gpu: n must not be negative");
    if (n > 0 && (!xyz || !ids)) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_points_gpu: NULL xyz or ids");
    if (n > 0x7FFFFFFFll) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: n must be below 2^31");
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_points_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_points_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    const int32_t L = t->levels;
    if (L < 2 || t->nodes.empty()) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: trees of fewer than 2 levels are not patched");
    if (t->palette.empty() || t->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: the palette must hold 1..65535 entries");
    if (n == 0) return SVO_OK;

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // the list may come from any stream, and records and ceilings are rewritten in place below: every cast over the tree
    // must be over first (svo_tree_sync's contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    Pool pool;
    std::vector<svo_block> blocks;
    std::vector<Material> pal;
    try {
        for (const Material& m : t->palette) blocks.push_back(to_block(m));
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_points_gpu: out of memory");
    }
    const uint32_t* in_view = nullptr;
    bool all = false;
    int rc = view_table(blocks.data(), (uint32_t)blocks.size(), t->view, pool, pal, &in_view, all);
    if (rc) return rc;

    // keys, sort, and the edit list E
    SortedPoints S;
    int32_t bad = 0;
    rc = sort_point_keys(xyz, ids, n, L, (uint32_t)blocks.size(), pool, &S, &bad);
    if (rc) return rc;
    if (bad == (kBadId | kBadCoord))
        SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: an id is not below the tree's palette size, and a coordinate is outside [0, 4^levels)");
    if (bad & kBadId) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: an id is not below the tree's palette size");
    if (bad & kBadCoord) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_points_gpu: a coordinate is outside [0, 4^levels)");
    ScanTmp tmp;
    uint32_t* flag;
    rc = pool.alloc(&flag, (size_t)n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_edit_last, lanes(n), dim3(256), 0, nullptr, S.keys, n, flag);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    uint64_t ne = 0;
    rc = scan(flag, S.spare, n, &ne, tmp.v);
    if (rc) return rc;
    uint64_t* ekeys;
    uint16_t* evals;
    rc = pool.alloc(&ekeys, (size_t)ne);
    if (!rc) rc = pool.alloc(&evals, (size_t)ne);
    if (rc) return rc;
    hipLaunchKernelGGL(k_edit_compact, lanes(n), dim3(256), 0, nullptr, S.keys, S.vals, flag, S.spare, n, in_view, ekeys, evals);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);

    // the column blocks E touches: sorted, each once
    uint64_t *cb0, *cb1, nblk = 0;
    rc = pool.alloc(&cb0, (size_t)ne);
    if (!rc) rc = pool.alloc(&cb1, (size_t)ne);
    if (rc) return rc;
    hipLaunchKernelGGL(k_edit_blocks, lanes((int64_t)ne), dim3(256), 0, nullptr, ekeys, (int64_t)ne, L, cb0);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    {
        hipcub::DoubleBuffer<uint64_t> db(cb0, cb1);
        size_t tb = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, db, (int64_t)ne, 0, 48), SVO_EDEVICE);
        char* st;
        rc = pool.alloc(&st, tb);
        if (rc) return rc;
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(st, tb, db, (int64_t)ne, 0, 48), SVO_EDEVICE);
        const uint64_t* sorted = db.Current();
        uint64_t* uniq = db.Alternate();
        hipLaunchKernelGGL(k_block_heads, lanes((int64_t)ne), dim3(256), 0, nullptr, sorted, (int64_t)ne, flag);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        rc = scan(flag, S.spare, (int64_t)ne, &nblk, tmp.v);
        if (rc) return rc;
        hipLaunchKernelGGL(k_block_compact, lanes((int64_t)ne), dim3(256), 0, nullptr, sorted, flag, S.spare, (int64_t)ne, uniq);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        cb0 = uniq;
    }
    std::vector<uint64_t> hblocks;
    try {
        hblocks.resize((size_t)nblk);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_points_gpu: out of host memory");
    }
    HIP_TRY(hipMemcpy(hblocks.data(), cb0, (size_t)nblk * 8, hipMemcpyDeviceToHost), SVO_EDEVICE);

    // the anchor, from E's first and last key
    uint64_t kfirst = 0, klast = 0;
    HIP_TRY(hipMemcpy(&kfirst, ekeys, 8, hipMemcpyDeviceToHost), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(&klast, ekeys + (ne - 1), 8, hipMemcpyDeviceToHost), SVO_EDEVICE);
    const PatchAnchor anchor = points_anchor(t->nodes.data(), L, kfirst, klast);
    const uint64_t nbase = t->synced_nodes, mbase = t->synced_mats;
    unsigned long long* dgarb;
    rc = pool.alloc(&dgarb, 2);
    if (rc) return rc;
    HIP_TRY(hipMemset(dgarb, 0, 16), SVO_EDEVICE);
    const DevEdits P{ekeys, evals, reinterpret_cast<const Node*>(t->d_nodes), reinterpret_cast<const uint16_t*>(t->d_mats), nbase, dgarb};

    CellsTail tail;
    rc = descend_cells(P, who, L, anchor.depth, EditItem{0u, anchor.old, anchor.kind, 0u, (uint32_t)ne}, nullptr, mbase, pool, tmp.v, &tail);
    if (rc) return rc;
    unsigned long long garb[2] = {0, 0};
    HIP_TRY(hipMemcpy(garb, dgarb, 16, hipMemcpyDeviceToHost), SVO_EDEVICE);
    std::vector<std::array<int64_t, 4>> rects;
    try {
        rects = ceil_block_rects(hblocks);
        t->ceil_dirty.reserve(t->ceil_dirty.size() + rects.size());
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_points_gpu: out of host memory");
    }
    const auto clock1 = std::chrono::steady_clock::now();

    return commit_cells(t, who, tail, anchor, nbase, mbase, garb[0], garb[1], rects, clock0, clock1);
}
