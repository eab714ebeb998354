// svo_list_voxels.hip — svo_tree_list_voxels_gpu: the voxels a resident tree stores inside a box, as (x, y, z, id) in HBM,
// in the point builder's key order (svo_points_source.h voxel_key) — the inverse of svo_build_points_gpu.  Only the tree is
// read, and only where it meets the box: the cost follows the records reached and the voxels written, never the box's
// volume.  Four level-synchronous phases over one list of records per depth, in the shape of svo_compact.hip:
//   1. reach, top down: reach[d] holds a copy of every record of depth d that a descent from the root can read and whose
//      region meets the box, with the region's first voxel beside it.  An interior record contributes its children whose
//      slot is set and whose cell meets the box (a count per item, an exclusive scan, a write pass: one wavefront per
//      item, lane = child slot); they land contiguously, in slot order, in reach[d + 1], and the copy's mask and ref are
//      re-pointed at them: mask = the slots kept, ref = the position of the first.  K_SOLID records are leaves at whatever
//      depth they lie; bricks lie at depth levels - 1.
//   2. totals, bottom up: one u64 per item — a brick: popcount(mask & the box's 64-voxel mask); a K_SOLID region: the
//      product of its three clipped edge lengths, in closed form; an interior item: the wave sum of its children's
//      totals.  The root's total is the count: count-only calls and capacity failures end here.
//   3. offsets, top down: a child's output offset is its parent's plus the exclusive wave scan of its elder siblings'
//      totals.  Slot order at every depth is key order, so the list comes out sorted without a sort.
//   4. write: bricks, one wavefront per item, lane = voxel: stored and inside the box, ranked by popcount.  K_SOLID leaves:
//      those of a depth are gathered (a flag, a scan), their totals scanned, and one lane per output voxel finds its leaf
//      by binary search and unranks its index digit by digit: per level the 64 sub-cells' clipped counts are separable
//      (lz * ly * lx), so a digit takes at most 3 + 3 + 3 comparisons (svo_list_unrank.h, shared with the host).  O(levels)
//      per voxel written, spread by output index.
// No voxel of the box is looked up from the root.  Everything runs on the caller's stream, which is waited for whenever the
// host needs a total.  Every node, material and output index is widened to 64 bits before it addresses memory, and every
// dispatch holds fewer than 2^32 work-items.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <string>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_list_unrank.h"
#include "svo_list_wave.h"
#include "svo_plan.h"

using namespace svo;

namespace {

// ---- 1. reach
// one lane per item: the children an item contributes to the next list (cs: the edge of a child's cell)
__global__ void k_list_count(const Node* cur, const ListOrg* org, int64_t i0, int64_t n, int32_t cs, ListBox B, uint32_t* cnt) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Node it = cur[i];
    cnt[i] = node_kind(it.info) == K_INTERIOR ? (uint32_t)__popcll(it.mask & box_slots(org[i], cs, B)) : 0u;
}

// one wavefront per item, lane = child slot: the kept children's records and origins written to next[off[r] ..] in slot
// order, and the item re-pointed at them
__global__ void k_list_reach(const Node* nodes, Node* cur, const ListOrg* org, int64_t r0, int64_t n, int32_t cs, ListBox B,
                             const uint64_t* off, Node* next, ListOrg* norg) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together
    const Node it = cur[r];
    if (node_kind(it.info) != K_INTERIOR) return;
    const ListOrg o = org[r];
    const uint64_t keep = it.mask & box_slots(o, cs, B), below = (1ull << sl) - 1ull;
    if ((keep >> sl) & 1ull) {
        const uint64_t at = off[r] + (uint64_t)__popcll(keep & below);
        next[at] = nodes[(uint64_t)it.ref + (uint64_t)__popcll(it.mask & below)];
        norg[at] = ListOrg{o.x + (int32_t)(sl & 3u) * cs, o.y + (int32_t)((sl >> 2) & 3u) * cs, o.z + (int32_t)(sl >> 4) * cs, 0};
    }
    if (sl == 0) cur[r] = Node{keep, (uint32_t)off[r], it.info};  // (a list holds fewer than 2^32 items: they are distinct nodes of the tree)
}

// ---- 2. totals
// one wavefront per item of depth d, lane = child.  s: the edge of the items' regions; kid: the totals of reach[d + 1]
// (NULL at the deepest list, whose interior items kept no child and were not re-pointed)
__global__ void k_list_totals(const Node* cur, const ListOrg* org, const uint64_t* kid, int64_t r0, int64_t n, int32_t s, ListBox B,
                              uint64_t* tot) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Node it = cur[r];
    const uint32_t kind = node_kind(it.info);  // (the same in every lane)
    uint64_t v = 0;
    if (kind == K_SOLID) {
        const ListOrg o = org[r];
        v = list_clip_volume(o.x, o.y, o.z, s, B);
    } else if (kind == K_BRICK) {
        v = (uint64_t)__popcll(it.mask & box_slots(org[r], 1, B));
    } else if (kid) {
        if (sl < (uint32_t)__popcll(it.mask)) v = kid[(uint64_t)it.ref + sl];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += shfl_xor64(v, o);
    }
    if (sl == 0) tot[r] = v;
}

// ---- 3. offsets
// one wavefront per item of a depth above the deepest, lane = child: off[r] plus the exclusive scan of the children's totals
__global__ void k_list_offsets(const Node* cur, const uint64_t* off, const uint64_t* ktot, int64_t r0, int64_t n, uint64_t* koff) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Node it = cur[r];
    if (node_kind(it.info) != K_INTERIOR) return;
    const bool has = sl < (uint32_t)__popcll(it.mask);
    const uint64_t v = has ? ktot[(uint64_t)it.ref + sl] : 0ull;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = shfl_up64(inc, o);
        if (sl >= (uint32_t)o) inc += up;
    }
    if (has) koff[(uint64_t)it.ref + sl] = off[r] + (inc - v);
}

// ---- 4. write
// bricks: one wavefront per item, lane = voxel
__global__ void k_list_bricks(const Node* cur, const ListOrg* org, const uint64_t* off, const uint16_t* mats, int64_t r0, int64_t n,
                              ListBox B, int32_t* xyz, uint16_t* ids) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const Node it = cur[r];
    if (node_kind(it.info) != K_BRICK) return;
    const ListOrg o = org[r];
    const uint64_t out = it.mask & box_slots(o, 1, B), below = (1ull << v) - 1ull;
    if (!((out >> v) & 1ull)) return;
    const uint64_t at = off[r] + (uint64_t)__popcll(out & below);
    const uint32_t id = (it.info & K_UNIFORM) ? node_material(it.info) : (uint32_t)mats[(uint64_t)it.ref + (uint64_t)__popcll(it.mask & below)];
    xyz[3 * at] = o.x + (int32_t)(v & 3u);
    xyz[3 * at + 1] = o.y + (int32_t)((v >> 2) & 3u);
    xyz[3 * at + 2] = o.z + (int32_t)(v >> 4);
    ids[at] = (uint16_t)id;
}

// K_SOLID leaves of one depth: 1 for every item that is one and has voxels inside the box
__global__ void k_list_solid_flag(const Node* cur, const uint64_t* tot, int64_t i0, int64_t n, uint32_t* flag) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (node_kind(cur[i].info) == K_SOLID && tot[i] > 0ull) ? 1u : 0u;
}

// the flagged items gathered: their positions in the list and their totals (below 2^31: the whole count is)
__global__ void k_list_solid_pick(const uint64_t* tot, const uint32_t* flag, const uint64_t* pos, int64_t i0, int64_t n, uint32_t* sidx,
                                  uint32_t* scnt) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    sidx[pos[i]] = (uint32_t)i;
    scnt[pos[i]] = (uint32_t)tot[i];
}

// one lane per voxel written from the K_SOLID leaves of one depth: entry j of the concatenation of their clipped regions.
// sstart: the exclusive scan of the nsol leaves' totals, S their sum; s: the edge of the leaves' regions
__global__ void k_list_solids(const Node* cur, const ListOrg* org, const uint64_t* off, const uint32_t* sidx, const uint64_t* sstart,
                              int64_t nsol, int64_t j0, int64_t S, int32_t s, ListBox B, int32_t* xyz, uint16_t* ids) {
    const int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    int64_t a = 0, b = nsol;  // the last leaf whose start is <= j
    while (b - a > 1) {
        const int64_t mid = a + ((b - a) >> 1);
        if (sstart[mid] <= (uint64_t)j) a = mid;
        else b = mid;
    }
    const uint64_t r = sidx[a], local = (uint64_t)j - sstart[a];
    const ListOrg o = org[r];
    int32_t p[3] = {o.x, o.y, o.z};
    list_unrank(p, s, B, local);
    const uint64_t at = off[r] + local;
    xyz[3 * at] = p[0];
    xyz[3 * at + 1] = p[1];
    xyz[3 * at + 2] = p[2];
    ids[at] = (uint16_t)node_material(cur[r].info);
}

int list_voxels(const svo_tree* t, const ListBox& B, int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n_out, hipStream_t st) {
    const std::string who = "svo_tree_list_voxels_gpu";
    const int32_t L = t->levels;
    const Node* nodes = reinterpret_cast<const Node*>(t->d_nodes);
    const uint16_t* mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    Pool pool;  // (released on return, after the stream has been waited for)

    // ---- 1. reach
    Node* reach[kMaxPyr] = {nullptr};
    ListOrg* org[kMaxPyr] = {nullptr};
    uint32_t* cnt[kMaxPyr] = {nullptr};   // per item: children kept; later, the K_SOLID-leaf flag
    uint64_t* spos[kMaxPyr] = {nullptr};  // their exclusive scans
    int64_t nreach[kMaxPyr] = {0};
    int rc = pool.alloc(&reach[0], 1);
    if (!rc) rc = pool.alloc(&org[0], 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(reach[0], nodes, sizeof(Node), hipMemcpyDeviceToDevice, st), SVO_EDEVICE);
    HIP_TRY(hipMemsetAsync(org[0], 0, sizeof(ListOrg), st), SVO_EDEVICE);
    nreach[0] = 1;
    int deepest = 0;
    for (int d = 0; d <= L - 1; d++) {
        const int64_t n = nreach[d];
        rc = pool.alloc(&cnt[d], n);
        if (!rc) rc = pool.alloc(&spos[d], n);
        if (rc) return rc;
        if (d == L - 1) break;  // bricks and K_SOLID records: no children
        const int32_t cs = 1 << (2 * (L - 1 - d));
        Node* cur = reach[d];
        const ListOrg* o = org[d];
        uint32_t* c = cnt[d];
        uint64_t* off = spos[d];
        rc = for_lane_chunks(n, [&](int64_t i0, dim3 g) { hipLaunchKernelGGL(k_list_count, g, dim3(256), 0, st, cur, o, i0, n, cs, B, c); });
        if (rc) return rc;
        uint64_t total = 0;
        rc = scan_on(st, c, off, n, &total, pool);
        if (rc) return rc;
        if (total > t->synced_nodes || total > (uint64_t)INT_MAX) SVO_FAIL(SVO_ESTATE, who + ": the tree's records do not form a tree");
        if (total == 0) break;
        Node* next;
        ListOrg* norg;
        rc = pool.alloc(&next, total);
        if (!rc) rc = pool.alloc(&norg, total);
        if (rc) return rc;
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_list_reach, g, dim3(256), 0, st, nodes, cur, o, r0, n, cs, B, off, next, norg);
        });
        if (rc) return rc;
        reach[d + 1] = next;
        org[d + 1] = norg;
        nreach[d + 1] = (int64_t)total;
        deepest = d + 1;
    }

    // ---- 2. totals
    uint64_t* tot[kMaxPyr] = {nullptr};
    for (int d = deepest; d >= 0; d--) {
        rc = pool.alloc(&tot[d], nreach[d]);
        if (rc) return rc;
        const Node* cur = reach[d];
        const ListOrg* o = org[d];
        const uint64_t* kid = d < deepest ? tot[d + 1] : nullptr;
        uint64_t* out = tot[d];
        const int64_t n = nreach[d];
        const int32_t s = 1 << (2 * (L - d));
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) { hipLaunchKernelGGL(k_list_totals, g, dim3(256), 0, st, cur, o, kid, r0, n, s, B, out); });
        if (rc) return rc;
    }
    uint64_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, tot[0], 8, hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    *n_out = (int64_t)count;
    if (!xyz) return SVO_OK;  // count only
    if (count > 0x7FFFFFFFull) SVO_FAIL(SVO_ERANGE, who + ": the box holds " + std::to_string(count) + " voxels; a list must stay below 2^31");
    if (count > (uint64_t)cap) SVO_FAIL(SVO_ERANGE, who + ": the box holds " + std::to_string(count) + " voxels, the buffers " + std::to_string(cap));
    if (count == 0) return SVO_OK;

    // ---- 3. offsets
    uint64_t* off[kMaxPyr] = {nullptr};
    for (int d = 0; d <= deepest; d++) {
        rc = pool.alloc(&off[d], nreach[d]);
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(off[0], 0, 8, st), SVO_EDEVICE);
    for (int d = 0; d < deepest; d++) {
        const Node* cur = reach[d];
        const uint64_t *po = off[d], *kt = tot[d + 1];
        uint64_t* ko = off[d + 1];
        const int64_t n = nreach[d];
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) { hipLaunchKernelGGL(k_list_offsets, g, dim3(256), 0, st, cur, po, kt, r0, n, ko); });
        if (rc) return rc;
    }

    // ---- 4. write
    if (deepest == L - 1) {
        const Node* cur = reach[deepest];
        const ListOrg* o = org[deepest];
        const uint64_t* po = off[deepest];
        const int64_t n = nreach[deepest];
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) { hipLaunchKernelGGL(k_list_bricks, g, dim3(256), 0, st, cur, o, po, mats, r0, n, B, xyz, ids); });
        if (rc) return rc;
    }
    for (int d = 0; d <= deepest; d++) {
        const Node* cur = reach[d];
        const ListOrg* o = org[d];
        const uint64_t *po = off[d], *tt = tot[d];
        uint32_t* flag = cnt[d];
        uint64_t* pos = spos[d];
        const int64_t n = nreach[d];
        rc = for_lane_chunks(n, [&](int64_t i0, dim3 g) { hipLaunchKernelGGL(k_list_solid_flag, g, dim3(256), 0, st, cur, tt, i0, n, flag); });
        if (rc) return rc;
        uint64_t nsol = 0, S = 0;
        rc = scan_on(st, flag, pos, n, &nsol, pool);
        if (rc) return rc;
        if (nsol == 0) continue;
        uint32_t *sidx, *scnt;
        uint64_t* sstart;
        rc = pool.alloc(&sidx, nsol);
        if (!rc) rc = pool.alloc(&scnt, nsol);
        if (!rc) rc = pool.alloc(&sstart, nsol);
        if (rc) return rc;
        rc = for_lane_chunks(n, [&](int64_t i0, dim3 g) { hipLaunchKernelGGL(k_list_solid_pick, g, dim3(256), 0, st, tt, flag, pos, i0, n, sidx, scnt); });
        if (rc) return rc;
        rc = scan_on(st, scnt, sstart, (int64_t)nsol, &S, pool);
        if (rc) return rc;
        if (S > count) SVO_FAIL(SVO_EDEVICE, who + ": the leaves' totals exceed the count");  // (never: nothing is written past it)
        const int32_t s = 1 << (2 * (L - d));
        rc = for_lane_chunks((int64_t)S, [&](int64_t j0, dim3 g) {
            hipLaunchKernelGGL(k_list_solids, g, dim3(256), 0, st, cur, o, po, sidx, sstart, (int64_t)nsol, j0, (int64_t)S, s, B, xyz, ids);
        });
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_tree_list_voxels_gpu(const svo_tree* t, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz, int32_t* xyz,
                                        uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: tree is NULL");
    if (!n) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: n is NULL");
    if (cap < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: cap must not be negative");
    if ((xyz == nullptr) != (ids == nullptr)) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: xyz and ids must both be given or both be NULL");
    if (!xyz && cap > 0) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: NULL xyz and ids with cap > 0");
    if (t->levels < 1 || t->levels >= kMaxPyr) SVO_FAIL(SVO_ESTATE, "svo_tree_list_voxels_gpu: not a tree of 1..7 levels");
    ListBox B;
    const int bad = list_box(t->levels, origin, nx, ny, nz, &B);
    if (bad == LIST_BOX_DIM) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: the box's dimensions must be positive");
    if (bad) SVO_FAIL(SVO_EINVAL, "svo_tree_list_voxels_gpu: the box leaves the extent (origin >= 0, origin + n <= 4^levels; no wrap)");
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_list_voxels_gpu: tree not uploaded (svo_upload)");
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    return list_voxels(t, B, xyz, ids, cap, n, (hipStream_t)hip_stream);
}
