// svo_diff_voxels.hip — svo_tree_diff_gpu: the voxels of a box in which two resident trees of equal levels store different
// ids, as (x, y, z, id_b) in HBM, in the point builder's key order: the edit list that svo_tree_patch_points_gpu applies to
// `a` to give it `b`'s content.  The listing (svo_list_voxels.hip) is the special case diff(empty, t); the phases are its
// four, over one list of *pairs* per depth.  An item is one aligned region: a side per tree (svo_diff_pair.h: a copy of the
// record a descent reads there, or the synthesised "uniform id u" below a K_SOLID ancestor or an unset slot) and the
// region's first voxel.
//   1. reach, top down: the root pair is (a.nodes[0], b.nodes[0]).  An item above brick depth looks at the child slots
//      set on either side (all 64 below a uniform non-empty side) whose cell meets the box: one wavefront per item, lane =
//      slot.  A slot whose two child states are both uniform is never materialised; the others (a ballot) land
//      contiguously, in slot order, in the next list, and the item's link holds their mask and the position of the first.
//      Every item so has a side that is a record with content of its own, reached by a descent of its tree: the lists hold
//      at most the records reached in a plus those reached in b, also when a solid root meets a sparse tree.
//   2. totals, bottom up, one u64 per item: at brick depth, lane v holds the two ids of voxel v and the total is
//      popcount(ballot(differ) & the box's 64-voxel mask); above, the wave sum over the slots of a materialised child's
//      total or, for a uniform/uniform slot whose ids differ, the clipped volume of its cell in closed form.  The root's
//      total is the count: count-only calls and capacity failures end here.
//   3. offsets, top down: the exclusive wave scan over the 64 slot totals, materialised and closed-form slots interleaved
//      in slot order, which is key order.  A materialised child receives its offset; a closed-form slot with voxels becomes
//      a uniform leaf (first voxel, id_b, offset, total), gathered per depth by a count per item and its scan.
//   4. write: brick-depth items by one wavefront each, lane = voxel: differing and inside the box, ranked by popcount,
//      id_b written; uniform leaves by one lane per output voxel, which finds its leaf by binary search over the scanned
//      totals and unranks its index (svo_list_unrank.h).
// A root pair of two uniform sides is settled on the host: nothing, or one uniform leaf.  No position is looked up from the
// root of either tree, both trees are only read, and everything runs on the caller's stream, which is waited for whenever
// the host needs a total.  Every node, material and output index is widened to 64 bits before it addresses memory, and
// every dispatch holds fewer than 2^32 work-items.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_diff_pair.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_list_unrank.h"
#include "svo_list_wave.h"
#include "svo_plan.h"

using namespace svo;

namespace {

struct DiffTrees {
    const Node *na, *nb;        // the two trees' records
    const uint16_t *ma, *mb;    // and material runs
};

struct alignas(16) DiffLink {   // an item's materialised children: their slots, and the position of the first in the next list
    uint64_t keep;
    uint32_t first, pad;
};

// the child slots of the pair at o that may hold a difference inside the box (cs: the edge of a child's cell)
__device__ __forceinline__ uint64_t diff_candidates(const Node& ia, const Node& ib, const ListOrg& o, int32_t cs, const ListBox& B) {
    return (diff_slot_mask(ia) | diff_slot_mask(ib)) & box_slots(o, cs, B);
}

__device__ __forceinline__ ListOrg child_org(const ListOrg& o, uint32_t sl, int32_t cs) {
    return ListOrg{o.x + (int32_t)(sl & 3u) * cs, o.y + (int32_t)((sl >> 2) & 3u) * cs, o.z + (int32_t)(sl >> 4) * cs, 0};
}

// what slot sl of an item above brick depth adds to the item's total, *v: 2, a materialised child's total (kid: the totals
// of the next list); 1, a uniform/uniform slot whose ids differ: the clipped volume of its cell at *co, which b fills with
// *idb; 0, nothing
__device__ __forceinline__ int slot_total(const DiffTrees& T, const Node& ia, const Node& ib, const ListOrg& o, const DiffLink& lk,
                                          const uint64_t* kid, uint32_t sl, int32_t cs, bool kid_brick, const ListBox& B, uint64_t* v,
                                          uint32_t* idb, ListOrg* co) {
    const uint64_t below = (1ull << sl) - 1ull;
    *v = 0;
    if ((lk.keep >> sl) & 1ull) {
        *v = kid[(uint64_t)lk.first + (uint64_t)__popcll(lk.keep & below)];
        return 2;
    }
    if (!((diff_candidates(ia, ib, o, cs, B) >> sl) & 1ull)) return 0;
    const Node ca = diff_child(ia, T.na, sl), cb = diff_child(ib, T.nb, sl);
    uint32_t ua, ub;
    (void)diff_both_uniform(ca, cb, kid_brick, &ua, &ub);  // (true: the slot was not kept)
    if (ua == ub) return 0;
    *co = child_org(o, sl, cs);
    *idb = ub;
    *v = list_clip_volume(co->x, co->y, co->z, cs, B);
    return *v ? 1 : 0;
}

// ---- 1. reach
// one wavefront per item above brick depth, lane = child slot: the slots to materialise (kid_brick: the children lie at
// brick depth)
__global__ void k_diff_count(DiffTrees T, const Node* sa, const Node* sb, const ListOrg* org, int64_t r0, int64_t n, int32_t cs, int kid_brick,
                             ListBox B, DiffLink* link, uint32_t* cnt) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together
    const Node ia = sa[r], ib = sb[r];
    bool keep = false;
    if ((diff_candidates(ia, ib, org[r], cs, B) >> sl) & 1ull) {
        const Node ca = diff_child(ia, T.na, sl), cb = diff_child(ib, T.nb, sl);
        uint32_t ua, ub;
        keep = !diff_both_uniform(ca, cb, kid_brick != 0, &ua, &ub);
    }
    const uint64_t m = __ballot(keep);
    if (sl == 0) {
        link[r] = DiffLink{m, 0u, 0u};
        cnt[r] = (uint32_t)__popcll(m);
    }
}

// the kept children's sides and origins written to the next list at off[r] .., in slot order, and the item linked to them
__global__ void k_diff_reach(DiffTrees T, const Node* sa, const Node* sb, const ListOrg* org, int64_t r0, int64_t n, int32_t cs,
                             const uint64_t* off, DiffLink* link, Node* nsa, Node* nsb, ListOrg* norg) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const uint64_t keep = link[r].keep;
    if ((keep >> sl) & 1ull) {
        const uint64_t at = off[r] + (uint64_t)__popcll(keep & ((1ull << sl) - 1ull));
        nsa[at] = diff_child(sa[r], T.na, sl);
        nsb[at] = diff_child(sb[r], T.nb, sl);
        norg[at] = child_org(org[r], sl, cs);
    }
    if (sl == 0) link[r].first = (uint32_t)off[r];  // (a list holds fewer than 2^31 items)
}

// ---- 2. totals
// one wavefront per item of a depth.  brick: the items lie at brick depth (lane = voxel); else lane = child slot, cs the
// edge of a child's cell and kid the totals of the next list.  lcnt: the item's closed-form slots that hold voxels
__global__ void k_diff_totals(DiffTrees T, const Node* sa, const Node* sb, const ListOrg* org, const DiffLink* link, const uint64_t* kid,
                              int64_t r0, int64_t n, int32_t cs, int brick, int kid_brick, ListBox B, uint64_t* tot, uint32_t* lcnt) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Node ia = sa[r], ib = sb[r];
    const ListOrg o = org[r];
    if (brick) {  // (the same in every lane)
        const uint64_t dm = __ballot(diff_voxel_id(ia, T.ma, sl) != diff_voxel_id(ib, T.mb, sl)) & box_slots(o, 1, B);
        if (sl == 0) {
            tot[r] = (uint64_t)__popcll(dm);
            lcnt[r] = 0u;
        }
        return;
    }
    uint64_t v;
    uint32_t idb = 0;
    ListOrg co = ListOrg{0, 0, 0, 0};
    const int cls = slot_total(T, ia, ib, o, link[r], kid, sl, cs, kid_brick != 0, B, &v, &idb, &co);
    const uint64_t leaves = __ballot(cls == 1);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) v += shfl_xor64(v, x);
    if (sl == 0) {
        tot[r] = v;
        lcnt[r] = (uint32_t)__popcll(leaves);
    }
}

// ---- 3. offsets
// one wavefront per item above brick depth, lane = child slot: off[r] plus the exclusive scan of the slot totals, handed to
// the materialised children (koff) and to the item's uniform leaves, which stand at lpos[r] .. among their depth's
__global__ void k_diff_offsets(DiffTrees T, const Node* sa, const Node* sb, const ListOrg* org, const DiffLink* link, const uint64_t* off,
                               const uint64_t* ktot, const uint64_t* lpos, int64_t r0, int64_t n, int32_t cs, int kid_brick, ListBox B,
                               uint64_t* koff, ListOrg* lorg, uint64_t* loff, uint32_t* lnum) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const DiffLink lk = link[r];
    uint64_t v;
    uint32_t idb = 0;
    ListOrg co = ListOrg{0, 0, 0, 0};
    const int cls = slot_total(T, sa[r], sb[r], org[r], lk, ktot, sl, cs, kid_brick != 0, B, &v, &idb, &co);
    const uint64_t leaves = __ballot(cls == 1), below = (1ull << sl) - 1ull;
    uint64_t inc = v;
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
        const uint64_t up = shfl_up64(inc, x);
        if (sl >= (uint32_t)x) inc += up;
    }
    const uint64_t at = off[r] + (inc - v);
    if (cls == 2) koff[(uint64_t)lk.first + (uint64_t)__popcll(lk.keep & below)] = at;
    if (cls == 1) {
        const uint64_t li = lpos[r] + (uint64_t)__popcll(leaves & below);
        lorg[li] = ListOrg{co.x, co.y, co.z, (int32_t)idb};
        loff[li] = at;
        lnum[li] = (uint32_t)v;  // (below 2^31: the whole count is)
    }
}

// ---- 4. write
// brick-depth items: one wavefront each, lane = voxel
__global__ void k_diff_bricks(DiffTrees T, const Node* sa, const Node* sb, const ListOrg* org, const uint64_t* off, int64_t r0, int64_t n,
                              ListBox B, int32_t* xyz, uint16_t* ids) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const ListOrg o = org[r];
    const uint32_t idb = diff_voxel_id(sb[r], T.mb, v);
    const uint64_t dm = __ballot(diff_voxel_id(sa[r], T.ma, v) != idb) & box_slots(o, 1, B);
    if (!((dm >> v) & 1ull)) return;
    const uint64_t at = off[r] + (uint64_t)__popcll(dm & ((1ull << v) - 1ull));
    xyz[3 * at] = o.x + (int32_t)(v & 3u);
    xyz[3 * at + 1] = o.y + (int32_t)((v >> 2) & 3u);
    xyz[3 * at + 2] = o.z + (int32_t)(v >> 4);
    ids[at] = (uint16_t)idb;
}

// one lane per voxel written from the uniform leaves of one depth: entry j of the concatenation of their clipped cells.
// lstart: the exclusive scan of the nleaf leaves' totals, S their sum; s: the edge of the leaves' cells; a leaf's id_b rides
// in its origin's fourth word
__global__ void k_diff_fill(const ListOrg* lorg, const uint64_t* loff, const uint64_t* lstart, int64_t nleaf, int64_t j0, int64_t S, int32_t s,
                            ListBox B, int32_t* xyz, uint16_t* ids) {
    const int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    int64_t a = 0, b = nleaf;  // the last leaf whose start is <= j
    while (b - a > 1) {
        const int64_t mid = a + ((b - a) >> 1);
        if (lstart[mid] <= (uint64_t)j) a = mid;
        else b = mid;
    }
    const uint64_t local = (uint64_t)j - lstart[a];
    const ListOrg o = lorg[a];
    int32_t p[3] = {o.x, o.y, o.z};
    list_unrank(p, s, B, local);
    const uint64_t at = loff[a] + local;
    xyz[3 * at] = p[0];
    xyz[3 * at + 1] = p[1];
    xyz[3 * at + 2] = p[2];
    ids[at] = (uint16_t)o.pad;
}

// the uniform leaves of one depth written out: their totals scanned, one lane per voxel
int fill_leaves(hipStream_t st, const ListOrg* lorg, const uint64_t* loff, const uint32_t* lnum, int64_t nleaf, int32_t s, const ListBox& B,
                uint64_t count, int32_t* xyz, uint16_t* ids, Pool& pool) {
    uint64_t* lstart;
    int rc = pool.alloc(&lstart, nleaf);
    if (rc) return rc;
    uint64_t S = 0;
    rc = scan_on(st, lnum, lstart, nleaf, &S, pool);
    if (rc) return rc;
    if (S > count) SVO_FAIL(SVO_EDEVICE, "svo_tree_diff_gpu: the leaves' totals exceed the count");  // (never: nothing is written past it)
    return for_lane_chunks((int64_t)S, [&](int64_t j0, dim3 g) {
        hipLaunchKernelGGL(k_diff_fill, g, dim3(256), 0, st, lorg, loff, lstart, nleaf, j0, (int64_t)S, s, B, xyz, ids);
    });
}

int check_count(const std::string& who, uint64_t count, const int32_t* xyz, int64_t cap, int64_t* n_out) {
    *n_out = (int64_t)count;
    if (!xyz) return SVO_OK;  // count only
    if (count > 0x7FFFFFFFull)
        SVO_FAIL(SVO_ERANGE, who + ": the trees differ in " + std::to_string(count) + " voxels of the box; a list must stay below 2^31");
    if (count > (uint64_t)cap)
        SVO_FAIL(SVO_ERANGE, who + ": the trees differ in " + std::to_string(count) + " voxels of the box, the buffers hold " + std::to_string(cap));
    return SVO_OK;
}

int diff_voxels(const svo_tree* a, const svo_tree* b, const ListBox& B, int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n_out,
                hipStream_t st) {
    const std::string who = "svo_tree_diff_gpu";
    const int32_t L = a->levels;
    const DiffTrees T{reinterpret_cast<const Node*>(a->d_nodes), reinterpret_cast<const Node*>(b->d_nodes),
                      reinterpret_cast<const uint16_t*>(a->d_mats), reinterpret_cast<const uint16_t*>(b->d_mats)};
    Pool pool;  // (released on return, after the stream has been waited for)

    // ---- the root pair
    Node root[2];
    HIP_TRY(hipMemcpyAsync(&root[0], T.na, sizeof(Node), hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipMemcpyAsync(&root[1], T.nb, sizeof(Node), hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    uint32_t ua, ub;
    if (diff_both_uniform(root[0], root[1], L == 1, &ua, &ub)) {  // two uniform sides: nothing, or one uniform leaf
        const int32_t E = 1 << (2 * L);
        const uint64_t count = ua != ub ? list_clip_volume(0, 0, 0, E, B) : 0ull;
        int rc = check_count(who, count, xyz, cap, n_out);
        if (rc || !xyz || count == 0) return rc;
        const ListOrg leaf = ListOrg{0, 0, 0, (int32_t)ub};  // (copied from before this block ends: the stream is waited for)
        const uint64_t zero = 0;
        const uint32_t num = (uint32_t)count;
        ListOrg* lorg;
        uint64_t* loff;
        uint32_t* lnum;
        rc = pool.alloc(&lorg, 1);
        if (!rc) rc = pool.alloc(&loff, 1);
        if (!rc) rc = pool.alloc(&lnum, 1);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(lorg, &leaf, sizeof(ListOrg), hipMemcpyHostToDevice, st), SVO_EDEVICE);
        HIP_TRY(hipMemcpyAsync(loff, &zero, 8, hipMemcpyHostToDevice, st), SVO_EDEVICE);
        HIP_TRY(hipMemcpyAsync(lnum, &num, 4, hipMemcpyHostToDevice, st), SVO_EDEVICE);
        HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
        rc = fill_leaves(st, lorg, loff, lnum, 1, E, B, count, xyz, ids, pool);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
        return SVO_OK;
    }

    // ---- 1. reach
    Node *sa[kMaxPyr] = {nullptr}, *sb[kMaxPyr] = {nullptr};
    ListOrg* org[kMaxPyr] = {nullptr};
    DiffLink* link[kMaxPyr] = {nullptr};
    uint32_t* cnt[kMaxPyr] = {nullptr};   // per item: children kept; later, its uniform leaves
    uint64_t* spos[kMaxPyr] = {nullptr};  // their exclusive scans
    int64_t nreach[kMaxPyr] = {0};
    int rc = pool.alloc(&sa[0], 1);
    if (!rc) rc = pool.alloc(&sb[0], 1);
    if (!rc) rc = pool.alloc(&org[0], 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sa[0], T.na, sizeof(Node), hipMemcpyDeviceToDevice, st), SVO_EDEVICE);
    HIP_TRY(hipMemcpyAsync(sb[0], T.nb, sizeof(Node), hipMemcpyDeviceToDevice, st), SVO_EDEVICE);
    HIP_TRY(hipMemsetAsync(org[0], 0, sizeof(ListOrg), st), SVO_EDEVICE);
    nreach[0] = 1;
    int deepest = 0;
    for (int d = 0; d <= L - 1; d++) {
        const int64_t n = nreach[d];
        rc = pool.alloc(&cnt[d], n);
        if (!rc) rc = pool.alloc(&spos[d], n);
        if (!rc) rc = pool.alloc(&link[d], n);
        if (rc) return rc;
        if (d == L - 1) break;  // brick depth: no children
        const int32_t cs = 1 << (2 * (L - 1 - d));
        const int kid_brick = d + 1 == L - 1;
        const Node *ca = sa[d], *cb = sb[d];
        const ListOrg* o = org[d];
        DiffLink* lk = link[d];
        uint32_t* c = cnt[d];
        uint64_t* off = spos[d];
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_diff_count, g, dim3(256), 0, st, T, ca, cb, o, r0, n, cs, kid_brick, B, lk, c);
        });
        if (rc) return rc;
        uint64_t total = 0;
        rc = scan_on(st, c, off, n, &total, pool);
        if (rc) return rc;
        if (total > a->synced_nodes + b->synced_nodes || total > (uint64_t)INT_MAX)
            SVO_FAIL(SVO_ESTATE, who + ": the trees' records do not form trees");
        if (total == 0) break;
        Node *na, *nb;
        ListOrg* norg;
        rc = pool.alloc(&na, total);
        if (!rc) rc = pool.alloc(&nb, total);
        if (!rc) rc = pool.alloc(&norg, total);
        if (rc) return rc;
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_diff_reach, g, dim3(256), 0, st, T, ca, cb, o, r0, n, cs, off, lk, na, nb, norg);
        });
        if (rc) return rc;
        sa[d + 1] = na;
        sb[d + 1] = nb;
        org[d + 1] = norg;
        nreach[d + 1] = (int64_t)total;
        deepest = d + 1;
    }

    // ---- 2. totals
    uint64_t* tot[kMaxPyr] = {nullptr};
    for (int d = deepest; d >= 0; d--) {
        rc = pool.alloc(&tot[d], nreach[d]);
        if (rc) return rc;
        const Node *ca = sa[d], *cb = sb[d];
        const ListOrg* o = org[d];
        const DiffLink* lk = link[d];
        const uint64_t* kid = d < deepest ? tot[d + 1] : nullptr;  // (the deepest list kept no child)
        uint64_t* out = tot[d];
        uint32_t* lc = cnt[d];
        const int64_t n = nreach[d];
        const int32_t cs = d < L - 1 ? 1 << (2 * (L - 1 - d)) : 1;
        const int brick = d == L - 1, kid_brick = d + 1 == L - 1;
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_diff_totals, g, dim3(256), 0, st, T, ca, cb, o, lk, kid, r0, n, cs, brick, kid_brick, B, out, lc);
        });
        if (rc) return rc;
    }
    uint64_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, tot[0], 8, hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    rc = check_count(who, count, xyz, cap, n_out);
    if (rc || !xyz || count == 0) return rc;

    // ---- 3. offsets, and the uniform leaves of every depth written as they are gathered
    uint64_t* off[kMaxPyr] = {nullptr};
    for (int d = 0; d <= deepest; d++) {
        rc = pool.alloc(&off[d], nreach[d]);
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(off[0], 0, 8, st), SVO_EDEVICE);
    for (int d = 0; d <= deepest && d < L - 1; d++) {
        const Node *ca = sa[d], *cb = sb[d];
        const ListOrg* o = org[d];
        const DiffLink* lk = link[d];
        const uint64_t *po = off[d], *kt = d < deepest ? tot[d + 1] : nullptr;
        uint64_t *ko = d < deepest ? off[d + 1] : nullptr, *lpos = spos[d];
        const int64_t n = nreach[d];
        const int32_t cs = 1 << (2 * (L - 1 - d));
        const int kid_brick = d + 1 == L - 1;
        uint64_t nleaf = 0;
        rc = scan_on(st, cnt[d], lpos, n, &nleaf, pool);
        if (rc) return rc;
        if (nleaf > count) SVO_FAIL(SVO_EDEVICE, who + ": the uniform leaves exceed the count");  // (never: each holds a voxel)
        ListOrg* lorg = nullptr;
        uint64_t* loff = nullptr;
        uint32_t* lnum = nullptr;
        if (nleaf) {
            rc = pool.alloc(&lorg, nleaf);
            if (!rc) rc = pool.alloc(&loff, nleaf);
            if (!rc) rc = pool.alloc(&lnum, nleaf);
            if (rc) return rc;
        }
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_diff_offsets, g, dim3(256), 0, st, T, ca, cb, o, lk, po, kt, lpos, r0, n, cs, kid_brick, B, ko, lorg, loff, lnum);
        });
        if (rc) return rc;
        if (nleaf) {
            rc = fill_leaves(st, lorg, loff, lnum, (int64_t)nleaf, cs, B, count, xyz, ids, pool);
            if (rc) return rc;
        }
    }

    // ---- 4. write: the brick-depth items
    if (deepest == L - 1) {
        const Node *ca = sa[deepest], *cb = sb[deepest];
        const ListOrg* o = org[deepest];
        const uint64_t* po = off[deepest];
        const int64_t n = nreach[deepest];
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) { hipLaunchKernelGGL(k_diff_bricks, g, dim3(256), 0, st, T, ca, cb, o, po, r0, n, B, xyz, ids); });
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_tree_diff_gpu(const svo_tree* a, const svo_tree* b, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                                 int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream) {
    if (!a || !b) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: a tree is NULL");
    if (!n) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: n is NULL");
    if (cap < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: cap must not be negative");
    if ((xyz == nullptr) != (ids == nullptr)) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: xyz and ids must both be given or both be NULL");
    if (!xyz && cap > 0) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: NULL xyz and ids with cap > 0");
    if (a->levels != b->levels)
        SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: the trees have " + std::to_string(a->levels) + " and " + std::to_string(b->levels) + " levels");
    if (a->levels < 1 || a->levels >= kMaxPyr) SVO_FAIL(SVO_ESTATE, "svo_tree_diff_gpu: not trees of 1..7 levels");
    ListBox B;
    const int bad = list_box(a->levels, origin, nx, ny, nz, &B);
    if (bad == LIST_BOX_DIM) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: the box's dimensions must be positive");
    if (bad) SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: the box leaves the extent (origin >= 0, origin + n <= 4^levels; no wrap)");
    if (a->device < 0 || !a->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_diff_gpu: tree a not uploaded (svo_upload)");
    if (b->device < 0 || !b->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_diff_gpu: tree b not uploaded (svo_upload)");
    if (a->device != b->device)
        SVO_FAIL(SVO_EINVAL, "svo_tree_diff_gpu: the trees live on devices " + std::to_string(a->device) + " and " + std::to_string(b->device));
    HIP_TRY(hipSetDevice(a->device), SVO_EDEVICE);
    return diff_voxels(a, b, B, xyz, ids, cap, n, (hipStream_t)hip_stream);
}
