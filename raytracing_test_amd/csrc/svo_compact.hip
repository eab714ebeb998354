// svo_compact.hip — svo_tree_compact_gpu: a resident tree re-emitted, on its device, as the canonical linearisation of its
// own content.  Edits (svo_tree_update, svo_tree_patch_volume_gpu) append records and leave the superseded ones, and the
// regions they made uniform or empty, in place; the compaction reads only the tree — its cost follows the tree's size,
// not the extent's volume — and leaves what svo_build_volume_gpu would emit for the same content, byte for byte.
// Three level-synchronous phases, one list of records per depth:
//   1. reach, top down: reach[d] holds a copy of every record of depth d that a descent from the root can read.  An
//      interior record contributes popcount(mask) children (a count per item, an exclusive scan, a write pass: one
//      wavefront per item, lane = child slot); the children of item i land contiguously, in slot order, at the scanned
//      offset of reach[d + 1], and the copy's `ref` is re-pointed there.  The lists are the reachable tree, linearised per
//      depth: they double as the parent -> child map of the other two phases, and no table by old node index exists.
//   2. classes, bottom up: one 16-bit class word per item (svo_volume_pyramid.h: C_EMPTY, an id, C_MIXED = 0xFFFF, which
//      no id equals: ids end at 65534).  K_SOLID: its id.  A brick: mask 0 is EMPTY; a full mask of one material
//      (K_UNIFORM, or 64 equal entries of its run) is that id; every other brick is MIXED.  An interior record: the fold
//      of its 64 slots (absent: EMPTY) by the pyramid's fold2, one wavefront per item, lane = slot (voxel for a brick).
//   3. emit, top down: svo_build_emit.h with the resident tree as its third source (after the terrain and the dense
//      volume): classify() descends the lists to the region and answers with its class word, voxel() reads the old brick
//      by svo_tree_get_block's descent (svo_tree_descent.h).  The record-forming rules stay the emitter's own.
// Everything is emitted beside the old arrays, which are read only; the new arrays (emit_arrays' slack rule) and the host
// image replace the old ones at the very end, so a failure leaves the tree untouched on host and device.  The content is
// unchanged, hence the ceilings, the pick buffer, the palette upload, the AO plan and the frame schedules are kept.
// Every node and material index is widened to 64 bits before it addresses memory, and every dispatch holds fewer than
// 2^32 work-items: trees above 2^28 nodes take the same kernels.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_plan.h"
#include "svo_tree_descent.h"
#include "svo_volume_pyramid.h"

using namespace svo;

namespace {

// the emitter's source over a resident tree
struct DevTree {
    const Node* nodes;  // the resident arrays (read only)
    const uint16_t* mats;
    int32_t levels;
    const Node* reach[kMaxPyr];    // depth d: the reachable records; an interior's ref = position of its first child in reach[d + 1]
    const uint16_t* cls[kMaxPyr];  // depth d: the class word of every item of reach[d]

    // the region of depth levels - k (k >= 1) at (x0, y0, z0): found through the lists
    __device__ uint32_t classify(int32_t x0, int32_t y0, int32_t z0, int32_t, int k) const {
        const int D = levels - k;
        uint64_t pos = 0;
        for (int d = 0; d < D; d++) {
            const Node n = reach[d][pos];
            const uint32_t kind = node_kind(n.info);
            if (kind == K_SOLID) return node_material(n.info);
            if (kind != K_INTERIOR) return G_EMPTY;  // (never: bricks lie at depth levels - 1 only)
            const uint32_t sh = (uint32_t)(2 * (levels - 1 - d));
            const uint32_t sl = ((((uint32_t)z0 >> sh) & 3u) << 4) | ((((uint32_t)y0 >> sh) & 3u) << 2) | (((uint32_t)x0 >> sh) & 3u);
            if (!((n.mask >> sl) & 1ull)) return G_EMPTY;
            pos = (uint64_t)n.ref + (uint64_t)__popcll(n.mask & ((1ull << sl) - 1ull));
        }
        const uint32_t c = cls[D][pos];
        return c == C_MIXED ? G_MIXED : c;
    }
    __device__ __forceinline__ uint32_t voxel(int32_t x, int32_t y, int32_t z) const {
        return old_voxel(*this, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    }
};

// ---- 1. reach
// one lane per item: the children an item contributes to the next list
__global__ void k_reach_count(const Node* cur, int64_t i0, int64_t n, uint32_t* cnt) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Node it = cur[i];
    cnt[i] = node_kind(it.info) == K_INTERIOR ? (uint32_t)__popcll(it.mask) : 0u;
}

// one wavefront per item, lane = child slot: the children's records copied to next[off[r] ..] in slot order, and the
// item's ref re-pointed at them
__global__ void k_reach_write(const Node* nodes, Node* cur, int64_t r0, int64_t n, const uint64_t* off, Node* next) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together
    const Node it = cur[r];
    if (node_kind(it.info) != K_INTERIOR) return;
    const uint64_t rank = (uint64_t)__popcll(it.mask & ((1ull << sl) - 1ull));
    if ((it.mask >> sl) & 1ull) next[off[r] + rank] = nodes[(uint64_t)it.ref + rank];
    if (sl == 0) cur[r].ref = (uint32_t)off[r];  // (a list holds fewer than 2^32 items: they are distinct nodes of the tree)
}

// ---- 2. classes
// the fold of a wavefront's 64 class words, in every lane (the fold is commutative and idempotent)
__device__ __forceinline__ uint32_t fold_wave(uint32_t c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c = fold2(c, (uint32_t)__shfl_xor((int)c, o));
    return c;
}

// one wavefront per item of depth d, lane = child slot (voxel for a brick).  kid: the class words of reach[d + 1]
// (NULL at the deepest list, whose items have no children)
__global__ void k_classes(const Node* cur, const uint16_t* mats, const uint16_t* kid, int64_t r0, int64_t n, uint16_t* cls) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Node it = cur[r];
    const uint32_t kind = node_kind(it.info);
    const uint64_t rank = (uint64_t)__popcll(it.mask & ((1ull << sl) - 1ull));
    const bool has = (it.mask >> sl) & 1ull;
    uint32_t c = C_EMPTY;
    if (kind == K_SOLID) {
        c = node_material(it.info);
    } else if (kind == K_BRICK) {
        if (it.mask == 0ull) c = C_EMPTY;
        else if (it.mask != ~0ull) c = C_MIXED;
        else if (it.info & K_UNIFORM) c = node_material(it.info);
        else c = fold_wave(mats[(uint64_t)it.ref + rank]);
    } else if (kid) {
        c = fold_wave(has ? (uint32_t)kid[(uint64_t)it.ref + rank] : C_EMPTY);
    }
    if (sl == 0) cls[r] = (uint16_t)c;
}

constexpr int64_t kItemChunk = (int64_t)1 << 30;  // one-lane-per-item dispatches

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// the three phases and the swap, once the arguments are checked and the device is idle; *done: the clock after the swap
// (the scratch allocations and the old host image are released on return)
int compact(svo_tree* t, std::chrono::steady_clock::time_point clock0, std::chrono::steady_clock::time_point* done) {
    const char* who = "svo_tree_compact_gpu";
    const int32_t L = t->levels;
    Pool pool;
    ScanTmp tmp;
    DevTree T;
    memset(&T, 0, sizeof(T));
    T.nodes = reinterpret_cast<const Node*>(t->d_nodes);
    T.mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    T.levels = L;

    // ---- 1. reach
    Node* reach[kMaxPyr] = {nullptr};
    int64_t nreach[kMaxPyr] = {0};
    int rc = pool.alloc(&reach[0], 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(reach[0], T.nodes, sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    nreach[0] = 1;
    int deepest = 0;
    for (int d = 0; d < L - 1 && nreach[d] > 0; d++) {
        const int64_t n = nreach[d];
        uint32_t* cnt;
        uint64_t *off, total = 0;
        rc = pool.alloc(&cnt, n);
        if (!rc) rc = pool.alloc(&off, n);
        if (rc) return rc;
        Node* cur = reach[d];
        for (int64_t i0 = 0; i0 < n; i0 += kItemChunk) {
            hipLaunchKernelGGL(k_reach_count, dim3(blocks_for(std::min(kItemChunk, n - i0), 256)), dim3(256), 0, nullptr, cur, i0, n, cnt);
            HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        }
        rc = scan(cnt, off, n, &total, tmp.v);
        if (rc) return rc;
        if (total > t->synced_nodes) SVO_FAIL(SVO_ESTATE, std::string(who) + ": the tree's records do not form a tree");
        if (total == 0) break;
        Node* next;
        rc = pool.alloc(&next, total);
        if (rc) return rc;
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_reach_write, g, dim3(256), 0, nullptr, T.nodes, cur, r0, n, off, next);
        });
        if (rc) return rc;
        reach[d + 1] = next;
        nreach[d + 1] = (int64_t)total;
        deepest = d + 1;
    }

    // ---- 2. classes
    uint16_t* cls[kMaxPyr] = {nullptr};
    for (int d = deepest; d >= 0; d--) {
        rc = pool.alloc(&cls[d], nreach[d]);
        if (rc) return rc;
        const Node* cur = reach[d];
        const uint16_t* kid = d < deepest ? cls[d + 1] : nullptr;
        uint16_t* out = cls[d];
        const int64_t n = nreach[d];
        rc = for_region_chunks(n, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_classes, g, dim3(256), 0, nullptr, cur, T.mats, kid, r0, n, out);
        });
        if (rc) return rc;
    }
    for (int d = 0; d <= deepest; d++) {
        T.reach[d] = reach[d];
        T.cls[d] = cls[d];
    }
    uint16_t top = 0;
    HIP_TRY(hipMemcpy(&top, cls[0], 2, hipMemcpyDeviceToHost), SVO_EDEVICE);

    // ---- 3. emit
    Emitted e;
    rc = emit_arrays(T, L, top == C_MIXED ? G_MIXED : (uint32_t)top, pool, who, &e);
    if (rc) return rc;
    const auto clock1 = std::chrono::steady_clock::now();

    // the host image of the new arrays, then the swap: nothing of the tree has changed before it
    std::vector<Node> hn;
    std::vector<uint16_t> hm;
    try {
        hn.reserve(e.node_cap);  // (with the device arrays' slack: appended tails do not move it)
        hm.reserve(e.mat_cap);
        hn.resize(e.n_nodes);
        hm.resize(e.n_mats);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_compact_gpu: out of host memory");
    }
    HIP_TRY(hipMemcpy(hn.data(), e.nodes, e.n_nodes * sizeof(Node), hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (e.n_mats) HIP_TRY(hipMemcpy(hm.data(), e.mats, e.n_mats * sizeof(uint16_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    pool.release(e.nodes);
    pool.release(e.mats);
    (void)hipFree(t->d_nodes);
    (void)hipFree(t->d_mats);
    t->d_nodes = e.nodes;
    t->d_mats = e.mats;
    t->device_bytes += e.node_cap * sizeof(Node) + e.mat_cap * sizeof(uint16_t);
    t->device_bytes -= t->dev_node_cap * sizeof(Node) + t->dev_mat_cap * sizeof(uint16_t);
    t->dev_node_cap = e.node_cap;
    t->dev_mat_cap = e.mat_cap;
    t->nodes.swap(hn);
    t->mats.swap(hm);
    t->synced_nodes = e.n_nodes;
    t->synced_mats = e.n_mats;
    for (int i = 0; i < 8; i++) t->nodes_per_level[i] = e.nodes_per_level[i];
    t->n_bricks = e.n_bricks;
    t->garbage_nodes = t->garbage_mats = 0;
    *done = std::chrono::steady_clock::now();
    t->compact_ms[0] = ms_between(clock0, clock1);
    t->compact_ms[1] = ms_between(clock1, *done);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_tree_compact_gpu(svo_tree* t) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_compact_gpu: NULL tree");
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_compact_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_compact_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    if (t->levels < 1 || t->levels >= kMaxPyr || t->nodes.empty()) SVO_FAIL(SVO_ESTATE, "svo_tree_compact_gpu: not a tree of 1..7 levels");

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // the arrays are replaced below: every cast over the tree must be over first (svo_tree_sync's contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    auto done = std::chrono::steady_clock::now();
    const int rc = compact(t, done, &done);
    if (!rc) t->compact_ms[2] = ms_between(done, std::chrono::steady_clock::now());
    return rc;
}

extern "C" int svo_tree_compact_times(const svo_tree* t, double ms[3]) {
    if (!t || !ms) SVO_FAIL(SVO_EINVAL, "svo_tree_compact_times: NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = t->compact_ms[i];
    return SVO_OK;
}
