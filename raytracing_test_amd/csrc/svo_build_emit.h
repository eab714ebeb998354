// svo_build_emit.h — the level-synchronous breadth-first emitter of the on-device builders (svo_build.hip: terrain
// columns; svo_build_volume.hip: dense voxel volumes; svo_build_points.hip: sparse voxel lists; svo_compact.hip: a
// resident tree), generic over its source.  A source S is passed to the kernels
// by value and answers two questions on the device:
//   uint32_t S::classify(x0, y0, z0, s, k)   class of the aligned region [x0, x0+s)^3, s = 4^k, k >= 1:
//                                            G_EMPTY, a palette id (the whole region that material), or G_MIXED
//   uint32_t S::voxel(x, y, z)               the palette id stored at a voxel (G_EMPTY: none)
// One wavefront per region, one lane per child slot (or per voxel at the brick level): ballots give the child mask,
// the MIXED children and the stored voxels; exclusive scans over the regions (hipCUB) place every child block and
// material run; a second pass writes them.  The output is the host's canonical linearisation (svo_linearise.cpp
// svo_build_view) byte for byte, left in HBM (emit_arrays); the builders adopt it as a new tree's uploaded copy
// (emit_tree), the compaction swaps it in under a tree that keeps the rest of its residency.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_hip.h"
#include "svo_internal.h"

namespace {

using namespace svo;

constexpr uint32_t G_EMPTY = 0u;
constexpr uint32_t G_MIXED = 0xFFFFFFFFu;
constexpr int kMaxPyr = 8;

struct Region {
    int32_t x0, y0, z0;
    uint32_t node;  // index of the region's record in the node array
};

// one wavefront per region, lane = child slot: counts of non-empty and MIXED children
template <class S>
__global__ void k_count(S T, const Region* cur, int64_t r0, int64_t n, int32_t cs, int k, uint32_t* nkid, uint32_t* nmix) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together (n is per wave)
    const Region R = cur[r];
    const uint32_t c = T.classify(R.x0 + (int32_t)(sl & 3u) * cs, R.y0 + (int32_t)((sl >> 2) & 3u) * cs,
                                  R.z0 + (int32_t)(sl >> 4) * cs, cs, k);
    const uint64_t kid = __ballot(c != G_EMPTY), mix = __ballot(c == G_MIXED);
    if (sl == 0) {
        nkid[r] = (uint32_t)__popcll(kid);
        nmix[r] = (uint32_t)__popcll(mix);
    }
}

// second pass: the region's INTERIOR record, its SOLID children, the next level's MIXED regions
template <class S>
__global__ void k_write(S T, const Region* cur, int64_t r0, int64_t n, int32_t cs, int k, const uint64_t* koff, const uint64_t* moff,
                        uint64_t base, Node* nodes, Region* next) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Region R = cur[r];
    const int32_t x = R.x0 + (int32_t)(sl & 3u) * cs, y = R.y0 + (int32_t)((sl >> 2) & 3u) * cs, z = R.z0 + (int32_t)(sl >> 4) * cs;
    const uint32_t c = T.classify(x, y, z, cs, k);
    const uint64_t kid = __ballot(c != G_EMPTY), mix = __ballot(c == G_MIXED);
    const uint64_t below = (1ull << sl) - 1ull;
    const uint64_t kpos = base + koff[r] + (uint64_t)__popcll(kid & below);
    if (c == G_MIXED) {
        next[moff[r] + (uint64_t)__popcll(mix & below)] = Region{x, y, z, (uint32_t)kpos};
    } else if (c != G_EMPTY) {
        nodes[kpos] = Node{~0ull, 0u, K_SOLID | (c << 16)};
    }
    if (sl == 0) nodes[R.node] = Node{kid, (uint32_t)(base + koff[r]), K_INTERIOR};
}

// bricks: one wavefront per brick region, lane = voxel (z<<4 | y<<2 | x)
template <class S>
__device__ __forceinline__ uint32_t g_voxel(const S& T, const Region& R, uint32_t v) {
    return T.voxel(R.x0 + (int32_t)(v & 3u), R.y0 + (int32_t)((v >> 2) & 3u), R.z0 + (int32_t)(v >> 4));
}

__device__ __forceinline__ bool g_uniform(uint32_t c, uint64_t solid) {
    const uint32_t first = (uint32_t)__shfl((int)c, (int)__builtin_ctzll(solid | (1ull << 63)));
    return __ballot(c != G_EMPTY && c != first) == 0ull;
}

template <class S>
__global__ void k_brick_count(S T, const Region* cur, int64_t r0, int64_t n, uint32_t* nmat) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const uint32_t c = g_voxel(T, cur[r], v);
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    if (v == 0) nmat[r] = uni ? 0u : (uint32_t)__popcll(solid);
}

template <class S>
__global__ void k_brick_write(S T, const Region* cur, int64_t r0, int64_t n, const uint64_t* moff, Node* nodes, uint16_t* mats) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const Region R = cur[r];
    const uint32_t c = g_voxel(T, R, v);
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    const uint32_t first = (uint32_t)__shfl((int)c, (int)__builtin_ctzll(solid | (1ull << 63)));
    if (!uni && c != G_EMPTY) mats[moff[r] + (uint64_t)__popcll(solid & ((1ull << v) - 1ull))] = (uint16_t)c;
    if (v == 0) nodes[R.node] = uni ? Node{solid, 0u, K_BRICK | K_UNIFORM | (first << 16)} : Node{solid, (uint32_t)moff[r], K_BRICK};
}

// exclusive scan of n counts; returns the total
inline int scan(const uint32_t* in, uint64_t* out, int64_t n, uint64_t* total, std::vector<void*>& tmp_pool) {
    if (n == 0) {
        *total = 0;
        return SVO_OK;
    }
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n), SVO_EDEVICE);
    void* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, std::max<size_t>(tb, 16)), SVO_ENOMEM);
    tmp_pool.push_back(tmp);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)n), SVO_EDEVICE);
    uint64_t last = 0;
    uint32_t lastc = 0;
    HIP_TRY(hipMemcpy(&last, out + n - 1, 8, hipMemcpyDeviceToHost), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(&lastc, in + n - 1, 4, hipMemcpyDeviceToHost), SVO_EDEVICE);
    *total = last + lastc;
    return SVO_OK;
}

// the scans' temporaries of one call (`v` is scan's tmp_pool), freed on every exit of it
struct ScanTmp {
    std::vector<void*> v;
    ~ScanTmp() {
        for (void* x : v) (void)hipFree(x);
    }
};

// device allocations of one build, freed on every exit
struct Pool {
    std::vector<void*> p;
    ~Pool() {
        for (void* x : p)
            if (x) (void)hipFree(x);
    }
    template <class T>
    int alloc(T** out, size_t n) {
        void* x = nullptr;
        HIP_TRY(hipMalloc(&x, std::max<size_t>(n * sizeof(T), 16)), SVO_ENOMEM);
        p.push_back(x);
        *out = reinterpret_cast<T*>(x);
        return SVO_OK;
    }
    void release(void* x) {  // hand over ownership
        for (auto& y : p)
            if (y == x) y = nullptr;
    }
};

inline uint32_t blocks_for(int64_t threads, int bs) { return (uint32_t)((threads + bs - 1) / bs); }

// A dispatch holds fewer than 2^32 work-items (the HSA packet's grid size is 32-bit): the one-wave-per-
// region kernels run over chunks of at most 2^24 regions (2^30 work-items).
constexpr int64_t kRegionChunk = (int64_t)1 << 24;
template <class F>
int for_region_chunks(int64_t n, F&& launch) {
    for (int64_t r0 = 0; r0 < n; r0 += kRegionChunk) {
        const int64_t m = std::min(kRegionChunk, n - r0);
        launch(r0, dim3(blocks_for(m * 64, 256)));
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    return SVO_OK;
}

// What an emission leaves in HBM: the canonical arrays in allocations with slack for edits (the rule of svo_upload), still
// owned by the emitter's pool, and the statistics a tree carries
struct Emitted {
    Node* nodes = nullptr;
    uint16_t* mats = nullptr;
    uint64_t n_nodes = 0, node_cap = 0, n_mats = 0, mat_cap = 0;
    uint64_t nodes_per_level[8] = {0};
    uint64_t n_bricks = 0;
};

// Emit the tree of source T (`levels` deep) into new device arrays: *e.  Nothing but the pool is touched.
// root_class: the class of the whole extent — G_MIXED descends; G_EMPTY is the lone record {0, 0, K_INTERIOR}; a
// palette id is a lone K_SOLID root (svo_build_view's two roots without children).  `who` prefixes error messages.
template <class S>
int emit_arrays(const S& T, int32_t levels, uint32_t root_class, Pool& pool, const char* who, Emitted* e) {
    // node array: grown per level (capacity doubling, device copies)
    uint64_t cap = 1 << 16, used = 1;
    Node* nodes;
    int rc = pool.alloc(&nodes, cap);
    if (rc) return rc;
    auto reserve = [&](uint64_t need) -> int {
        if (need <= cap) return SVO_OK;
        uint64_t nc = cap;
        while (nc < need) nc *= 2;
        Node* nn;
        int r2 = pool.alloc(&nn, nc);
        if (r2) return r2;
        HIP_TRY(hipMemcpy(nn, nodes, used * sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
        pool.release(nodes);
        (void)hipFree(nodes);
        nodes = nn;
        cap = nc;
        return SVO_OK;
    };
    uint16_t* mats = nullptr;
    uint64_t n_mats = 0;
    std::vector<void*> tmp;

    Region root{0, 0, 0, 0};
    Region* cur;
    rc = pool.alloc(&cur, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(cur, &root, sizeof(Region), hipMemcpyHostToDevice), SVO_EDEVICE);
    int64_t ncur = 1;
    e->nodes_per_level[0] = 1;
    Node root_rec{0, 0, K_INTERIOR};
    if (root_class != G_MIXED) {  // a root without children: nothing to descend into
        if (root_class != G_EMPTY) root_rec = Node{~0ull, 0u, K_SOLID | (root_class << 16)};
        ncur = 0;
    }
    HIP_TRY(hipMemcpy(nodes, &root_rec, sizeof(Node), hipMemcpyHostToDevice), SVO_EDEVICE);
    for (int d = 0; d < levels && ncur > 0; d++) {
        const int32_t cs = 1 << (2 * (levels - d - 1));
        if (d == levels - 1) {
            uint32_t* nmat;
            uint64_t* moff;
            rc = pool.alloc(&nmat, ncur);
            if (!rc) rc = pool.alloc(&moff, ncur);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_brick_count<S>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, nmat);
            });
            if (rc) return rc;
            rc = scan(nmat, moff, ncur, &n_mats, tmp);
            if (rc) return rc;
            if (n_mats > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 material entries");
            rc = pool.alloc(&mats, n_mats + 1);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_brick_write<S>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, moff, nodes, mats);
            });
            if (rc) return rc;
            e->n_bricks = (uint64_t)ncur;
            break;
        }
        uint32_t *nkid, *nmix;
        uint64_t *koff, *moff, nk = 0, nm = 0;
        rc = pool.alloc(&nkid, ncur);
        if (!rc) rc = pool.alloc(&nmix, ncur);
        if (!rc) rc = pool.alloc(&koff, ncur);
        if (!rc) rc = pool.alloc(&moff, ncur);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_count<S>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, cs, levels - d - 1, nkid, nmix);
        });
        if (rc) return rc;
        rc = scan(nkid, koff, ncur, &nk, tmp);
        if (!rc) rc = scan(nmix, moff, ncur, &nm, tmp);
        if (rc) return rc;
        if (used + nk > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 nodes");
        rc = reserve(used + nk);
        if (rc) return rc;
        Region* next;
        rc = pool.alloc(&next, nm);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_write<S>, g, dim3(256), 0, nullptr, T, cur, r0, ncur, cs, levels - d - 1, koff, moff, used, nodes, next);
        });
        if (rc) return rc;
        e->nodes_per_level[d + 1] = nk;
        used += nk;
        cur = next;
        ncur = (int64_t)nm;
    }
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    for (void* x : tmp) (void)hipFree(x);
    // the arrays with slack for edits
    const uint64_t ncap = std::min<uint64_t>(used + used / 8 + 65536, 1ull << 32), mcap = std::min<uint64_t>(n_mats + n_mats / 8 + 65536, 1ull << 32);
    Node* dn;
    uint16_t* dm;
    rc = pool.alloc(&dn, ncap);
    if (!rc) rc = pool.alloc(&dm, mcap);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dn, nodes, used * sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    if (n_mats) HIP_TRY(hipMemcpy(dm, mats, n_mats * sizeof(uint16_t), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    e->nodes = dn;
    e->mats = dm;
    e->n_nodes = used;
    e->node_cap = ncap;
    e->n_mats = n_mats;
    e->mat_cap = mcap;
    return SVO_OK;
}

// Emit the tree of source T into t (levels, view and palette already set) and leave it uploaded to `device`: the host
// image is copied back and the arrays are adopted, which computes the rest of the residency (ceilings included) anew.
template <class S>
int emit_tree(const S& T, int32_t levels, uint32_t root_class, svo_tree* t, Pool& pool, int32_t device, const char* who) {
    Emitted e;
    int rc = emit_arrays(T, levels, root_class, pool, who, &e);
    if (rc) return rc;
    for (int i = 0; i < 8; i++) t->nodes_per_level[i] = e.nodes_per_level[i];
    t->n_bricks = e.n_bricks;
    t->nodes.reserve(e.node_cap);  // (the host image with the device arrays' slack: appended tails do not move it)
    t->mats.reserve(e.mat_cap);
    t->nodes.resize(e.n_nodes);
    t->mats.resize(e.n_mats);
    HIP_TRY(hipMemcpy(t->nodes.data(), e.nodes, e.n_nodes * sizeof(Node), hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (e.n_mats) HIP_TRY(hipMemcpy(t->mats.data(), e.mats, e.n_mats * sizeof(uint16_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    pool.release(e.nodes);
    pool.release(e.mats);
    rc = adopt_device(t, device, e.nodes, e.node_cap, e.mats, e.mat_cap);
    if (rc) {
        (void)hipFree(e.nodes);
        (void)hipFree(e.mats);
        return rc;
    }
    return SVO_OK;
}

}  // namespace
