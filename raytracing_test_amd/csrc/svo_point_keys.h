// svo_point_keys.h — the first stage shared by the kernels that take a sparse list of voxels (x, y, z, id) in HBM
// (svo_build_points.hip: a tree from the list; svo_patch_points.hip: a resident tree patched from it): the key pass, which
// computes every point's 64-bit cell key (svo_points_source.h) and checks its id and coordinates, and the stable radix
// sort of (key, id) over the key's 6 * levels bits (hipCUB), after which the entries of a voxel lie next to each other in
// list order.  24 B of scratch per point: two key buffers, two id buffers, and the sort's temporaries.
#pragma once

#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_points_source.h"

namespace {

constexpr int32_t kBadId = 1, kBadCoord = 2;  // bits of the key pass's flag word

// keys and ids of points 0..n; a bad point gets key 0 (nothing is built from the keys then)
__global__ void k_point_keys(const int32_t* xyz, const uint16_t* ids, int64_t n, int32_t levels, uint32_t n_pal, uint64_t* keys,
                             uint16_t* vals, int32_t* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t E = 1u << (2 * levels);
    const uint32_t x = (uint32_t)xyz[3 * i], y = (uint32_t)xyz[3 * i + 1], z = (uint32_t)xyz[3 * i + 2];  // (negative: above E)
    const uint32_t id = ids[i];
    const int32_t b = (id >= n_pal ? kBadId : 0) | ((x >= E || y >= E || z >= E) ? kBadCoord : 0);
    if (b) atomicOr(bad, b);
    keys[i] = b ? 0ull : voxel_key(x, y, z, levels);
    vals[i] = (uint16_t)id;
}

inline dim3 lanes(int64_t n) { return dim3(blocks_for(n, 256)); }  // n < 2^31 lanes: fewer than 2^32 work-items

// the sorted list: n (key, id) pairs, and the sort's other key buffer (n entries, free for the caller's scans)
struct SortedPoints {
    const uint64_t* keys;
    const uint16_t* vals;
    uint64_t* spare;
};

// The keys of n > 0 points, sorted with their ids, in allocations of `pool`.  *bad: the key pass's flag word, read on the
// host before anything else is allocated; when it is set nothing is sorted and *S is not filled.
inline int sort_point_keys(const int32_t* xyz, const uint16_t* ids, int64_t n, int32_t levels, uint32_t n_pal, Pool& pool, SortedPoints* S,
                           int32_t* bad) {
    int32_t* dbad;
    uint64_t* k0;
    uint16_t* v0;
    int rc = pool.alloc(&dbad, 1);
    if (!rc) rc = pool.alloc(&k0, (size_t)n);
    if (!rc) rc = pool.alloc(&v0, (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemset(dbad, 0, 4), SVO_EDEVICE);
    hipLaunchKernelGGL(k_point_keys, lanes(n), dim3(256), 0, nullptr, xyz, ids, n, levels, n_pal, k0, v0, dbad);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(bad, dbad, 4, hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (*bad) return SVO_OK;

    // the stable sort, between two pairs of buffers
    uint64_t* k1;
    uint16_t* v1;
    rc = pool.alloc(&k1, (size_t)n);
    if (!rc) rc = pool.alloc(&v1, (size_t)n);
    if (rc) return rc;
    hipcub::DoubleBuffer<uint64_t> dk(k0, k1);
    hipcub::DoubleBuffer<uint16_t> dv(v0, v1);
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, dk, dv, n, 0, 6 * levels), SVO_EDEVICE);
    char* tmp;
    rc = pool.alloc(&tmp, tb);
    if (rc) return rc;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, dk, dv, n, 0, 6 * levels), SVO_EDEVICE);
    S->keys = dk.Current();
    S->vals = dv.Current();
    S->spare = dk.Alternate();
    return SVO_OK;
}

}  // namespace
