// svo_list_wave.h — what the level-synchronous listings over a resident tree share on the device side (svo_list_voxels.hip,
// svo_diff_voxels.hip): a region's first voxel, the 64-slot mask of a region's cells that meet the box, 64-bit wave
// shuffles, the stream-ordered exclusive scan and the chunked one-lane-per-item dispatch.  Everything stands in an
// unnamed namespace: each translation unit holds its own copy, as it did when these lived in svo_list_voxels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>
#include <algorithm>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_list_unrank.h"

namespace {

using namespace svo;

struct alignas(16) ListOrg {  // a region's first voxel (one 16-B load)
    int32_t x, y, z, pad;
};

// the cells i = 0..3, [o + i * cs, o + (i + 1) * cs), that meet [lo, hi): a 4-bit mask
__device__ __forceinline__ uint64_t axis_cells(int32_t o, int32_t cs, int32_t lo, int32_t hi) {
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int32_t a = o + i * cs;
        if (a < hi && a + cs > lo) m |= 1ull << i;
    }
    return m;
}

// the slots (z<<4 | y<<2 | x) of the region at o whose cell of edge cs meets the box (cs = 1: a brick's voxels inside it)
__device__ __forceinline__ uint64_t box_slots(const ListOrg& o, int32_t cs, const ListBox& B) {
    const uint64_t mx = axis_cells(o.x, cs, B.lo[0], B.hi[0]), my = axis_cells(o.y, cs, B.lo[1], B.hi[1]),
                   mz = axis_cells(o.z, cs, B.lo[2], B.hi[2]);
    uint64_t plane = 0, all = 0;
#pragma unroll
    for (int y = 0; y < 4; y++)
        if ((my >> y) & 1ull) plane |= mx << (4 * y);
#pragma unroll
    for (int z = 0; z < 4; z++)
        if ((mz >> z) & 1ull) all |= plane << (16 * z);
    return all;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o);
    return ((uint64_t)hi << 32) | lo;
}

constexpr int64_t kLaneChunk = (int64_t)1 << 30;  // one-lane-per-item dispatches

// exclusive scan of n counts on a stream; the total comes back once the stream has passed it
int scan_on(hipStream_t st, const uint32_t* in, uint64_t* out, int64_t n, uint64_t* total, Pool& pool) {
    *total = 0;
    if (n == 0) return SVO_OK;
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, st), SVO_EDEVICE);
    char* tmp;
    int rc = pool.alloc(&tmp, tb);
    if (rc) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)n, st), SVO_EDEVICE);
    uint64_t last = 0;
    uint32_t lastc = 0;
    HIP_TRY(hipMemcpyAsync(&last, out + n - 1, 8, hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipMemcpyAsync(&lastc, in + n - 1, 4, hipMemcpyDeviceToHost, st), SVO_EDEVICE);
    HIP_TRY(hipStreamSynchronize(st), SVO_EDEVICE);
    *total = last + lastc;
    return SVO_OK;
}

template <class F>
int for_lane_chunks(int64_t n, F&& launch) {
    for (int64_t i0 = 0; i0 < n; i0 += kLaneChunk) {
        launch(i0, dim3(blocks_for(std::min(kLaneChunk, n - i0), 256)));
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    return SVO_OK;
}

}  // namespace
