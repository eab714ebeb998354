// svo_build_args.h — host helpers shared by the builders that take their content from HBM under a caller's palette
// (svo_build_volume.hip: a dense volume; svo_build_points.hip: a sparse list of voxels): the argument checks on the view
// and the palette, the device a build runs on, and the palette as the kernels see it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"

namespace {

// the view and the palette of a desc: before any HIP call, so that a machine without a GPU still reports them
inline int check_view_palette(int32_t view, const svo_block* palette, uint32_t n_palette, const std::string& w) {
    if (view != SVO_VIEW_SOLID && view != SVO_VIEW_ALL) SVO_FAIL(SVO_EINVAL, w + ": unknown view");
    if (n_palette < 1 || n_palette > 65535) SVO_FAIL(SVO_ERANGE, w + ": n_palette must be in [1, 65535]");
    if (palette[0].flags != 0 || palette[0].color != ~0ull || palette[0].metadata != 0.0f)
        SVO_FAIL(SVO_EINVAL, w + ": palette[0] must be the empty block {0, ~0, 0}");
    return SVO_OK;
}

inline int open_device(int32_t device, const char* who) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), SVO_EDEVICE);
    if (device < 0 || device >= ndev) SVO_FAIL(SVO_EDEVICE, std::string(who) + ": no such HIP device");
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    // the content may have been produced on another stream; the build then runs on the null stream
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    return SVO_OK;
}

// The stored palette (flags 1 | flags, as putBlock stores them) and the in-view bit table in HBM (bit id: the tree's view
// stores palette id).  `all` = every id but 0 is in view (the table need not be consulted).
inline int view_table(const svo_block* palette, uint32_t n_palette, int32_t view, Pool& pool, std::vector<Material>& pal,
                      const uint32_t** in_view, bool& all) {
    pal.clear();
    pal.push_back(Material{0, ~0ull, 0.0f});
    for (uint32_t i = 1; i < n_palette; i++) pal.push_back(Material{1u | palette[i].flags, palette[i].color, palette[i].metadata});
    std::vector<uint32_t> bits((n_palette + 31u) / 32u, 0u);
    all = true;
    for (uint32_t i = 1; i < n_palette; i++) {
        if (material_in_view(pal[i], view)) bits[i >> 5] |= 1u << (i & 31u);
        else all = false;
    }
    uint32_t* dbits;
    int rc = pool.alloc(&dbits, bits.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dbits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice), SVO_EDEVICE);
    *in_view = dbits;
    return SVO_OK;
}

}  // namespace
