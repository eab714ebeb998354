// svo_build_volume.hip — trees from dense voxel volumes in HBM, and the read-back of a resident tree into one.
//
// svo_build_volume_gpu: the volume is a (nz, ny, nx) box of palette ids somewhere in the world (origin need not be a
// multiple of 4, so brick boundaries may fall inside it; everything outside the box is empty).
//   * class pyramid, bottom up, over the world-aligned bounding box of the volume (svo_volume_pyramid.h, shared with the
//     patch of resident trees, svo_patch_volume.hip): level 1 reads the whole volume once and checks the ids.
//   * emission, top down: svo_build_emit.h with this source — region classes are looked up in the pyramid, brick voxels
//     are read from the volume.
// svo_tree_read_volume: one lane per output voxel, x fastest; svo_tree_get_block's descent over the device arrays.
// Every index into a volume is 64-bit, and every dispatch holds fewer than 2^32 work-items.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_args.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_volume_pyramid.h"

using namespace svo;

namespace {

// svo_tree_get_block's descent for voxels i0 .. of the box, one lane each
__global__ void k_read_volume(const Node* nodes, const uint16_t* mats, int32_t levels, uint32_t ox, uint32_t oy, uint32_t oz, int32_t nx,
                              int32_t ny, int64_t i0, int64_t total, uint16_t* out) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t yz = i / nx;
    const uint32_t mk = (1u << (2 * levels)) - 1u;
    const uint32_t wx = (ox + (uint32_t)(i - yz * nx)) & mk, wy = (oy + (uint32_t)(yz % ny)) & mk, wz = (oz + (uint32_t)(yz / ny)) & mk;
    uint64_t ni = 0;
    uint32_t mat = 0;
    for (int d = 0; d < levels; d++) {
        const Node n = nodes[ni];
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) {
            mat = node_material(n.info);
            break;
        }
        if (kind == K_BRICK) {
            const uint32_t v = ((wz & 3u) << 4) | ((wy & 3u) << 2) | (wx & 3u);
            if ((n.mask >> v) & 1ull)
                mat = (n.info & K_UNIFORM) ? node_material(n.info) : mats[(uint64_t)n.ref + (uint64_t)__popcll(n.mask & ((1ull << v) - 1ull))];
            break;
        }
        const uint32_t sh = (uint32_t)(2 * (levels - 1 - d));
        const uint32_t sl = (((wz >> sh) & 3u) << 4) | (((wy >> sh) & 3u) << 2) | ((wx >> sh) & 3u);
        if (!((n.mask >> sl) & 1ull)) break;
        ni = (uint64_t)n.ref + (uint64_t)__popcll(n.mask & ((1ull << sl) - 1ull));
    }
    out[i] = (uint16_t)mat;
}

// argument checks of a volume desc: before any HIP call, so that a machine without a GPU still reports them
int check_desc(const svo_volume_desc* v, const char* who) {
    const std::string w(who);
    if (!v) SVO_FAIL(SVO_EINVAL, w + ": desc is NULL");
    if (!v->voxels || !v->palette) SVO_FAIL(SVO_EINVAL, w + ": NULL voxels or palette");
    if (v->levels < 2 || v->levels > 7) SVO_FAIL(SVO_EINVAL, w + ": levels must be in [2, 7]");
    if (v->nx < 1 || v->ny < 1 || v->nz < 1) SVO_FAIL(SVO_EINVAL, w + ": dimensions must be positive");
    const int64_t E = (int64_t)1 << (2 * v->levels);
    const int32_t n[3] = {v->nx, v->ny, v->nz};
    for (int a = 0; a < 3; a++)
        if (v->origin[a] < 0 || (int64_t)v->origin[a] + n[a] > E) SVO_FAIL(SVO_EINVAL, w + ": the box must lie within the extent (no wrap)");
    if (int rc = check_view_palette(v->view, v->palette, v->n_palette, w)) return rc;
    return SVO_OK;
}

}  // namespace

extern "C" int svo_build_volume_gpu(const svo_volume_desc* v, svo_tree** out) {
    const char* who = "svo_build_volume_gpu";
    if (!out) SVO_FAIL(SVO_EINVAL, "svo_build_volume_gpu: out is NULL");
    int rc = check_desc(v, who);
    if (!rc) rc = open_device(v->device, who);
    if (rc) return rc;
    Pool pool;
    DevVolume V;
    std::vector<Material> pal;
    bool all = false;
    rc = prepare(v, pool, V, pal, all);
    if (rc) return rc;
    const int32_t levels = v->levels;
    bool bad = false;
    uint16_t top = 0;  // the box lies within the extent: the top level is the one cell that is the root
    rc = build_pyramid(V, levels, all, pool, &bad, &top);
    if (rc) return rc;
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_build_volume_gpu: a voxel id is not below n_palette");

    svo_tree* t = new (std::nothrow) svo_tree();
    if (!t) SVO_FAIL(SVO_ENOMEM, "svo_build_volume_gpu: out of memory");
    std::unique_ptr<svo_tree> guard(t);
    t->levels = levels;
    t->view = v->view;
    t->palette = pal;
    rc = emit_tree(V, levels, top == C_MIXED ? G_MIXED : (uint32_t)top, t, pool, v->device, who);
    if (rc) return rc;
    *out = guard.release();
    return SVO_OK;
}

extern "C" int svo_volume_classify_pass(const svo_volume_desc* v, int32_t runs, float* ms) {
    const char* who = "svo_volume_classify_pass";
    if (!ms || runs < 1) SVO_FAIL(SVO_EINVAL, "svo_volume_classify_pass: bad argument");
    int rc = check_desc(v, who);
    if (!rc) rc = open_device(v->device, who);
    if (rc) return rc;
    Pool pool;
    DevVolume V;
    std::vector<Material> pal;
    bool all = false;
    rc = prepare(v, pool, V, pal, all);
    if (rc) return rc;
    int32_t* dbad;
    uint16_t* c1;
    rc = pool.alloc(&dbad, 1);
    if (!rc) rc = pool.alloc(&c1, (size_t)cells(V, 1));
    if (rc) return rc;
    HIP_TRY(hipMemset(dbad, 0, 4), SVO_EDEVICE);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0), SVO_EDEVICE);
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        SVO_FAIL(SVO_EDEVICE, "svo_volume_classify_pass: hipEventCreate failed");
    }
    for (int32_t i = 0; i < runs && !rc; i++) {
        hipError_t e = hipEventRecord(e0, nullptr);
        rc = launch_classes(V, all, c1, dbad);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[i], e0, e1);
        if (!rc && e != hipSuccess) {
            set_error(std::string("svo_volume_classify_pass: ") + hipGetErrorString(e));
            rc = SVO_EDEVICE;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

extern "C" int svo_tree_read_volume(const svo_tree* t, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz, uint16_t* voxels,
                                    void* hip_stream) {
    if (!t || !origin || !voxels) SVO_FAIL(SVO_EINVAL, "svo_tree_read_volume: NULL argument");
    if (nx < 1 || ny < 1 || nz < 1) SVO_FAIL(SVO_EINVAL, "svo_tree_read_volume: dimensions must be positive");
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_read_volume: tree not uploaded (svo_upload)");
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    const int64_t total = (int64_t)nx * ny * nz, chunk = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < total; i0 += chunk) {
        hipLaunchKernelGGL(k_read_volume, dim3(blocks_for(std::min(chunk, total - i0), 256)), dim3(256), 0, (hipStream_t)hip_stream,
                           reinterpret_cast<const Node*>(t->d_nodes), reinterpret_cast<const uint16_t*>(t->d_mats), t->levels,
                           (uint32_t)origin[0], (uint32_t)origin[1], (uint32_t)origin[2], nx, ny, i0, total, voxels);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    return SVO_OK;
}
