// svo_build.hip — on-device world generation and tree build.
//
// genWorld's column tops (world_gen.cpp:22, OpenSimplex 2D from include/OpenSimplexNoise.cpp:77-208)
// are evaluated one column per lane, then the same canonical breadth-first tree the host terrain
// builder emits (svo_terrain.cpp build_from_heights) is built level by level on the GPU:
//   * a min/max height pyramid over aligned 4^k column footprints classifies any aligned region
//     in O(1) (EMPTY / uniform SOLID / MIXED, the host's classify_region);
//   * one wavefront per region, one lane per child slot (or per voxel at the brick level):
//     ballots give the child mask, the MIXED children and the solid voxels; exclusive scans over
//     the regions (hipCUB) place every child block and material run; a second pass writes them
//     (svo_build_emit.h, shared with the volume builder; the terrain is one source of it).
// The node array is identical, byte for byte, to svo_build_terrain's (tests), and it stays in HBM
// (adopted as the uploaded copy); the host image is copied back for host queries and edits.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_noise.h"

using namespace svo;

namespace {

// the emitter's source over genWorld's columns
struct DevTerrain {
    int32_t levels, E, W, L;
    const int16_t* h;  // [x*L + z]
    const int16_t* hmin[kMaxPyr];
    const int16_t* hmax[kMaxPyr];
    int32_t dimz[kMaxPyr];
    uint32_t id_of[5];
    int32_t view;  // SVO_VIEW_SOLID / SVO_VIEW_ALL

    // svo_terrain.cpp classify_region: class of the aligned region [x0,x0+s)x[y0,y0+s)x[z0,z0+s), s = 4^k
    __device__ uint32_t classify(int32_t x0, int32_t y0, int32_t z0, int32_t s, int k) const {
        const int32_t y1 = y0 + s - 1;
        if (x0 >= W || z0 >= L) return G_EMPTY;
        const bool partial = (x0 + s > W) || (z0 + s > L);
        const size_t ci = (size_t)(x0 >> (2 * k)) * dimz[k] + (z0 >> (2 * k));
        const int32_t mn = hmin[k][ci], mx = hmax[k][ci];
        if (terrain_region_empty(view, mx, y0, y1)) return G_EMPTY;
        if (partial) return G_MIXED;
        return terrain_region_class(id_of, view, mn, mx, y0, y1, G_EMPTY, G_MIXED);
    }
    __device__ __forceinline__ uint32_t voxel(int32_t x, int32_t y, int32_t z) const {
        if (x >= W || z >= L) return G_EMPTY;
        return id_of[terrain_material(h[(size_t)x * L + z], y)];
    }
};

__global__ void k_heights(const uint8_t* perms, int32_t W, int32_t L, int16_t* h, int32_t* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)W * L) return;
    const int32_t x = (int32_t)(i / L), z = (int32_t)(i - (int64_t)x * L);
    const int32_t v = terrain_height(perms, perms + 256, perms + 512, x, z);
    if (v < 0 || v > 32767) atomicOr(bad, 1);
    h[i] = (int16_t)v;
}

__global__ void k_pyramid(const int16_t* pmn, const int16_t* pmx, int32_t px, int32_t pz, int16_t* mn, int16_t* mx, int32_t dx,
                          int32_t dz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)dx * dz) return;
    const int32_t cx = (int32_t)(i / dz), cz = (int32_t)(i - (int64_t)cx * dz);
    int16_t a = 32767, c = -32768;
    for (int u = 0; u < 4; u++)
        for (int v = 0; v < 4; v++) {
            const int64_t sx = (int64_t)cx * 4 + u, sz = (int64_t)cz * 4 + v;
            if (sx >= px || sz >= pz) continue;
            a = min(a, pmn[sx * pz + sz]);
            c = max(c, pmx[sx * pz + sz]);
        }
    mn[i] = a;
    mx[i] = c;
}

int build_on_device(int32_t levels, int32_t W, int32_t L, int16_t* dh, Pool& pool, int32_t device, int32_t view, svo_tree** out) {
    const int32_t E = 1 << (2 * levels);
    DevTerrain T;
    memset(&T, 0, sizeof(T));
    T.levels = levels;
    T.E = E;
    T.W = W;
    T.L = L;
    T.h = dh;
    T.id_of[TM_AIR] = G_EMPTY;
    T.id_of[TM_WATER] = view ? 4u : G_EMPTY;
    T.view = view;
    T.id_of[TM_GRASS] = 1;
    T.id_of[TM_DIRT] = 2;
    T.id_of[TM_STONE] = 3;
    // ---- min / max pyramid
    T.hmin[0] = T.hmax[0] = dh;
    T.dimz[0] = L;
    int32_t px = W, pz = L;
    for (int k = 1; k <= levels; k++) {
        const int32_t dx = (px + 3) / 4, dz = (pz + 3) / 4;
        int16_t *mn, *mx;
        int rc = pool.alloc(&mn, (size_t)dx * dz);
        if (!rc) rc = pool.alloc(&mx, (size_t)dx * dz);
        if (rc) return rc;
        hipLaunchKernelGGL(k_pyramid, dim3(blocks_for((int64_t)dx * dz, 256)), dim3(256), 0, nullptr, T.hmin[k - 1], T.hmax[k - 1], px, pz,
                           mn, mx, dx, dz);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        T.hmin[k] = mn;
        T.hmax[k] = mx;
        T.dimz[k] = dz;
        px = dx;
        pz = dz;
    }
    int16_t top_max = 0;
    HIP_TRY(hipMemcpy(&top_max, T.hmax[levels], 2, hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (top_max + 1 >= E || 21 >= E)
        SVO_FAIL(SVO_ERANGE, "svo_build_terrain_gpu: a column top falls outside [0, extent-2] (wrap not supported here)");

    svo_tree* t = new (std::nothrow) svo_tree();
    if (!t) SVO_FAIL(SVO_ENOMEM, "svo_build_terrain_gpu: out of memory");
    std::unique_ptr<svo_tree> guard(t);
    t->levels = levels;
    t->view = view;
    t->palette.push_back(Material{0, ~0ull, 0.0f});
    t->palette.push_back(Material{1u, rgb_to_u64(0, 150, 10), 0.0f});         // 1 grass
    t->palette.push_back(Material{1u, rgb_to_u64(45, 18, 0), 0.0f});          // 2 dirt
    t->palette.push_back(Material{1u, rgb_to_u64(33, 33, 33), 0.0f});         // 3 stone
    t->palette.push_back(Material{1u | 0x14u, rgb_to_u64(0, 150, 10), 0.0f});  // 4 water (LIQUID)

    // (the root is never EMPTY or uniform SOLID: the extent reaches above every column, checked above)
    const int rc = emit_tree(T, levels, G_MIXED, t, pool, device, "svo_build_terrain_gpu");
    if (rc) return rc;
    *out = guard.release();
    return SVO_OK;
}

}  // namespace

extern "C" int svo_build_terrain_gpu(int32_t levels, int32_t width, int32_t length, int32_t device, svo_tree** out) {
    return svo_build_terrain_gpu_view(levels, width, length, device, SVO_VIEW_SOLID, out);
}

extern "C" int svo_build_terrain_gpu_view(int32_t levels, int32_t width, int32_t length, int32_t device, int32_t view, svo_tree** out) {
    if (!out) SVO_FAIL(SVO_EINVAL, "svo_build_terrain_gpu: out is NULL");
    if (view != SVO_VIEW_SOLID && view != SVO_VIEW_ALL) SVO_FAIL(SVO_EINVAL, "svo_build_terrain_gpu: unknown view");
    if (levels < 2 || levels > 7) SVO_FAIL(SVO_EINVAL, "svo_build_terrain_gpu: levels must be in [2, 7]");
    const int32_t E = 1 << (2 * levels);
    if (width < 1 || length < 1 || width > E || length > E) SVO_FAIL(SVO_EINVAL, "svo_build_terrain_gpu: columns must fit the extent");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), SVO_EDEVICE);
    if (device < 0 || device >= ndev) SVO_FAIL(SVO_EDEVICE, "svo_build_terrain_gpu: no such HIP device");
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    Pool pool;
    uint8_t perms[768];
    {
        Simplex2 a, b, c;
        simplex2_seed(a, 42);
        simplex2_seed(b, 64);
        simplex2_seed(c, 100);
        memcpy(perms, a.perm, 256);
        memcpy(perms + 256, b.perm, 256);
        memcpy(perms + 512, c.perm, 256);
    }
    uint8_t* dperm;
    int16_t* dh;
    int32_t* dbad;
    int rc = pool.alloc(&dperm, 768);
    if (!rc) rc = pool.alloc(&dh, (size_t)width * length);
    if (!rc) rc = pool.alloc(&dbad, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dperm, perms, 768, hipMemcpyHostToDevice), SVO_EDEVICE);
    HIP_TRY(hipMemset(dbad, 0, 4), SVO_EDEVICE);
    hipLaunchKernelGGL(k_heights, dim3(blocks_for((int64_t)width * length, 256)), dim3(256), 0, nullptr, dperm, width, length, dh, dbad);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    int32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_build_terrain_gpu: a column top falls outside [0, 32767]");
    return build_on_device(levels, width, length, dh, pool, device, view, out);
}

extern "C" int svo_build_heightfield_gpu(int32_t levels, int32_t width, int32_t length, const int32_t* heights, int32_t device,
                                         svo_tree** out) {
    if (!out || !heights) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield_gpu: NULL argument");
    if (levels < 2 || levels > 7) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield_gpu: levels must be in [2, 7]");
    const int32_t E = 1 << (2 * levels);
    if (width < 1 || length < 1 || width > E || length > E) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield_gpu: columns must fit the extent");
    std::vector<int16_t> hg((size_t)width * length);
    for (size_t i = 0; i < hg.size(); i++) {
        if (heights[i] < 0 || heights[i] > 32767) SVO_FAIL(SVO_ERANGE, "svo_build_heightfield_gpu: heights must be in [0, extent-2]");
        hg[i] = (int16_t)heights[i];
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), SVO_EDEVICE);
    if (device < 0 || device >= ndev) SVO_FAIL(SVO_EDEVICE, "svo_build_heightfield_gpu: no such HIP device");
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    Pool pool;
    int16_t* dh;
    int rc = pool.alloc(&dh, hg.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dh, hg.data(), hg.size() * sizeof(int16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    return build_on_device(levels, width, length, dh, pool, device, SVO_VIEW_SOLID, out);
}
