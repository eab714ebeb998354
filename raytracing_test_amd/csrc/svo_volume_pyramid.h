// svo_volume_pyramid.h — the class pyramid over a dense box of voxels in HBM and the emitter's source that reads it, shared
// by the volume builder (svo_build_volume.hip: the box is the whole content of a new tree) and the volume patch
// (svo_patch_volume.hip: the box replaces a part of a resident tree).
//   * class pyramid, bottom up, over the world-aligned bounding box of the volume: level 1 holds one 16-bit class word
//     per world-aligned 4^3 brick — C_EMPTY, an id (all 64 voxels that one in-view id) or C_MIXED — and levels 2..levels
//     fold 64 child classes each (all equal and not MIXED: that class; else MIXED; children outside the box are EMPTY:
//     svo_world.h fold_classes).  Level 1 reads the whole volume once and is the memory-bound pass: a block takes a
//     strip of 128 bricks along x of one (y, z) brick row; a lane loads 8 consecutive voxels (16 B at any even address,
//     two bricks) of two of the strip's 16 rows, 8 neighbouring lanes read 128 contiguous bytes of a row, and the 8
//     lanes holding the 16 rows of the same two bricks (8, 16 and 32 lanes apart) fold their class words by three lane
//     exchanges.  (With the 16 rows of a span in 16 neighbouring lanes instead — 64 contiguous bytes per row and load —
//     the pass ran at 4.7 instead of 5.6-5.7 TB/s.)  Ids are checked against the palette size on the way (an atomicOr flag, as k_heights
//     reports a bad height), and ids out of the tree's view count as empty through a bit table kept in LDS.
// Every index into a volume is 64-bit, and every dispatch holds fewer than 2^32 work-items.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_args.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"

namespace {

constexpr uint32_t C_EMPTY = 0u, C_MIXED = 0xFFFFu;  // 16-bit class words (ids are below 65535)

// the emitter's source over a dense volume
struct DevVolume {
    const uint16_t* vox;  // [(z * ny + y) * nx + x]
    int32_t nx, ny, nz;
    int32_t o[3];             // world position of vox[0]
    uint32_t n_pal;
    const uint32_t* in_view;  // bit id: palette id is stored by the tree's view
    const uint16_t* cls[kMaxPyr];              // level k = 1..levels: classes of the 4^k cells of the bounding box
    int32_t lo[kMaxPyr][3], dim[kMaxPyr][3];   // first cell and cell counts of level k, per axis (x, y, z)

    __device__ uint32_t classify(int32_t x0, int32_t y0, int32_t z0, int32_t, int k) const {
        const uint32_t cx = (uint32_t)((x0 >> (2 * k)) - lo[k][0]), cy = (uint32_t)((y0 >> (2 * k)) - lo[k][1]),
                       cz = (uint32_t)((z0 >> (2 * k)) - lo[k][2]);
        if (cx >= (uint32_t)dim[k][0] || cy >= (uint32_t)dim[k][1] || cz >= (uint32_t)dim[k][2]) return G_EMPTY;
        const uint32_t c = cls[k][((int64_t)cz * dim[k][1] + cy) * dim[k][0] + cx];
        return c == C_MIXED ? G_MIXED : c;
    }
    __device__ __forceinline__ uint32_t voxel(int32_t x, int32_t y, int32_t z) const {
        const uint32_t vx = (uint32_t)(x - o[0]), vy = (uint32_t)(y - o[1]), vz = (uint32_t)(z - o[2]);
        if (vx >= (uint32_t)nx || vy >= (uint32_t)ny || vz >= (uint32_t)nz) return G_EMPTY;
        const uint32_t id = vox[((int64_t)vz * ny + vy) * nx + vx];
        if (id >= n_pal) return G_EMPTY;  // (never: the classification pass has checked every id)
        return ((in_view[id >> 5] >> (id & 31u)) & 1u) ? id : G_EMPTY;
    }
};

// fold of class words: equal -> that class, else MIXED (MIXED absorbs: it equals no id)
__device__ __forceinline__ uint32_t fold2(uint32_t a, uint32_t b) { return a == b ? a : C_MIXED; }

// the value of another lane of the same row of 16 lanes (DPP: no LDS traffic).  0x128: row_ror:8, the lane 8 away
template <int kCtrl>
__device__ __forceinline__ uint32_t row_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}

// two class words at once (low and high halves)
__device__ __forceinline__ uint32_t fold_pair(uint32_t a, uint32_t b) {
    return fold2(a & 0xFFFFu, b & 0xFFFFu) | (fold2(a >> 16, b >> 16) << 16);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(2))) Row8 {  // 8 voxels of a row: 16 B at any even address
    u32x4 v;
};

constexpr int kStripBricks = 128;                   // bricks along x per block: 64 per pass of its 4 waves (8 spans of two bricks each)
constexpr int64_t kStripChunk = (int64_t)1 << 22;   // blocks per dispatch (2^30 work-items)

// Level 1 of the class pyramid.  Block b (of `nblocks` from b0 on) = strip sx of brick row (by, bz).  Lane t: span
// s = t & 7 of its wave's 8 spans (8 lanes = 128 contiguous bytes of a row), rows q and q + 8 with q = (t >> 3) & 7
// (row r: y = r & 3, z = r >> 2 within the brick row); wave t >> 6 takes spans 8 (t >> 6) .. + 8 of every 32.
template <bool kMap>
__global__ __launch_bounds__(256) void k_vol_classes(DevVolume V, int64_t b0, int32_t strips, uint16_t* out, int32_t* bad) {
    __shared__ uint32_t s_view[kMap ? 2048 : 1];
    const uint32_t t = threadIdx.x;
    if (kMap) {
        const uint32_t words = (V.n_pal + 31u) >> 5;  // <= 2048
        for (uint32_t i = t; i < words; i += 256u) s_view[i] = V.in_view[i];
        __syncthreads();
    }
    const int64_t b = b0 + blockIdx.x;
    const int32_t sx = (int32_t)(b % strips);
    const int64_t row = b / strips;
    const int32_t by = (int32_t)(row % V.dim[1][1]), bz = (int32_t)(row / V.dim[1][1]);  // (the grid holds only whole rows of the box)
    const uint32_t q = (t >> 3) & 7u;
    constexpr int kIter = kStripBricks / 64;
    const uint16_t* rowp[2];
    bool row_in[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t r = q + 8u * h;
        const int32_t vy = ((V.lo[1][1] + by) << 2) + (int32_t)(r & 3u) - V.o[1], vz = ((V.lo[1][2] + bz) << 2) + (int32_t)(r >> 2) - V.o[2];
        row_in[h] = (uint32_t)vy < (uint32_t)V.ny && (uint32_t)vz < (uint32_t)V.nz;
        rowp[h] = V.vox + (row_in[h] ? ((int64_t)vz * V.ny + vy) * V.nx : 0);
    }
    uint32_t ids[kIter][2][8];
    int32_t bx[kIter];
#pragma unroll
    for (int u = 0; u < kIter; u++) {  // the loads first: every lane has its bytes in flight before it folds
        bx[u] = sx * kStripBricks + 2 * (32 * u + 8 * (int32_t)(t >> 6) + (int32_t)(t & 7u));  // first brick of the span, within the box
        const int32_t vx = ((V.lo[1][0] + bx[u]) << 2) - V.o[0];                             // its first voxel in the volume (-3 .. )
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int i = 0; i < 8; i++) ids[u][h][i] = 0u;
            if (!row_in[h] || bx[u] >= V.dim[1][0]) continue;
            if (vx >= 0 && vx + 8 <= V.nx) {
                const u32x4 w = reinterpret_cast<const Row8*>(rowp[h] + vx)->v;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    ids[u][h][2 * i] = w[i] & 0xFFFFu;
                    ids[u][h][2 * i + 1] = w[i] >> 16;
                }
            } else {  // a span over the box's x faces
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if ((uint32_t)(vx + i) < (uint32_t)V.nx) ids[u][h][i] = rowp[h][vx + i];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kIter; u++) {
        if (bx[u] >= V.dim[1][0]) continue;  // (the same for the 8 lanes of a span, which exchange below)
        bool oob = false;
        uint32_t ac2[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t id = ids[u][h][i];
                if (id >= V.n_pal) {
                    oob = true;
                    id = 0u;
                }
                if (kMap) id = ((s_view[id >> 5] >> (id & 31u)) & 1u) ? id : 0u;
                ids[u][h][i] = id;
            }
            const uint32_t a = fold2(fold2(ids[u][h][0], ids[u][h][1]), fold2(ids[u][h][2], ids[u][h][3]));
            const uint32_t c = fold2(fold2(ids[u][h][4], ids[u][h][5]), fold2(ids[u][h][6], ids[u][h][7]));
            ac2[h] = a | (c << 16);
        }
        if (oob) atomicOr(bad, 1);
        // the 16 rows of the two bricks: two in this lane, the others in the lanes 8, 16 and 32 away — every lane ends
        // with the fold of all 16 (the fold is commutative and idempotent)
        uint32_t ac = fold_pair(ac2[0], ac2[1]);
        ac = fold_pair(ac, row_lane<0x128>(ac));
        ac = fold_pair(ac, (uint32_t)__shfl_xor((int)ac, 16));
        ac = fold_pair(ac, (uint32_t)__shfl_xor((int)ac, 32));
        if (q == 0) {
            uint16_t* dst = out + ((int64_t)bz * V.dim[1][1] + by) * V.dim[1][0] + bx[u];
            dst[0] = (uint16_t)(ac & 0xFFFFu);
            if (bx[u] + 1 < V.dim[1][0]) dst[1] = (uint16_t)(ac >> 16);
        }
    }
}

// levels 2..levels: one lane per parent cell folds its 64 children (those outside the child level's box are EMPTY)
__global__ void k_vol_fold(const uint16_t* child, int32_t clx, int32_t cly, int32_t clz, int32_t cdx, int32_t cdy, int32_t cdz,
                           uint16_t* parent, int32_t plx, int32_t ply, int32_t plz, int32_t pdx, int32_t pdy, int32_t pdz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)pdx * pdy * pdz) return;
    const int32_t px = (int32_t)(i % pdx), py = (int32_t)((i / pdx) % pdy), pz = (int32_t)(i / ((int64_t)pdx * pdy));
    const int32_t x0 = ((plx + px) << 2) - clx, y0 = ((ply + py) << 2) - cly, z0 = ((plz + pz) << 2) - clz;
    uint32_t f = 0u;
    for (int s = 0; s < 64; s++) {
        const uint32_t x = (uint32_t)(x0 + (s & 3)), y = (uint32_t)(y0 + ((s >> 2) & 3)), z = (uint32_t)(z0 + (s >> 4));
        uint32_t c = C_EMPTY;
        if (x < (uint32_t)cdx && y < (uint32_t)cdy && z < (uint32_t)cdz) c = child[((int64_t)z * cdy + y) * cdx + x];
        f = s == 0 ? c : fold2(f, c);
    }
    parent[i] = (uint16_t)f;
}

// the desc as the kernels see it: the stored palette and the in-view bit table in HBM (svo_build_args.h view_table),
// the geometry of the class pyramid.  `all` = every id but 0 is in view (the table need not be consulted).
inline int prepare(const svo_volume_desc* v, Pool& pool, DevVolume& V, std::vector<Material>& pal, bool& all) {
    memset(&V, 0, sizeof(V));
    V.vox = v->voxels;
    V.nx = v->nx;
    V.ny = v->ny;
    V.nz = v->nz;
    V.n_pal = v->n_palette;
    int rc = view_table(v->palette, v->n_palette, v->view, pool, pal, &V.in_view, all);
    if (rc) return rc;
    const int32_t n[3] = {v->nx, v->ny, v->nz};
    for (int a = 0; a < 3; a++) V.o[a] = v->origin[a];
    for (int k = 1; k <= v->levels; k++)
        for (int a = 0; a < 3; a++) {
            V.lo[k][a] = v->origin[a] >> (2 * k);
            V.dim[k][a] = ((v->origin[a] + n[a] - 1) >> (2 * k)) - V.lo[k][a] + 1;
        }
    return SVO_OK;
}

// level 1 of the pyramid into c1 (dim[1] cells)
inline int launch_classes(const DevVolume& V, bool all, uint16_t* c1, int32_t* bad) {
    const int32_t strips = (V.dim[1][0] + kStripBricks - 1) / kStripBricks;
    const int64_t nblocks = (int64_t)strips * V.dim[1][1] * V.dim[1][2];
    for (int64_t b0 = 0; b0 < nblocks; b0 += kStripChunk) {
        const dim3 g((uint32_t)std::min(kStripChunk, nblocks - b0));
        if (all) hipLaunchKernelGGL(k_vol_classes<false>, g, dim3(256), 0, nullptr, V, b0, strips, c1, bad);
        else hipLaunchKernelGGL(k_vol_classes<true>, g, dim3(256), 0, nullptr, V, b0, strips, c1, bad);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    return SVO_OK;
}

inline int64_t cells(const DevVolume& V, int k) { return (int64_t)V.dim[k][0] * V.dim[k][1] * V.dim[k][2]; }

// The whole pyramid of a prepared volume, levels 1..levels, allocated from `pool` and hung into V.cls.  *bad: an id was
// not below the palette size (nothing may be emitted from the pyramid then); *top: the class word of the one cell of
// level `levels` (the box lies within the extent).
inline int build_pyramid(DevVolume& V, int32_t levels, bool all, Pool& pool, bool* bad, uint16_t* top) {
    int32_t* dbad;
    int rc = pool.alloc(&dbad, 1);
    if (rc) return rc;
    HIP_TRY(hipMemset(dbad, 0, 4), SVO_EDEVICE);
    uint16_t* cls[kMaxPyr] = {nullptr};
    for (int k = 1; k <= levels; k++) {
        rc = pool.alloc(&cls[k], (size_t)cells(V, k));
        if (rc) return rc;
        V.cls[k] = cls[k];
    }
    rc = launch_classes(V, all, cls[1], dbad);
    if (rc) return rc;
    for (int k = 2; k <= levels; k++) {
        hipLaunchKernelGGL(k_vol_fold, dim3(blocks_for(cells(V, k), 256)), dim3(256), 0, nullptr, cls[k - 1], V.lo[k - 1][0], V.lo[k - 1][1],
                           V.lo[k - 1][2], V.dim[k - 1][0], V.dim[k - 1][1], V.dim[k - 1][2], cls[k], V.lo[k][0], V.lo[k][1], V.lo[k][2],
                           V.dim[k][0], V.dim[k][1], V.dim[k][2]);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    int32_t b = 0;
    HIP_TRY(hipMemcpy(&b, dbad, 4, hipMemcpyDeviceToHost), SVO_EDEVICE);
    *bad = b != 0;
    *top = 0;
    HIP_TRY(hipMemcpy(top, cls[levels], 2, hipMemcpyDeviceToHost), SVO_EDEVICE);
    return SVO_OK;
}

}  // namespace
