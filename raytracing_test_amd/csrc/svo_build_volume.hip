// svo_build_volume.hip — trees from dense voxel volumes in HBM, and the read-back of a resident tree into one.
//
// svo_build_volume_gpu: the volume is a (nz, ny, nx) box of palette ids somewhere in the world (origin need not be a
// multiple of 4, so brick boundaries may fall inside it; everything outside the box is empty).
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
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"

using namespace svo;

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
    if (v->view != SVO_VIEW_SOLID && v->view != SVO_VIEW_ALL) SVO_FAIL(SVO_EINVAL, w + ": unknown view");
    if (v->n_palette < 1 || v->n_palette > 65535) SVO_FAIL(SVO_ERANGE, w + ": n_palette must be in [1, 65535]");
    if (v->palette[0].flags != 0 || v->palette[0].color != ~0ull || v->palette[0].metadata != 0.0f)
        SVO_FAIL(SVO_EINVAL, w + ": palette[0] must be the empty block {0, ~0, 0}");
    return SVO_OK;
}

// the desc as the kernels see it: the stored palette (flags 1 | flags, as putBlock stores them), the in-view bit table
// in HBM, the geometry of the class pyramid.  `all` = every id but 0 is in view (the table need not be consulted).
int prepare(const svo_volume_desc* v, Pool& pool, DevVolume& V, std::vector<Material>& pal, bool& all) {
    memset(&V, 0, sizeof(V));
    V.vox = v->voxels;
    V.nx = v->nx;
    V.ny = v->ny;
    V.nz = v->nz;
    V.n_pal = v->n_palette;
    pal.clear();
    pal.push_back(Material{0, ~0ull, 0.0f});
    for (uint32_t i = 1; i < v->n_palette; i++) pal.push_back(Material{1u | v->palette[i].flags, v->palette[i].color, v->palette[i].metadata});
    std::vector<uint32_t> bits((v->n_palette + 31u) / 32u, 0u);
    all = true;
    for (uint32_t i = 1; i < v->n_palette; i++) {
        if (material_in_view(pal[i], v->view)) bits[i >> 5] |= 1u << (i & 31u);
        else all = false;
    }
    uint32_t* dbits;
    int rc = pool.alloc(&dbits, bits.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dbits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice), SVO_EDEVICE);
    V.in_view = dbits;
    const int32_t n[3] = {v->nx, v->ny, v->nz};
    for (int a = 0; a < 3; a++) V.o[a] = v->origin[a];
    for (int k = 1; k <= v->levels; k++)
        for (int a = 0; a < 3; a++) {
            V.lo[k][a] = v->origin[a] >> (2 * k);
            V.dim[k][a] = ((v->origin[a] + n[a] - 1) >> (2 * k)) - V.lo[k][a] + 1;
        }
    return SVO_OK;
}

int open_device(int32_t device, const char* who) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), SVO_EDEVICE);
    if (device < 0 || device >= ndev) SVO_FAIL(SVO_EDEVICE, std::string(who) + ": no such HIP device");
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    // the volume may have been produced on another stream; the build then runs on the null stream
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    return SVO_OK;
}

// level 1 of the pyramid into c1 (dim[1] cells)
int launch_classes(const DevVolume& V, bool all, uint16_t* c1, int32_t* bad) {
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
    int32_t* dbad;
    rc = pool.alloc(&dbad, 1);
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
    int32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_build_volume_gpu: a voxel id is not below n_palette");
    uint16_t top = 0;  // the box lies within the extent: the top level is the one cell that is the root
    HIP_TRY(hipMemcpy(&top, cls[levels], 2, hipMemcpyDeviceToHost), SVO_EDEVICE);

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
