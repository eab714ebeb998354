// svo_build_points.hip — trees from sparse lists of voxels in HBM, and the lookup of scattered voxels in a resident tree.
//
// svo_build_points_gpu: n points (x, y, z, id), applied in list order (the last entry of a voxel decides).  The cost
// follows the number of points, never the extent's volume:
//   * key pass: one lane per point computes its 64-bit cell key (svo_points_source.h) and checks the id and the
//     coordinates (an atomicOr flag, read on the host before anything else is allocated);
//   * a stable radix sort of (key, id) over the key's 6 * levels bits (hipCUB): the entries of a voxel end up next to
//     each other in list order (both in svo_point_keys.h, shared with svo_patch_points.hip), so the last of each run
//     of equal keys is the voxel's content; it is stored unless its id is 0 or out of the tree's view, and the stored
//     voxels are compacted to level 0;
//   * class levels, bottom up: level k's cells are the runs of level k - 1 under key >> 6; a run of 64 children that
//     all carry one id has that id for its class, every other run is MIXED (absent cells are empty: no class);
//   * emission, top down: svo_build_emit.h over PointSource, which finds a cell by binary search in its level.
// svo_tree_get_blocks_gpu: one lane per position over svo_tree_descent.h.
// Every index into a list is 64-bit, and every dispatch holds fewer than 2^32 work-items.
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
#include "svo_point_keys.h"
#include "svo_points_source.h"
#include "svo_tree_descent.h"

using namespace svo;

namespace {

// sorted entries: 1 for the last entry of a voxel when it is stored
__global__ void k_point_winners(const uint64_t* keys, const uint16_t* vals, int64_t n, const uint32_t* in_view, uint32_t* keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = vals[i];
    const bool last = i + 1 == n || keys[i + 1] != keys[i];
    keep[i] = (last && id != 0u && ((in_view[id >> 5] >> (id & 31u)) & 1u)) ? 1u : 0u;
}

__global__ void k_point_compact(const uint64_t* keys, const uint16_t* vals, const uint32_t* keep, const uint64_t* off, int64_t n,
                                uint64_t* okeys, uint16_t* ovals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    okeys[off[i]] = keys[i];
    ovals[off[i]] = vals[i];
}

// a level's cells: 1 for the first child of every parent
__global__ void k_cell_heads(const uint64_t* ckeys, int64_t n, uint32_t* head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || (ckeys[i - 1] >> 6) != (ckeys[i] >> 6)) ? 1u : 0u;
}

__global__ void k_cell_parents(const uint64_t* ckeys, const uint32_t* head, const uint64_t* off, int64_t n, uint64_t* pkeys, uint32_t* pstart) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    pkeys[off[i]] = ckeys[i] >> 6;
    pstart[off[i]] = (uint32_t)i;  // (n < 2^31)
}

// one lane per parent: its class from the run of its children [pstart[p], pstart[p + 1])
__global__ void k_cell_classes(const uint16_t* ccls, const uint32_t* pstart, int64_t np, int64_t nc, uint16_t* pcls) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int64_t s = pstart[p], e = p + 1 < np ? (int64_t)pstart[p + 1] : nc;
    uint32_t c = P_MIXED;
    if (e - s == 64) {
        c = ccls[s];
        for (int j = 1; j < 64; j++)
            if (ccls[s + j] != c) {
                c = P_MIXED;
                break;
            }
    }
    pcls[p] = (uint16_t)c;
}

struct DevTree {
    const Node* nodes;
    const uint16_t* mats;
    int32_t levels;
};

__global__ void k_get_blocks(DevTree P, const int32_t* xyz, int64_t i0, int64_t n, uint16_t* ids) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t mk = (1u << (2 * P.levels)) - 1u;
    ids[i] = (uint16_t)old_voxel(P, (uint32_t)xyz[3 * i] & mk, (uint32_t)xyz[3 * i + 1] & mk, (uint32_t)xyz[3 * i + 2] & mk);
}

// argument checks of a points desc: before any HIP call, so that a machine without a GPU still reports them
int check_points(const svo_points_desc* p, const std::string& w) {
    if (!p) SVO_FAIL(SVO_EINVAL, w + ": desc is NULL");
    if (p->n < 0) SVO_FAIL(SVO_EINVAL, w + ": n must not be negative");
    if (p->n > 0 && (!p->xyz || !p->ids)) SVO_FAIL(SVO_EINVAL, w + ": NULL xyz or ids");
    if (!p->palette) SVO_FAIL(SVO_EINVAL, w + ": NULL palette");
    if (p->levels < 2 || p->levels > 7) SVO_FAIL(SVO_EINVAL, w + ": levels must be in [2, 7]");
    if (p->n > 0x7FFFFFFFll) SVO_FAIL(SVO_ERANGE, w + ": n must be below 2^31");
    return check_view_palette(p->view, p->palette, p->n_palette, w);
}

// The cell levels of the list, allocated from `pool` and hung into S; *bad: the key pass's flag word (nothing else is
// allocated or built then).
int build_levels(const svo_points_desc* p, const uint32_t* in_view, Pool& pool, PointSource& S, int32_t* bad) {
    memset(&S, 0, sizeof(S));
    S.levels = p->levels;
    *bad = 0;
    const int64_t n = p->n;
    if (n == 0) return SVO_OK;
    SortedPoints P;
    int rc = sort_point_keys(p->xyz, p->ids, n, p->levels, p->n_palette, pool, &P, bad);
    if (rc || *bad) return rc;
    const uint64_t* keys = P.keys;
    const uint16_t* vals = P.vals;
    uint64_t* off = P.spare;  // the sort's other key buffer: the scans' output from here on (n entries at most)
    uint32_t* flag;
    rc = pool.alloc(&flag, (size_t)n);
    if (rc) return rc;
    ScanTmp scan_tmp;

    // level 0: the stored voxels
    hipLaunchKernelGGL(k_point_winners, lanes(n), dim3(256), 0, nullptr, keys, vals, n, in_view, flag);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    uint64_t n0 = 0;
    rc = scan(flag, off, n, &n0, scan_tmp.v);
    if (rc) return rc;
    if (n0 == 0) {
        HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
        return SVO_OK;
    }
    uint64_t* ck;
    uint16_t* cc;
    rc = pool.alloc(&ck, (size_t)n0);
    if (!rc) rc = pool.alloc(&cc, (size_t)n0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_point_compact, lanes(n), dim3(256), 0, nullptr, keys, vals, flag, off, n, ck, cc);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    S.key[0] = ck;
    S.cls[0] = cc;
    S.n[0] = (int64_t)n0;

    // levels 1..levels: the runs of the level below
    for (int k = 1; k <= p->levels; k++) {
        const int64_t nc = S.n[k - 1];
        hipLaunchKernelGGL(k_cell_heads, lanes(nc), dim3(256), 0, nullptr, S.key[k - 1], nc, flag);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        uint64_t np = 0;
        rc = scan(flag, off, nc, &np, scan_tmp.v);
        if (rc) return rc;
        uint64_t* pk;
        uint32_t* ps;
        uint16_t* pc;
        rc = pool.alloc(&pk, (size_t)np);
        if (!rc) rc = pool.alloc(&ps, (size_t)np);
        if (!rc) rc = pool.alloc(&pc, (size_t)np);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cell_parents, lanes(nc), dim3(256), 0, nullptr, S.key[k - 1], flag, off, nc, pk, ps);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        hipLaunchKernelGGL(k_cell_classes, lanes((int64_t)np), dim3(256), 0, nullptr, S.cls[k - 1], ps, (int64_t)np, nc, pc);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
        S.key[k] = pk;
        S.cls[k] = pc;
        S.n[k] = (int64_t)np;
    }
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);  // (the scans' temporaries are freed on return)
    return SVO_OK;
}

}  // namespace

extern "C" int svo_build_points_gpu(const svo_points_desc* p, svo_tree** out) {
    const char* who = "svo_build_points_gpu";
    if (!out) SVO_FAIL(SVO_EINVAL, "svo_build_points_gpu: out is NULL");
    int rc = check_points(p, who);
    if (!rc) rc = open_device(p->device, who);
    if (rc) return rc;
    Pool pool;
    std::vector<Material> pal;
    const uint32_t* in_view = nullptr;
    bool all = false;
    rc = view_table(p->palette, p->n_palette, p->view, pool, pal, &in_view, all);
    if (rc) return rc;
    PointSource S;
    int32_t bad = 0;
    rc = build_levels(p, in_view, pool, S, &bad);
    if (rc) return rc;
    if (bad == (kBadId | kBadCoord))
        SVO_FAIL(SVO_ERANGE, "svo_build_points_gpu: a point's id is not below n_palette, and a coordinate is outside [0, 4^levels)");
    if (bad & kBadId) SVO_FAIL(SVO_ERANGE, "svo_build_points_gpu: a point's id is not below n_palette");
    if (bad & kBadCoord) SVO_FAIL(SVO_ERANGE, "svo_build_points_gpu: a coordinate is outside [0, 4^levels)");
    uint32_t root = G_EMPTY;
    if (S.n[0] > 0) {  // the top level is the one cell that is the root
        uint16_t top = 0;
        HIP_TRY(hipMemcpy(&top, S.cls[p->levels], 2, hipMemcpyDeviceToHost), SVO_EDEVICE);
        root = top == P_MIXED ? G_MIXED : (uint32_t)top;
    }

    svo_tree* t = new (std::nothrow) svo_tree();
    if (!t) SVO_FAIL(SVO_ENOMEM, "svo_build_points_gpu: out of memory");
    std::unique_ptr<svo_tree> guard(t);
    t->levels = p->levels;
    t->view = p->view;
    t->palette = pal;
    t->no_world = true;
    rc = emit_tree(S, p->levels, root, t, pool, p->device, who);
    if (rc) return rc;
    *out = guard.release();
    return SVO_OK;
}

extern "C" int svo_tree_get_blocks_gpu(const svo_tree* t, const int32_t* xyz, int64_t n, uint16_t* ids, void* hip_stream) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_get_blocks_gpu: tree is NULL");
    if (n < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_get_blocks_gpu: n must not be negative");
    if (n > 0 && (!xyz || !ids)) SVO_FAIL(SVO_EINVAL, "svo_tree_get_blocks_gpu: NULL xyz or ids");
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_get_blocks_gpu: tree not uploaded (svo_upload)");
    if (n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    const DevTree P{reinterpret_cast<const Node*>(t->d_nodes), reinterpret_cast<const uint16_t*>(t->d_mats), t->levels};
    const int64_t chunk = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        hipLaunchKernelGGL(k_get_blocks, lanes(std::min(chunk, n - i0)), dim3(256), 0, (hipStream_t)hip_stream, P, xyz, i0, std::min(n, i0 + chunk),
                           ids);
        HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    }
    return SVO_OK;
}
