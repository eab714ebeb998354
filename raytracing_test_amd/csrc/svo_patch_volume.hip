// svo_patch_volume.hip — svo_tree_patch_volume_gpu: the content of a resident tree inside a dense box of voxels in HBM is
// replaced by the box, on the device.  The result is the tree of the composite (the box inside, the old tree outside).  The
// descent, its kernels, its level loop and its commit are svo_patch_cells.h's, shared with the other patches; the question
// a cell asks is the box test, and inside the box the class pyramid of svo_build_volume_gpu over the box
// (svo_volume_pyramid.h; its level-1 pass reads the box once and checks the ids):
//   * a region the box does not meet is OUT: it keeps its record and its subtree;
//   * an aligned region wholly inside the box is emitted canonically from the box alone, by the plain emitter's rules:
//     EMPTY is IN with id 0 (the slot bit is cleared), an id is IN (a K_SOLID child), MIXED is FULL (it descends with
//     nothing of the old tree, and every cell below it is inside the box again);
//   * a region the box cuts is CUT.  A voxel of a cut brick is the box's (after the view filter) inside the box, else the
//     old tree's.
// The descent starts at the anchor the host finds on its image (svo_plan.cpp patch_anchor), whose record is the only one
// rewritten in place; the superseded records are counted by a host walk (patch_superseded).  A box that is the whole
// extent restarts the arrays: the first item is the root holding nothing, or the root is a lone record when the pyramid's
// top class is not MIXED.  Everything is written to scratch first: the totals are known, and every id checked, before the
// tree is touched.
// Every node and material index is widened to 64 bits before it addresses memory: trees above 2^28 nodes take the same
// kernels.
#include <hip/hip_runtime.h>
#include <string.h>

#include <chrono>
#include <new>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_patch_cells.h"
#include "svo_volume_pyramid.h"

using namespace svo;

namespace {

// the patch as svo_patch_cells.h's kernels ask it
struct DevBox {
    DevVolume V;           // the box and its pyramid
    const Node* nodes;     // the resident tree (read only: the patch is written to scratch)
    const uint16_t* mats;
    int32_t levels;
    int32_t b0[3], b1[3];  // the box, [b0, b1)
    uint64_t nbase;        // scratch record s >= 1 becomes node nbase + s - 1 of the tree
    using Item = ::Item;
    static constexpr bool kFull = true;
    __device__ uint32_t relation(int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) const {
        const int32_t c[3] = {x, y, z};
        bool out = false, in = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            out = out || c[a] + cs <= b0[a] || c[a] >= b1[a];
            in = in && c[a] >= b0[a] && c[a] + cs <= b1[a];
        }
        if (out || !in) return out ? SHAPE_OUT : SHAPE_CUT;
        *id = V.classify(x, y, z, cs, k);  // (G_EMPTY is id 0)
        return *id == G_MIXED ? SHAPE_FULL : SHAPE_IN;
    }
    __device__ bool voxel(int32_t x, int32_t y, int32_t z, uint32_t* id) const {
        const bool in = x >= b0[0] && x < b1[0] && y >= b0[1] && y < b1[1] && z >= b0[2] && z < b1[2];
        if (in) *id = V.voxel(x, y, z);  // (after the view filter)
        return in;
    }
};

}  // namespace

extern "C" int svo_tree_garbage(const svo_tree* t, uint64_t* nodes, uint64_t* mats) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_garbage: NULL tree");
    if (nodes) *nodes = t->garbage_nodes;
    if (mats) *mats = t->garbage_mats;
    return SVO_OK;
}

extern "C" int svo_tree_patch_volume_gpu(svo_tree* t, const svo_volume_box* box) {
    const char* who = "svo_tree_patch_volume_gpu";
    if (!t || !box) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: NULL argument");
    if (!box->voxels) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: NULL voxels");
    if (box->nx < 1 || box->ny < 1 || box->nz < 1) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: dimensions must be positive");
    const int32_t L = t->levels;
    const int64_t E = (int64_t)1 << (2 * L);
    const int32_t dims[3] = {box->nx, box->ny, box->nz};
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        if (box->origin[a] < 0 || (int64_t)box->origin[a] + dims[a] > E)
            SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: the box must lie within the extent (no wrap)");
        lo[a] = box->origin[a];
        hi[a] = box->origin[a] + dims[a];
    }
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_volume_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_volume_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    if (L < 2 || t->nodes.empty()) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: trees of fewer than 2 levels are not patched");
    if (t->palette.empty() || t->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: the palette must hold 1..65535 entries");

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // the box may come from any stream, and records and ceilings are rewritten in place below: every cast over the tree
    // must be over first (svo_tree_sync's contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    // the box as a volume of the tree's own palette and view, and its class pyramid: ids are checked here
    std::vector<svo_block> blocks;
    std::vector<Material> pal;
    try {
        for (const Material& m : t->palette) blocks.push_back(to_block(m));
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_volume_gpu: out of memory");
    }
    svo_volume_desc vd;
    memset(&vd, 0, sizeof(vd));
    vd.levels = L;
    vd.nx = box->nx;
    vd.ny = box->ny;
    vd.nz = box->nz;
    for (int a = 0; a < 3; a++) vd.origin[a] = box->origin[a];
    vd.voxels = box->voxels;
    vd.palette = blocks.data();
    vd.n_palette = (uint32_t)blocks.size();
    vd.view = t->view;
    vd.device = t->device;
    Pool pool;
    DevBox P;
    memset(&P, 0, sizeof(P));
    bool all = false, bad = false;
    uint16_t top = 0;
    int rc = prepare(&vd, pool, P.V, pal, all);
    if (!rc) rc = build_pyramid(P.V, L, all, pool, &bad, &top);
    if (rc) return rc;
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: a voxel id is not below the tree's palette size");

    PatchAnchor anchor = patch_anchor(t->nodes.data(), L, lo, hi);
    // a box that is the whole extent is a full build: the arrays restart behind the root and nothing is left superseded
    const uint64_t nbase = anchor.whole ? 1 : t->synced_nodes, mbase = anchor.whole ? 0 : t->synced_mats;
    uint64_t gnodes = 0, gmats = 0;
    if (!anchor.whole) patch_superseded(t->nodes.data(), L, anchor, lo, hi, &gnodes, &gmats);
    P.nodes = reinterpret_cast<const Node*>(t->d_nodes);
    P.mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    P.levels = L;
    for (int a = 0; a < 3; a++) {
        P.b0[a] = lo[a];
        P.b1[a] = hi[a];
    }
    P.nbase = nbase;
    std::vector<std::array<int64_t, 4>> rects;
    try {
        rects.push_back({lo[0], lo[2], hi[0], hi[2]});
        t->ceil_dirty.reserve(t->ceil_dirty.size() + 1);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_volume_gpu: out of memory");
    }

    if (anchor.whole) {  // the root, holding nothing
        anchor.kind = P_EMPTY;
        anchor.old = 0u;
    }
    // a root without children when the whole extent is one class
    const Node root = top == C_EMPTY ? Node{0ull, 0u, K_INTERIOR} : Node{~0ull, 0u, K_SOLID | ((uint32_t)top << 16)};
    ScanTmp tmp;
    CellsTail tail;
    rc = descend_cells(P, who, L, anchor.depth, anchor_item(anchor), anchor.whole && top != C_MIXED ? &root : nullptr, mbase, pool, tmp.v, &tail);
    if (rc) return rc;
    const auto clock1 = std::chrono::steady_clock::now();

    return commit_cells(t, who, tail, anchor, nbase, mbase, gnodes, gmats, rects, clock0, clock1);
}

extern "C" int svo_tree_patch_times(const svo_tree* t, double ms[3]) {
    if (!t || !ms) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_times: NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = t->patch_ms[i];
    return SVO_OK;
}
