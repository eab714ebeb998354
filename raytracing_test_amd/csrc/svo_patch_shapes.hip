// svo_patch_shapes.hip — svo_tree_patch_shapes_gpu: a resident tree is changed, on the device, by an ordered list of solid
// shapes (boxes and balls, each with the id it stores; id 0 erases).  A voxel ends up with the id of the last shape that
// contains it; the cost follows the shapes' surfaces, never their volumes.  The descent, its kernels, its level loop and
// its commit are svo_patch_cells.h's, shared with the other patches; the question a cell asks is a closed form
// (svo_shape_cell.h cell_relation, asked per cell over the whole table): a cell no shape touches is OUT, a
// cell wholly inside the deciding shape IN, a cell the deciding shape cuts CUT.  The table sits in HBM and is indexed by
// the loop counter alone, the same in every lane; it is not copied per lane.
// The descent starts at the anchor the host finds on its image (svo_plan.cpp patch_anchor over the union of the shapes'
// clipped bounding boxes), whose record is the only one rewritten in place.  A bounding box equal to the extent does not
// restart the arrays: they restart only when cell_relation calls the whole extent IN.  The superseded records are counted
// by a host walk (svo_plan.cpp shapes_superseded) that asks the same cell_relation about the same cells.  Everything is
// written to scratch first, and committed through svo_patch_commit.h as the other patches are.
// Every node and material index is widened to 64 bits before it addresses memory.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_patch_cells.h"

using namespace svo;

static_assert(kShapeBox == SVO_SHAPE_BOX && kShapeBall == SVO_SHAPE_BALL, "svo_shape_cell.h's kinds are the ABI's");

namespace {

// the patch as svo_patch_cells.h's kernels ask it
struct DevShapes {
    const ShapeRec* shapes;  // the table, in list order
    int32_t n;
    const Node* nodes;       // the resident tree (read only: the patch is written to scratch)
    const uint16_t* mats;
    int32_t levels;
    uint64_t nbase;          // scratch record s >= 1 becomes node nbase + s - 1 of the tree
    using Item = ::Item;
    static constexpr bool kFull = false;
    __device__ uint32_t relation(int32_t x, int32_t y, int32_t z, int32_t cs, int, uint32_t* id) const {
        return cell_relation(shapes, n, x, y, z, cs, id);
    }
    __device__ bool voxel(int32_t x, int32_t y, int32_t z, uint32_t* id) const { return shape_voxel(shapes, n, x, y, z, id); }
};

}  // namespace

extern "C" int svo_tree_patch_shapes_gpu(svo_tree* t, const svo_shape* shapes, int32_t n) {
    const char* who = "svo_tree_patch_shapes_gpu";
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: NULL tree");
    if (n < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: n must not be negative");
    if (n > 0 && !shapes) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: NULL shapes");
    if (n > kShapesMax) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: n must not exceed 1024");
    const int32_t L = t->levels;
    if (L < 2 || t->nodes.empty()) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: trees of fewer than 2 levels are not patched");
    if (t->palette.empty() || t->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: the palette must hold 1..65535 entries");
    ShapesPlan plan;
    int32_t bad = -1;
    int why = SHAPES_OK;
    try {
        why = shapes_plan(L, t->view, t->palette, shapes, n, &plan, &bad);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_shapes_gpu: out of memory");
    }
    if (why != SHAPES_OK) {
        const std::string at = std::string(who) + ": shape " + std::to_string(bad) + ": ";
        switch (why) {
            case SHAPES_KIND: SVO_FAIL(SVO_EINVAL, at + "unknown kind");
            case SHAPES_BOX_DIM: SVO_FAIL(SVO_EINVAL, at + "a box's dimensions must be positive");
            case SHAPES_BOX_EXTENT: SVO_FAIL(SVO_EINVAL, at + "a box must lie within the extent (no wrap)");
            case SHAPES_R2_NEG: SVO_FAIL(SVO_EINVAL, at + "r2 must not be negative");
            case SHAPES_CENTRE: SVO_FAIL(SVO_ERANGE, at + "a ball's centre must lie within 2^20 of the origin on every axis");
            case SHAPES_R2_BIG: SVO_FAIL(SVO_ERANGE, at + "r2 must not exceed 2^42");
            default: SVO_FAIL(SVO_ERANGE, at + "the id is not below the tree's palette size");
        }
    }
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_shapes_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_shapes_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    const int32_t ns = (int32_t)plan.table.size();
    if (ns == 0) return SVO_OK;  // no shape, or every one clipped away

    // the anchor, the restart and the superseded records: host work on the image, before the first HIP call
    uint32_t top_id = 0;
    const bool whole = cell_relation(plan.table.data(), ns, 0, 0, 0, 1 << (2 * L), &top_id) == SHAPE_IN;
    PatchAnchor anchor = patch_anchor(t->nodes.data(), L, plan.lo, plan.hi);
    anchor.whole = whole;  // (patch_anchor's own `whole`, a bounding box equal to the extent, only keeps the anchor at the root)

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // records and ceilings are rewritten in place below: every cast over the tree must be over first (svo_tree_sync's
    // contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    const uint64_t nbase = whole ? 1 : t->synced_nodes, mbase = whole ? 0 : t->synced_mats;
    uint64_t gnodes = 0, gmats = 0;
    if (!whole) shapes_superseded(t->nodes.data(), L, anchor, plan.table.data(), ns, &gnodes, &gmats);
    try {
        t->ceil_dirty.reserve(t->ceil_dirty.size() + plan.rects.size());
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_shapes_gpu: out of host memory");
    }

    Pool pool;
    ShapeRec* dshapes;
    int rc = pool.alloc(&dshapes, (size_t)ns);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dshapes, plan.table.data(), (size_t)ns * sizeof(ShapeRec), hipMemcpyHostToDevice), SVO_EDEVICE);
    const DevShapes P{dshapes, ns, reinterpret_cast<const Node*>(t->d_nodes), reinterpret_cast<const uint16_t*>(t->d_mats), L, nbase};

    ScanTmp tmp;
    // a root without children when the whole extent is IN
    const Node root = top_id == 0 ? Node{0ull, 0u, K_INTERIOR} : Node{~0ull, 0u, K_SOLID | (top_id << 16)};
    CellsTail tail;
    rc = descend_cells(P, who, L, anchor.depth, anchor_item(anchor), whole ? &root : nullptr, mbase, pool, tmp.v, &tail);
    if (rc) return rc;
    const auto clock1 = std::chrono::steady_clock::now();

    return commit_cells(t, who, tail, anchor, nbase, mbase, gnodes, gmats, plan.rects, clock0, clock1);
}
