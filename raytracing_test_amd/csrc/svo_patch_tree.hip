// svo_patch_tree.hip — svo_tree_patch_tree_gpu and svo_tree_patch_tree_oriented_gpu: a box of one resident tree (src) is
// pasted into another (dst), on the device, at an offset that is on no grid — and, by the second call, turned or mirrored
// by any of the 48 signed axis permutations, its ids through a table —, without expanding src's uniform regions: the cost
// follows the box's surface and the src records reached in it, never the volume.  The descent, its kernels, its level
// loop and its commit are svo_patch_cells.h's, shared with the other patches; the question a cell asks is svo_paste_cell.h's
// paste_relation: the aligned destination cell is clipped to the box, its ends are mapped into src (a shift; oriented: a
// per-axis affine map, under which an aligned cs^3 box is still a cs^3 box), and it is compared with the at most
// 2 x 2 x 2 aligned src cells it meets, each found by a walk from src's root (eight walks of at most 7 dependent loads
// per lane, the same trip count in every lane; with an id map one table load after each walk, in every lane too).  A cut
// brick's composite voxels come from src inside the box (where the mode lets them through) and from dst elsewhere.
// The two calls share everything but the record type the cell logic is instantiated over: PasteRec for the plain paste
// (identity orientation and map at compile time: its kernels carry neither), PasteTurn for the oriented one.
// Everything is read from the arrays as they were on entry and written to scratch first, so src == dst with overlapping
// boxes copies the old content; src is only ever read.  The descent starts at the anchor the host finds on dst's image
// (svo_plan.cpp patch_anchor over the destination box), whose record is the only one rewritten in place; a REPLACE paste
// over the whole extent restarts the arrays (the volume patch's rule).  The superseded records are counted by a host walk
// (svo_plan.cpp paste_superseded) that asks the same paste_relation about the same cells over the two host images.
// svo_tree_patch_tree_rule_gpu is the oriented paste under a rule that also asks what dst holds (svo_paste_cell.h PasteRule,
// rule_relation, rule_takes): a ninth walk per cell, over dst's own arrays at the cell's depth, and per voxel of a cut brick
// a second lookup, in dst.  The arrays it reads are dst's as they were on entry, since the patch is written to scratch.  It
// never restarts the arrays.  Its kernels are four more instances of svo_patch_cells.h's (DevPasteRule); the other
// instances do not change.
// Every node and material index is widened to 64 bits before it addresses memory.
#include <hip/hip_runtime.h>

#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_paste_cell.h"
#include "svo_patch_cells.h"

using namespace svo;

namespace {

// the patch as svo_patch_cells.h's kernels ask it, over the record type of the cell logic
template <class Rec>
struct DevPasteOf {
    Rec rec;  // (in_view, id_map: the tables in HBM, or NULL); the cell and the voxel ask through relation_of / takes_of
    PasteTree src;
    const Node* nodes;  // dst (read only: the patch is written to scratch)
    const uint16_t* mats;
    int32_t levels;
    uint64_t nbase;  // scratch record s >= 1 becomes node nbase + s - 1 of dst
    using Item = ::Item;
    static constexpr bool kFull = false;
    __device__ uint32_t relation(int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) const {
        return relation_of(rec, src, x, y, z, cs, k, id);
    }
    __device__ bool voxel(int32_t x, int32_t y, int32_t z, uint32_t* id) const { return takes_of(rec, src, x, y, z, id); }
};
struct DevPaste : DevPasteOf<PasteRec> {};      // svo_tree_patch_tree_gpu
struct DevPasteTurn : DevPasteOf<PasteTurn> {};  // svo_tree_patch_tree_oriented_gpu
struct DevPasteRule : DevPasteOf<PasteRule> {};  // svo_tree_patch_tree_rule_gpu (rec.dst: dst's arrays in HBM, as nodes and mats)

// dst's arrays into the record, where the cell logic reads them
void set_dst(PasteRec&, const PasteTree&) {}
void set_dst(PasteRule& rec, const PasteTree& dst) { rec.dst = dst; }

// the id map (a host array of n entries) to the device, where the record has one
int upload_id_map(Pool&, PasteRec&, size_t) { return SVO_OK; }
int upload_id_map(Pool& pool, PasteTurn& rec, size_t n) {
    if (!rec.id_map) return SVO_OK;
    uint16_t* dmap;
    const int rc = pool.alloc(&dmap, n);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dmap, rec.id_map, n * sizeof(uint16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    rec.id_map = dmap;
    return SVO_OK;
}

// The checks on the trees, after the arguments' and before the first HIP call.  id_map: the oriented call's table (its
// entries are then the range check), or NULL: ids are numbers in dst's palette
int paste_check_trees(const svo_tree* dst, const svo_tree* src, const std::string& who, const uint16_t* id_map) {
    if (dst->levels < 2 || dst->nodes.empty()) SVO_FAIL(SVO_ERANGE, who + ": trees of fewer than 2 levels are not patched");
    if (src->levels < 1 || src->nodes.empty()) SVO_FAIL(SVO_ERANGE, who + ": src holds no tree");
    if (dst->palette.empty() || dst->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, who + ": the palette must hold 1..65535 entries");
    if (id_map) {
        for (size_t i = 0; i < src->palette.size(); i++)
            if (id_map[i] >= dst->palette.size())
                SVO_FAIL(SVO_ERANGE, who + ": id_map[" + std::to_string(i) + "] = " + std::to_string(id_map[i]) + " is not an id of dst's palette (" +
                                         std::to_string(dst->palette.size()) + " entries)");
    } else if (src->palette.size() > dst->palette.size()) {
        SVO_FAIL(SVO_ERANGE, who + ": src's palette holds more entries than dst's (ids are numbers in dst's palette)");
    }
    if (dst->device < 0 || !dst->d_nodes) SVO_FAIL(SVO_ESTATE, who + ": tree dst not uploaded (svo_upload)");
    if (src->device < 0 || !src->d_nodes) SVO_FAIL(SVO_ESTATE, who + ": tree src not uploaded (svo_upload)");
    if (src->device != dst->device) SVO_FAIL(SVO_ESTATE, who + ": the trees are on different devices");
    if (tree_unsynced(dst)) SVO_FAIL(SVO_ESTATE, who + ": dst has host edits not yet synced (svo_tree_sync)");
    if (tree_unsynced(src)) SVO_FAIL(SVO_ESTATE, who + ": src has host edits not yet synced (svo_tree_sync)");
    return SVO_OK;
}

// The paste itself, the same for both calls.  rec: the plan's record (in_view NULL; id_map the host array or NULL)
template <class Dev, class Rec>
int paste_run(svo_tree* dst, const svo_tree* src, const char* who, const Rec& rec, bool whole) {
    const int32_t L = dst->levels;
    // the view table, the anchor and the superseded records: host work on the two images, before the first HIP call
    std::vector<uint32_t> bits;
    std::vector<std::array<int64_t, 4>> rects;
    PatchAnchor anchor;
    uint64_t gnodes = 0, gmats = 0;
    bool all = true;
    try {
        all = paste_view_bits(dst->palette, dst->view, &bits);
        rects.push_back({rec.lo[0], rec.lo[2], rec.hi[0], rec.hi[2]});
        dst->ceil_dirty.reserve(dst->ceil_dirty.size() + 1);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, std::string(who) + ": out of host memory");
    }
    anchor = patch_anchor(dst->nodes.data(), L, rec.lo, rec.hi);
    anchor.whole = whole;  // (a KEEP_EMPTY paste over the whole extent stays at the root and restarts nothing)

    HIP_TRY(hipSetDevice(dst->device), SVO_EDEVICE);
    // records and ceilings are rewritten in place below: every cast over the tree must be over first (svo_tree_sync's
    // contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    const uint64_t nbase = whole ? 1 : dst->synced_nodes, mbase = whole ? 0 : dst->synced_mats;
    if (!whole) {
        Rec hrec = rec;
        hrec.in_view = all ? nullptr : bits.data();
        set_dst(hrec, PasteTree{dst->nodes.data(), dst->mats.data(), L});
        paste_superseded(dst->nodes.data(), L, anchor, hrec, PasteTree{src->nodes.data(), src->mats.data(), src->levels}, &gnodes, &gmats);
    }

    Pool pool;
    int rc = SVO_OK;
    Dev P{{rec,
           PasteTree{reinterpret_cast<const Node*>(src->d_nodes), reinterpret_cast<const uint16_t*>(src->d_mats), src->levels},
           reinterpret_cast<const Node*>(dst->d_nodes),
           reinterpret_cast<const uint16_t*>(dst->d_mats),
           L,
           nbase}};
    set_dst(P.rec, PasteTree{P.nodes, P.mats, L});
    if (!all) {
        uint32_t* dbits;
        rc = pool.alloc(&dbits, bits.size());
        if (rc) return rc;
        HIP_TRY(hipMemcpy(dbits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice), SVO_EDEVICE);
        P.rec.in_view = dbits;
    }
    rc = upload_id_map(pool, P.rec, src->palette.size());
    if (rc) return rc;

    ScanTmp tmp;
    CellsTail tail;
    rc = descend_cells(P, who, L, anchor.depth, anchor_item(anchor), nullptr, mbase, pool, tmp.v, &tail);
    if (rc) return rc;
    const auto clock1 = std::chrono::steady_clock::now();
    return commit_cells(dst, who, tail, anchor, nbase, mbase, gnodes, gmats, rects, clock0, clock1);
}

}  // namespace

extern "C" int svo_tree_patch_tree_gpu(svo_tree* dst, const svo_tree* src, const int32_t src_origin[3], int32_t nx, int32_t ny, int32_t nz,
                                       const int32_t dst_origin[3], uint32_t flags) {
    const char* who = "svo_tree_patch_tree_gpu";
    if (!dst || !src) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: NULL tree");
    if (!dst_origin) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: NULL dst_origin");
    PastePlan plan;
    switch (paste_plan(dst->levels, src->levels, src_origin, nx, ny, nz, dst_origin, flags, &plan)) {
        case PASTE_FLAGS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: unknown flag bits");
        case PASTE_DIM: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: the box's dimensions must be positive");
        case PASTE_SRC_EXTENT: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: the source box must lie within src's extent (no wrap)");
        case PASTE_DST_EXTENT: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_gpu: the destination box must lie within dst's extent (no wrap)");
        default: break;
    }
    const int rc = paste_check_trees(dst, src, who, nullptr);
    if (rc) return rc;
    return paste_run<DevPaste, PasteRec>(dst, src, who, plan.rec, plan.whole);
}

extern "C" int svo_tree_patch_tree_oriented_gpu(svo_tree* dst, const svo_tree* src, const svo_paste* p) {
    const char* who = "svo_tree_patch_tree_oriented_gpu";
    if (!dst || !src) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: NULL tree");
    if (!p) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: NULL svo_paste");
    PastePlan plan;
    switch (paste_plan(dst->levels, src->levels, p->src_origin, p->n[0], p->n[1], p->n[2], p->dst_origin, p->flags, &plan, p->axis, p->flip)) {
        case PASTE_FLAGS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: unknown flag bits");
        case PASTE_AXIS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: axis must be a permutation of 0, 1, 2");
        case PASTE_FLIP: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: flip entries must be 0 or 1");
        case PASTE_DIM: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: the box's dimensions must be positive");
        case PASTE_SRC_EXTENT: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: the source box must lie within src's extent (no wrap)");
        case PASTE_DST_EXTENT:
            SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: the destination box (the dimensions permuted by axis) must lie within dst's extent (no wrap)");
        default: break;
    }
    if (p->id_map && !src->palette.empty() && p->id_map[0] != 0) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_oriented_gpu: id_map[0] must be 0");
    const int rc = paste_check_trees(dst, src, who, p->id_map);
    if (rc) return rc;
    plan.rec.id_map = p->id_map;
    return paste_run<DevPasteTurn, PasteTurn>(dst, src, who, plan.rec, plan.whole);
}

extern "C" int svo_tree_patch_tree_rule_gpu(svo_tree* dst, const svo_tree* src, const svo_paste* p, uint32_t rule) {
    const char* who = "svo_tree_patch_tree_rule_gpu";
    if (!dst || !src) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: NULL tree");
    if (!p) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: NULL svo_paste");
    switch (paste_rule_check(p->flags, rule)) {
        case RULE_FLAGS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: svo_paste's flags must be 0 (the rule replaces them)");
        case RULE_BITS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: unknown rule bits (a rule is SVO_RULE(a, b, c), below 64)");
        case RULE_SRC_ONLY: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the rule's src-only case must be SVO_RULE_KEEP or SVO_RULE_TAKE");
        case RULE_BOTH: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the rule's both case must be SVO_RULE_KEEP, SVO_RULE_TAKE or SVO_RULE_CLEAR");
        case RULE_DST_ONLY: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the rule's dst-only case must be SVO_RULE_KEEP or SVO_RULE_CLEAR");
        default: break;
    }
    PastePlan plan;
    switch (paste_plan(dst->levels, src->levels, p->src_origin, p->n[0], p->n[1], p->n[2], p->dst_origin, 0u, &plan, p->axis, p->flip)) {
        case PASTE_AXIS: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: axis must be a permutation of 0, 1, 2");
        case PASTE_FLIP: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: flip entries must be 0 or 1");
        case PASTE_DIM: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the box's dimensions must be positive");
        case PASTE_SRC_EXTENT: SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the source box must lie within src's extent (no wrap)");
        case PASTE_DST_EXTENT:
            SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: the destination box (the dimensions permuted by axis) must lie within dst's extent (no wrap)");
        default: break;
    }
    if (p->id_map && !src->palette.empty() && p->id_map[0] != 0) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_tree_rule_gpu: id_map[0] must be 0");
    const int rc = paste_check_trees(dst, src, who, p->id_map);
    if (rc) return rc;
    if (rule == 0u) return SVO_OK;  // every case keeps: nothing to do
    PasteRule rec;
    static_cast<PasteTurn&>(rec) = plan.rec;
    rec.id_map = p->id_map;
    rec.keep_empty = 0u;
    rec.rule = rule;
    rec.dst = PasteTree{nullptr, nullptr, dst->levels};
    return paste_run<DevPasteRule, PasteRule>(dst, src, who, rec, false);  // (never a restart: svo_tree_compact_gpu exists)
}
