// svo_plan.h — the host arithmetic behind a launch and behind device residency: no HIP, so it also builds with g++
// and runs on a CPU (tests/sanitize/host_sanitize.cpp).  The HIP translation units act on its results.
#pragma once

#include <utility>

#include "svo_internal.h"
#include "svo_list_unrank.h"
#include "svo_paste_cell.h"
#include "svo_shape_cell.h"

namespace svo {

// The AO plan of (n samples, `steps`) as the image ao_count_plan reads (svo_shade.h); empty: no plan for them
std::vector<uint32_t> ao_plan_image(int32_t n, int32_t steps, const float* tab);

int frame_dirs(const RayGen& rg, int32_t width, int32_t height, int32_t flags);
bool need_seg(int32_t flags, bool explicit_rays, int32_t steps, const float* org, int32_t n_org);
void frame_axes(int dirs, const float org[3], double frac[3], int32_t cell[3]);

// Which k_cast instance a launch runs: the one place that decides it.  Almost every instance gives identical results, so
// a wrong pick would only be slower: tests/sanitize/host_sanitize.cpp holds the rule as a table, over every request.
struct CastRequest {
    bool stats, timeline;  // SVO_CAST_STATS, SVO_CAST_TIMELINE
    bool ao;               // the launch casts AO rays
    bool shade;            // the shading pass
    bool records;          // (shading) hit records are output
    bool wide;             // 64-bit node addresses (shading: either tree's)
    bool seg;              // need_seg
    int dirs;              // frame_dirs (0: no common octant; the pick ray: 0)
};
struct CastInstance {  // k_cast's template arguments, in their order (svo_cast_instances.h)
    bool stats, stamps, ao, shade, wide, seg;
    int dirs;
    bool norec;
};
CastInstance cast_instance(const CastRequest& q);

// The host copies of the ceiling tables (svo_tree.ceil_host / ceilp_host / ceilq_host, ceil_off): rebuilt whole from the
// tree (returns the number of levels), or brought up to date over one rectangle of svo_tree.ceil_dirty, which returns the
// rows rewritten, first and one past the last: zr per level of the ceilings and pairs, qr of the quads.  Both may throw
// std::bad_alloc.
int32_t ceil_tables_build(svo_tree* t);
void ceil_tables_update(svo_tree* t, int32_t n, const std::array<int64_t, 4>& r, int64_t zr[kCeilMax][2], int64_t qr[2]);
// The same over every rectangle of svo_tree.ceil_dirty at once (sync_ceilings), with the same tables as one call of
// ceil_tables_update per rectangle, in order, leaves.  The rows rewritten come back as sorted, disjoint intervals
// [first, last): one rectangle gives the one interval per table ceil_tables_update reports.  The rectangles of a list of
// scattered edits (svo_tree_patch_points_gpu) share their coarsest blocks: the quads of each distinct span of those are
// recomputed once, after every rectangle's ceilings are final, and rows that several rectangles rewrite are sent once.
struct CeilRows {
    std::vector<std::pair<int64_t, int64_t>> level[kCeilMax], quads;
};
void ceil_tables_update_all(svo_tree* t, int32_t n, const std::vector<std::array<int64_t, 4>>& rects, CeilRows* rows);
// The fine ceilings (svo_tree.ceil_fine_host) are kept by the same three calls.  Their rows rewritten lie within the level-0
// rows reported (a rectangle is widened to level-0 blocks, the pairs' rows to their partner level's): the elements of the
// fine table, first and count, that an interval [first, last) of level-0 rows covers.
struct CeilFineSpan {
    int64_t first, count;
};
// whether a launch whose first ceiling level is `first_level` of the table, with `launch_levels` levels in use, marches on
// the fine ceilings: they lie one level below the table's finest, so only a launch that starts there descends onto them
bool ceil_fine_for(int32_t launch_levels, int32_t first_level);
// The levels of the table coarser than a launch's first level that its march walks before it (CastParams::march_sh,
// svo_ceil_march.h), coarsest first: levels first_level + 1 .. first_level + kMarchCoarseMax of the `ceil_levels` the table
// has, each 4 times as wide as the next, and only levels with at least 2 x 2 blocks in a tree of `levels` levels (a single
// block says nothing a wrap does not repeat).  None (n 0) for a table that does not reach the launch's first level.
constexpr int32_t kMarchCoarseMax = 2;  // 64- and 256-column blocks above a first level of 16
struct MarchLevels {
    int32_t n;
    int32_t level[kMarchCoarseMax];  // levels of the table
};
MarchLevels march_levels(int32_t ceil_levels, int32_t first_level, int32_t levels);
// ... as a launch takes them over tree t (CastParams::march_n, march_sh, march_off): log2 of each level's block width and its
// first element in the tree's table (svo_tree.ceil_off); none for a launch that uses no level of it (launch_levels 0)
struct MarchParams {
    int32_t n;
    uint32_t sh[kMarchCoarseMax];
    int64_t off[kMarchCoarseMax];
};
MarchParams march_params(const svo_tree* t, int32_t launch_levels, int32_t first_level);
CeilFineSpan ceil_fine_span(const svo_tree* t, const std::pair<int64_t, int64_t>& level0_rows);

// the tree's rewritten records (svo_tree.dirty_nodes, sorted here) as runs [first, last] of consecutive indices
std::vector<std::pair<uint32_t, uint32_t>> dirty_runs(std::vector<uint32_t>& dirty);
// the host image holds something its copy in HBM does not (svo_tree_sync would move data)
bool tree_unsynced(const svo_tree* t);

// svo_tree_patch_volume_gpu (svo_patch_volume.hip) replaces the content of the box [lo, hi) of a resident tree.  What a
// region held before the patch, as the work items of every patch's descent carry it (svo_patch_cells.h):
enum : uint32_t {
    P_NODE = 1u,    // the record nodes[old] (INTERIOR above the brick level, BRICK at it)
    P_UNIFORM = 2u,  // material `old` throughout (a K_SOLID record, or a region below one)
    P_EMPTY = 3u,    // nothing stored (a clear slot bit, or a region below one)
};
// Where the patch starts, as svo_tree_update's walk: down from the root while the box lies inside one child region without
// filling it and that child's record is K_INTERIOR.  The node reached is the anchor, the only record rewritten in place;
// every child of it that the box meets is cut by the box or wholly inside it.  A root that is a lone K_SOLID record is the
// anchor itself (kind P_UNIFORM: it becomes interior).  whole: the box is the whole extent, and the root itself is replaced.
struct PatchAnchor {
    uint32_t node;   // index of the anchor's record
    int32_t depth;   // its depth: the region is 4^(levels - depth) voxels wide
    int32_t o[3];    // the region's first voxel
    uint32_t kind;   // P_NODE, or P_UNIFORM for a lone K_SOLID root
    uint32_t old;    // the material of P_UNIFORM (P_NODE: node)
    bool whole;
};
PatchAnchor patch_anchor(const Node* nodes, int32_t levels, const int32_t lo[3], const int32_t hi[3]);
// the node records and material entries the patch supersedes below the anchor: the child block of every interior node the
// box cuts (it is rewritten at the tail), every subtree wholly inside the box, the material run of every brick the box meets
void patch_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const int32_t lo[3], const int32_t hi[3], uint64_t* n_nodes,
                      uint64_t* n_mats);

// svo_tree_patch_points_gpu (svo_patch_points.hip) applies a sorted list of edits, each a voxel's cell key (6 bits per
// level, the slot bits z<<4 | y<<2 | x with the top level first).  Its anchor is the deepest K_INTERIOR record, at depth
// <= levels - 2, whose region holds every edit: down from the root along the 6-bit digits the list's first and last key
// have in common, stopping as patch_anchor does at an absent slot, at a K_SOLID or K_BRICK child, and at a lone K_SOLID
// root (kind P_UNIFORM).  It is never whole: a list does not restart the arrays.
PatchAnchor points_anchor(const Node* nodes, int32_t levels, uint64_t key_first, uint64_t key_last);
// The 16 x 16-column blocks a list of edits touches, each as (bz << 32) | bx in block units (any order, duplicates allowed),
// merged into column rectangles {x0, z0, x1, z1} in voxels for svo_tree.ceil_dirty: runs of adjacent blocks within a block
// row, and runs of equal span in consecutive rows joined into one rectangle.  `blocks` is sorted in place.
std::vector<std::array<int64_t, 4>> ceil_block_rects(std::vector<uint64_t>& blocks);

// svo_tree_patch_shapes_gpu (svo_patch_shapes.hip) applies an ordered list of boxes and balls.  The host's part of it:
// every shape checked (the first one that fails decides, *bad = its index), its id resolved against the tree's view
// (an id the view does not hold is stored as 0) and its bounding box clipped to the extent 4^levels.  A shape whose
// clipped box is empty is dropped; the others make up the table the cells are asked against (svo_shape_cell.h), one
// column rectangle {x0, z0, x1, z1} each for svo_tree.ceil_dirty, and the union [lo, hi) of their boxes.
enum : int {
    SHAPES_OK = 0,
    SHAPES_KIND = 1,        // an unknown kind
    SHAPES_BOX_DIM = 2,     // a box with a non-positive dimension
    SHAPES_BOX_EXTENT = 3,  // a box that leaves the extent
    SHAPES_R2_NEG = 4,      // r2 < 0
    SHAPES_CENTRE = 5,      // a ball centre beyond 2^20
    SHAPES_R2_BIG = 6,      // r2 > 2^42
    SHAPES_ID = 7,          // an id at or beyond the palette size
};
constexpr int32_t kShapesMax = 1024, kShapeCentreMax = 1 << 20;
constexpr int64_t kShapeR2Max = (int64_t)1 << 42;
struct ShapesPlan {
    std::vector<ShapeRec> table;
    std::vector<std::array<int64_t, 4>> rects;
    int32_t lo[3], hi[3];
};
int shapes_plan(int32_t levels, int32_t view, const std::vector<Material>& palette, const svo_shape* shapes, int32_t n, ShapesPlan* plan,
                int32_t* bad);
// the analogue of patch_superseded: the node records and material entries the shapes patch supersedes below the anchor,
// by the device pass's own rule — the child block of the anchor and of every interior node whose cell cell_relation calls
// CUT, every subtree whose cell it calls IN, the material run of every brick whose cell is IN or CUT
void shapes_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const ShapeRec* shapes, int32_t n, uint64_t* n_nodes,
                       uint64_t* n_mats);

// svo_tree_patch_tree_gpu (svo_patch_tree.hip) pastes a box of one resident tree into another.  The host's part of it: the
// flags and the two boxes checked (src_origin == NULL: src's whole extent, the dimensions then ignored; otherwise the list
// box's rule for src, and the same box moved to dst_origin inside dst's extent, the sums taken in 64 bits), the paste as
// the cells are asked against it (svo_paste_cell.h; in_view is left NULL for the caller to set), and whether it restarts
// the arrays: a REPLACE paste whose destination box is the whole extent.
// svo_tree_patch_tree_oriented_gpu adds the orientation (svo_paste's axis and flip; NULL: the identity): checked after the
// flags and before the boxes, it gives the destination box its dimensions dn[a] = n[axis[a]] and the record its affine
// map, s[axis[a]] = sign[a] * q[a] + shift[a] with shift[a] = src_origin[axis[a]] - dst_origin[a], or under a flip
// src_origin[axis[a]] + n[axis[a]] - 1 + dst_origin[a].  rec.id_map is left NULL for the caller to set.  Sliced to its
// PasteRec, the record of an identity plan is the plain paste's.
enum : int {
    PASTE_OK = 0,
    PASTE_FLAGS = 1,       // an unknown flag bit
    PASTE_DIM = 2,         // a non-positive dimension
    PASTE_SRC_EXTENT = 3,  // the source box leaves src's extent
    PASTE_DST_EXTENT = 4,  // the destination box leaves dst's extent
    PASTE_AXIS = 5,        // axis is not a permutation of 0, 1, 2
    PASTE_FLIP = 6,        // a flip entry other than 0 or 1
};
struct PastePlan {
    PasteTurn rec;
    bool whole;
};
int paste_plan(int32_t dst_levels, int32_t src_levels, const int32_t* src_origin, int32_t nx, int32_t ny, int32_t nz, const int32_t dst_origin[3],
               uint32_t flags, PastePlan* plan, const uint8_t* axis = nullptr, const uint8_t* flip = nullptr);
// svo_tree_patch_tree_rule_gpu (svo_patch_tree.hip) is the oriented paste under a rule over both sides (svo_paste_cell.h
// PasteRule).  Its geometry is paste_plan's with flags 0; the rule has a check and statuses of its own, in the order of
// the list: svo_paste's flags must be 0 (the rule replaces them), no bit above 5, A is KEEP or TAKE, B any of the three,
// C is KEEP or CLEAR
enum : int {
    RULE_OK = 0,
    RULE_FLAGS = 1,     // svo_paste.flags is not 0
    RULE_BITS = 2,      // a bit above 5
    RULE_SRC_ONLY = 3,  // A is CLEAR or 3
    RULE_BOTH = 4,      // B is 3
    RULE_DST_ONLY = 5,  // C is TAKE or 3
};
int paste_rule_check(uint32_t flags, uint32_t rule);
// the in-view bit table of a palette under `view` (bit id: the view stores the id; bit 0 is set: id 0 stays 0); returns
// true when every id is in view
bool paste_view_bits(const std::vector<Material>& palette, int32_t view, std::vector<uint32_t>* bits);
// shapes_superseded's walk over dst's host image with paste_relation asked over src's host image: what the paste
// supersedes below the anchor, by the device pass's own rule
void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteRec& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats);
void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteTurn& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats);
// the same walk with rule_relation asked (rec.dst: dst's host image, the array `nodes` belongs to)
void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteRule& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats);

// svo_tree_list_voxels_gpu (svo_list_voxels.hip) lists the voxels inside a box of the extent 4^levels: origin == NULL is the
// whole extent (the dimensions are then ignored), otherwise origin >= 0, origin + n <= extent and positive dimensions, with
// no wrap (the patch box's rule; the sums are taken in 64 bits).  Fills *B; LIST_BOX_DIM: a non-positive dimension;
// LIST_BOX_EXTENT: the box leaves the extent.
enum : int { LIST_BOX_OK = 0, LIST_BOX_DIM = 1, LIST_BOX_EXTENT = 2 };
int list_box(int32_t levels, const int32_t* origin, int32_t nx, int32_t ny, int32_t nz, ListBox* B);

// A schedule predicts a frame from the last one: a camera that turned more than kSchedTurn or moved more than kSchedMove
// voxels since runs the default order (and re-primes).  Measured (tools/shade_motion.py, r04_ax): a still view 0.462 ->
// 0.368 ms; 0.25 deg + 0.14 voxels per frame 0.400 -> 0.395; 2 deg per frame 0.292 -> 0.374 and a cut every frame
// 0.308 -> 0.358 when a stale order was used — a wrong order is worse than the default one.  A frame far from the last
// one is not sorted after either (the sort costs ~9 us): the schedule comes back one frame after the camera settles.
constexpr float kSchedTurnCos = 0.99996f;  // cos(0.5 deg)
// A still camera's order holds for the next frames too: a scheduled frame writes its durations and is sorted after only
// every kSchedEvery-th frame (the sort, one workgroup for ~9 us between two launches, is otherwise on every frame's path)
constexpr int32_t kSchedEvery = 4;
constexpr float kSchedMove = 1.0f;
struct SchedPlan {
    bool use_order;   // dispatch in the stored order
    bool write_cost;  // the blocks write their durations
    bool sort;        // the durations are sorted into the next order after the launch (sched_order, which primes)
};
// this frame's use of schedule s (its buffer already holds `blocks` blocks), and s moved on to it
SchedPlan sched_decide(svo_tree::Sched& s, int64_t blocks, const int64_t sig[7], const float cam[6]);

}  // namespace svo
