// svo_shape_cell.h — the cell logic of svo_tree_patch_shapes_gpu (svo_patch_shapes.hip), shared by its kernels and the
// host (svo_plan.cpp: the garbage walk): no HIP, so it also builds with g++ and runs on a CPU
// (tests/sanitize/shapes_patch_plan_sanitize.cpp).  A patch is an ordered table of analytic shapes, each with the id it
// stores (0 erases); a voxel holds the id of the last shape that contains it.  How an aligned cell of cs^3 voxels stands to
// the table is answered in closed form, in exact integers, and both sides of the patch ask through these functions: the
// device pass decides from the answer what a child slot becomes, the host walk counts from it what the pass supersedes,
// and the two must agree on every cell.
// Not done here: a spatial index over the shapes.  Every cell scans the whole table, so a call costs (cells cut) x (shapes).
#pragma once

#include <stdint.h>

#include "svo_common.h"

namespace svo {

enum : int32_t { kShapeBox = 0, kShapeBall = 1 };  // SVO_SHAPE_BOX / SVO_SHAPE_BALL (include/svo_rt.h)

// A shape as the patch holds it, after the host's checks: the id already resolved against the tree's view.
//   box:  the voxels a <= p < b (b = one past the last voxel), inside the extent
//   ball: the voxels with |p - a|^2 <= r2, a the centre (anywhere within |a| <= 2^20), r2 <= 2^42; b is not read.
// With coordinates below 2^16 and these limits a squared distance stays below 2^43: every sum is exact in int64.
struct ShapeRec {
    int32_t kind;
    int32_t a[3];
    int32_t b[3];
    uint32_t id;  // what the shape's voxels store: 0 = nothing
    int64_t r2;
};
static_assert(sizeof(ShapeRec) == 40, "the shape table is read as 40-byte records");

// (SHAPE_FULL: the patch alone decides every voxel of the cell, and not uniformly.  No shape answers it: it is the volume
// patch's, whose box holds arbitrary voxels, to svo_patch_cells.h)
enum : uint32_t { SHAPE_OUT = 0u, SHAPE_IN = 1u, SHAPE_CUT = 2u, SHAPE_FULL = 3u };

// The cell [x, x + cs) x [y, y + cs) x [z, z + cs) against one shape: OUT when no voxel of the cell lies in the shape, IN
// when every voxel does, else CUT.  Box: the interval tests of the volume patch.  Ball: IN when the cell's farthest
// corner is within r2, OUT when its nearest voxel is beyond r2 (the nearest point of an integer box to an integer centre
// is a voxel, so CUT means exactly "some voxel in, some out").
SVO_HD uint32_t shape_relation(const ShapeRec& s, int32_t x, int32_t y, int32_t z, int32_t cs) {
    const int32_t c[3] = {x, y, z};
    if (s.kind == kShapeBox) {
        bool out = false, in = true;
        for (int a = 0; a < 3; a++) {
            out = out || c[a] + cs <= s.a[a] || c[a] >= s.b[a];
            in = in && c[a] >= s.a[a] && c[a] + cs <= s.b[a];
        }
        return out ? SHAPE_OUT : (in ? SHAPE_IN : SHAPE_CUT);
    }
    int64_t far = 0, near = 0;
    for (int a = 0; a < 3; a++) {
        const int64_t lo = (int64_t)c[a] - (int64_t)s.a[a], hi = lo + (int64_t)cs - 1;  // the cell's offsets from the centre
        const int64_t alo = lo < 0 ? -lo : lo, ahi = hi < 0 ? -hi : hi;
        const int64_t f = alo > ahi ? alo : ahi;
        const int64_t n = lo > 0 ? lo : (hi < 0 ? -hi : 0);
        far += f * f;
        near += n * n;
    }
    return near > s.r2 ? SHAPE_OUT : (far <= s.r2 ? SHAPE_IN : SHAPE_CUT);
}

// The cell against the whole table, scanned from the last shape to the first: the first shape that is not OUT decides.
// IN: the cell is uniformly *id.  CUT: descend.  OUT: no shape touches the cell, which keeps what the tree holds.
// The scan is conservative: a cell cut by a late shape but covered by an earlier one is CUT, and its bricks then come out
// uniform (the result is content, not canonical layout).  The loop runs over all n shapes whatever it finds, so that on
// the device its trip count, and with it every read of the table, is the same in all lanes.
SVO_HD uint32_t cell_relation(const ShapeRec* shapes, int32_t n, int32_t x, int32_t y, int32_t z, int32_t cs, uint32_t* id) {
    uint32_t rel = SHAPE_OUT, rid = 0u;
    for (int32_t i = n - 1; i >= 0; i--) {
        const ShapeRec s = shapes[i];
        const uint32_t r = shape_relation(s, x, y, z, cs);
        const bool take = rel == SHAPE_OUT && r != SHAPE_OUT;
        rid = take ? s.id : rid;
        rel = take ? r : rel;
    }
    *id = rid;
    return rel;
}

// one voxel: true when a shape contains it, *id then what the last such shape stores
SVO_HD bool shape_voxel(const ShapeRec* shapes, int32_t n, int32_t x, int32_t y, int32_t z, uint32_t* id) {
    return cell_relation(shapes, n, x, y, z, 1, id) != SHAPE_OUT;
}

}  // namespace svo
