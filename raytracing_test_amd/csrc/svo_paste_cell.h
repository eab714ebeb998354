// svo_paste_cell.h — the cell logic of svo_tree_patch_tree_gpu and svo_tree_patch_tree_oriented_gpu (svo_patch_tree.hip),
// shared by their kernels and the host (svo_plan.cpp: the garbage walk): no HIP, so it also builds with g++ and runs on a
// CPU (tests/sanitize/paste_tree_plan_sanitize.cpp, paste_oriented_plan_sanitize.cpp).  A paste copies the box [lo, hi) of
// the destination's extent from a source tree, read at the destination's position plus `shift` (src_origin - dst_origin,
// on no grid) or, oriented, through a per-axis affine map (PasteTurn), its ids through a table.  How an aligned
// destination cell of cs^3 voxels stands to the source is answered from the source's records, without expanding a
// uniform region, and both sides of the patch ask through these functions: the device pass decides from the answer what a
// child slot becomes, the host walk counts from it what the pass supersedes, and the two must agree on every cell.
// The functions are written once, over the record type: PasteRec is the identity orientation and the identity map at
// compile time (the plain paste's kernels carry neither), PasteTurn the general case.
// svo_tree_patch_tree_rule_gpu's cell logic is at the end: PasteRule, a PasteTurn with a rule over both sides and dst's own
// arrays, asked through rule_relation and rule_takes (tests/sanitize/paste_rule_plan_sanitize.cpp).
// The arrays may be the host images or the copies in HBM; every node and material index is widened to 64 bits before it
// addresses memory.
#pragma once

#include <stdint.h>

#include "svo_common.h"

namespace svo {

// a tree's arrays as the cell logic reads them
struct PasteTree {
    const Node* nodes;
    const uint16_t* mats;
    int32_t levels;
};

// A paste as the patch holds it, after the host's checks.
struct PasteRec {
    int32_t lo[3], hi[3];     // the destination box (hi = one past the last voxel), inside the destination's extent
    int32_t shift[3];         // a destination voxel q reads the source at q + shift: lo + shift .. hi + shift lies inside src
    uint32_t keep_empty;      // SVO_PASTE_KEEP_EMPTY: a voxel at which src stores nothing leaves dst as it is
    const uint32_t* in_view;  // bit id: dst's view stores palette id (an id it does not hold is stored empty); NULL: all
};

// An oriented paste: a signed permutation of the axes and a table for the ids.  The destination voxel q reads the source
// at s with s[axis[a]] = sign[a] * q[a] + shift[a]: PasteRec's shift is the map's offset here (for the identity the two
// readings agree).  An aligned box of cs voxels per axis maps to a box of cs voxels per axis, so what paste_relation says
// about the 2 x 2 x 2 aligned src cells holds as it stands.
struct PasteTurn : PasteRec {
    uint8_t axis[3];         // a permutation of 0, 1, 2
    int8_t sign[3];          // +1, or -1 where dst's axis runs against src's
    const uint16_t* id_map;  // one entry per entry of src's palette, [0] == 0 (host image or HBM, as the trees); NULL: none
};

enum : uint32_t { PASTE_OUT = 0u, PASTE_IN = 1u, PASTE_CUT = 2u };
constexpr uint32_t kPasteMixed = 0xFFFFFFFFu;  // src_cell: not uniform (an id is below 65536)

// where the destination voxel q reads the source
SVO_HD void paste_source(const PasteRec& R, const int32_t q[3], uint32_t s[3]) {
    for (int a = 0; a < 3; a++) s[a] = (uint32_t)(q[a] + R.shift[a]);
}
SVO_HD void paste_source(const PasteTurn& R, const int32_t q[3], uint32_t s[3]) {
    for (int a = 0; a < 3; a++) {
        const uint32_t v = (uint32_t)((int32_t)R.sign[a] * q[a] + R.shift[a]);
        // (no indexing by axis[a]: the arrays stay in registers)
        s[0] = R.axis[a] == 0 ? v : s[0];
        s[1] = R.axis[a] == 1 ? v : s[1];
        s[2] = R.axis[a] == 2 ? v : s[2];
    }
}

// what src_cell or tree_voxel returned, through the id map: applied before the uniformity comparison and the mode.  The
// table is read whatever the id is (kPasteMixed reads entry 0), so that every lane makes the same loads
SVO_HD uint32_t paste_mapped(const PasteRec&, uint32_t id) { return id; }
SVO_HD uint32_t paste_mapped(const PasteTurn& R, uint32_t id) {
    if (!R.id_map) return id;
    const uint32_t m = R.id_map[id == kPasteMixed ? 0u : id];
    return id == kPasteMixed ? id : m;
}

// the id as dst stores it
SVO_HD uint32_t paste_resolve(const PasteRec& R, uint32_t id) {
    return (!R.in_view || ((R.in_view[id >> 5] >> (id & 31u)) & 1u)) ? id : 0u;
}

// svo_tree_get_block's descent: the id the tree stores at a voxel of its extent, 0 for none
SVO_HD uint32_t tree_voxel(const PasteTree& T, uint32_t x, uint32_t y, uint32_t z) {
    uint64_t ni = 0;
    for (int d = 0; d < T.levels; d++) {
        const Node n = T.nodes[ni];
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) return node_material(n.info);
        if (kind == K_BRICK) {
            const uint32_t v = ((z & 3u) << 4) | ((y & 3u) << 2) | (x & 3u);
            if (!((n.mask >> v) & 1ull)) return 0u;
            return (n.info & K_UNIFORM) ? node_material(n.info)
                                        : T.mats[(uint64_t)n.ref + (uint64_t)__builtin_popcountll(n.mask & ((1ull << v) - 1ull))];
        }
        const uint32_t sh = (uint32_t)(2 * (T.levels - 1 - d));
        const uint32_t sl = (((z >> sh) & 3u) << 4) | (((y >> sh) & 3u) << 2) | ((x >> sh) & 3u);
        if (!((n.mask >> sl) & 1ull)) return 0u;
        ni = (uint64_t)n.ref + (uint64_t)__builtin_popcountll(n.mask & ((1ull << sl) - 1ull));
    }
    return 0u;
}

// The aligned cell of src at depth `depth` (4^(levels - depth) voxels wide, depth <= levels - 1) that holds the voxel
// (x, y, z): the id it holds throughout (0: nothing), or kPasteMixed.  Down from the root: a K_SOLID record at or above
// the cell gives its id, a clear slot bit at or above it gives 0, a record at the cell's own level — K_INTERIOR with any
// mask, K_BRICK — gives kPasteMixed.  The loop runs depth + 1 times whatever it finds (a finished walk re-reads its
// last record), so that on the device its trip count is the same in all lanes.
SVO_HD uint32_t src_cell(const PasteTree& S, int depth, uint32_t x, uint32_t y, uint32_t z) {
    uint64_t ni = 0;
    uint32_t res = kPasteMixed;
    bool done = false;
    for (int d = 0; d <= depth; d++) {
        const Node n = S.nodes[ni];
        const uint32_t kind = node_kind(n.info);
        const uint32_t sh = (uint32_t)(2 * (S.levels - 1 - d));
        const uint32_t sl = (((z >> sh) & 3u) << 4) | (((y >> sh) & 3u) << 2) | ((x >> sh) & 3u);
        const bool has = (n.mask >> sl) & 1ull;
        const uint64_t child = (uint64_t)n.ref + (uint64_t)__builtin_popcountll(n.mask & ((1ull << sl) - 1ull));
        if (!done) {
            if (kind == K_SOLID) {
                res = node_material(n.info);
                done = true;
            } else if (d == depth || kind == K_BRICK) {
                done = true;  // mixed
            } else if (!has) {
                res = 0u;
                done = true;
            } else {
                ni = child;
            }
        }
    }
    return res;
}

// The aligned destination cell [x, x + cs) x [y, y + cs) x [z, z + cs), cs = 4^k with k >= 1, against the paste:
//   OUT     no voxel of the cell changes: the cell does not meet the box, or (KEEP_EMPTY) src stores nothing in its part
//           of the box, wherever the cell lies against the box;
//   IN      the cell lies wholly inside the box and ends up uniformly *id (already resolved against dst's view; 0: empty);
//   CUT     everything else: descend.
// The cell is clipped to the box and its two ends are mapped into src (paste_source; under a flip the first end is the
// higher one, and the eight corners take either end per src axis, so nothing is reordered); the mapped region is at most
// cs wide per axis, so it meets at most 2 x 2 x 2 aligned src cells of width min(cs, src's extent), and it is uniform when
// all of them are, with one mapped id (two src cells of different ids that map to one id count as uniform).
// Conservative on purpose, as cell_relation is for late shapes: a mixed src cell whose overlapping part happens to be
// uniform is CUT and comes out right at a finer level or at the voxels; a full one-material brick that stayed a brick and
// an interior record with mask 0 count as mixed.  The result is content, not canonical layout.  All eight src cells are
// walked even where they coincide, so that on the device every lane makes the same number of dependent loads.
template <class Rec>
SVO_HD uint32_t paste_relation(const Rec& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) {
    const int32_t c[3] = {x, y, z};
    bool out = false, in = true;
    int32_t q0[3], q1[3];
    for (int a = 0; a < 3; a++) {
        out = out || c[a] + cs <= R.lo[a] || c[a] >= R.hi[a];
        in = in && c[a] >= R.lo[a] && c[a] + cs <= R.hi[a];
        const int32_t lo = c[a] > R.lo[a] ? c[a] : R.lo[a], hi = c[a] + cs < R.hi[a] ? c[a] + cs : R.hi[a];
        q0[a] = lo;  // the first and the last voxel of the clipped cell
        q1[a] = hi - 1;
    }
    uint32_t a0[3] = {0u, 0u, 0u}, a1[3] = {0u, 0u, 0u};  // the same two in src (not read when the cell is out)
    paste_source(R, q0, a0);
    paste_source(R, q1, a1);
    *id = 0u;
    if (out) return PASTE_OUT;
    const int depth = k < S.levels ? S.levels - k : 0;
    uint32_t first = 0u;
    bool uni = true;
    for (uint32_t i = 0; i < 8u; i++) {
        const uint32_t u = paste_mapped(R, src_cell(S, depth, (i & 1u) ? a1[0] : a0[0], (i & 2u) ? a1[1] : a0[1], (i & 4u) ? a1[2] : a0[2]));
        first = i == 0u ? u : first;
        uni = uni && u != kPasteMixed && u == first;
    }
    if (uni && first == 0u && R.keep_empty) return PASTE_OUT;
    if (uni && in) {
        *id = paste_resolve(R, first);
        return PASTE_IN;
    }
    return PASTE_CUT;
}

// one destination voxel: true when the paste decides it — the box holds it and the mode lets src's mapped id through —,
// *id then what dst stores there
template <class Rec>
SVO_HD bool paste_takes(const Rec& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, uint32_t* id) {
    *id = 0u;
    if (x < R.lo[0] || x >= R.hi[0] || y < R.lo[1] || y >= R.hi[1] || z < R.lo[2] || z >= R.hi[2]) return false;
    const int32_t q[3] = {x, y, z};
    uint32_t p[3] = {0u, 0u, 0u};
    paste_source(R, q, p);
    const uint32_t s = paste_mapped(R, tree_voxel(S, p[0], p[1], p[2]));
    if (s == 0u && R.keep_empty) return false;
    *id = paste_resolve(R, s);
    return true;
}

// the composite voxel after the paste: the paste's where it decides, else dst's own
template <class Rec>
SVO_HD uint32_t paste_voxel(const Rec& R, const PasteTree& S, const PasteTree& D, int32_t x, int32_t y, int32_t z) {
    uint32_t id;
    return paste_takes(R, S, x, y, z, &id) ? id : tree_voxel(D, (uint32_t)x, (uint32_t)y, (uint32_t)z);
}

// svo_tree_patch_tree_rule_gpu: an oriented paste that decides every voxel from both sides.  s is src's mapped id (steps
// (1) and (2) of the oriented paste), d the id dst stores at the voxel on entry, in dst's own view; `rule` holds, two bits
// each, what the voxel keeps in the three cases that are not trivially empty (include/svo_rt.h SVO_RULE):
//   A = rule & 3         s != 0, d == 0:  KEEP (stays empty) or TAKE (src's id, resolved against dst's view)
//   B = (rule >> 2) & 3  s != 0, d != 0:  KEEP (d), TAKE or CLEAR (empty)
//   C = (rule >> 4) & 3  s == 0, d != 0:  KEEP (d) or CLEAR
// The record carries dst's arrays as they were on entry (the host images, or the copies in HBM, as src's): the patch is
// written to scratch, so they do not change under the descent.  keep_empty is not read.
enum : uint32_t { RULE_KEEP = 0u, RULE_TAKE = 1u, RULE_CLEAR = 2u };
struct PasteRule : PasteTurn {
    uint32_t rule;  // checked by the host (svo_plan.cpp paste_rule_check)
    PasteTree dst;
};

// The aligned destination cell under a rule: paste_relation's three answers.  The src side is paste_relation's — the
// clipped cell's ends mapped into src, the 2 x 2 x 2 src_cell walks through the id map: uniform 0, uniform id or mixed —
// and the dst side is one more src_cell walk, over dst's arrays at the cell's own depth: a K_SOLID record at or above the
// cell (uniform), a clear slot bit at or above it (empty), or a record at its level (mixed).  Nine walks of at most 7
// dependent loads, the same trip count in every lane.
//   OUT     the cell misses the box, or no voxel of its part of the box can change: src stores nothing there and C keeps
//           (or dst is empty too); dst is empty and A keeps; src stores something throughout and dst's answer is kept
//           whatever it is (dst uniform and B keeps, dst mixed and A and B keep); src is mixed and dst uniform, B and C
//           keep.  All of them wherever the cell lies against the box;
//   IN      the cell lies wholly inside the box and every voxel of it ends as *id: src is uniform, and so is dst, or the
//           rule gives d == 0 and d != 0 the same outcome;
//   CUT     everything else: the box's surface cuts the cell, a src record of its level overlaps it, or the outcome depends
//           on d and dst holds a record of the cell's level under a non-empty src region.
// Conservative as paste_relation is; a K_SOLID record of id 0, should one exist, reads as empty on either side.
SVO_HD uint32_t rule_relation(const PasteRule& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) {
    const int32_t c[3] = {x, y, z};
    bool out = false, in = true;
    int32_t q0[3], q1[3];
    for (int a = 0; a < 3; a++) {
        out = out || c[a] + cs <= R.lo[a] || c[a] >= R.hi[a];
        in = in && c[a] >= R.lo[a] && c[a] + cs <= R.hi[a];
        const int32_t lo = c[a] > R.lo[a] ? c[a] : R.lo[a], hi = c[a] + cs < R.hi[a] ? c[a] + cs : R.hi[a];
        q0[a] = lo;
        q1[a] = hi - 1;
    }
    uint32_t a0[3] = {0u, 0u, 0u}, a1[3] = {0u, 0u, 0u};
    paste_source(R, q0, a0);
    paste_source(R, q1, a1);
    *id = 0u;
    if (out) return PASTE_OUT;
    const int depth = k < S.levels ? S.levels - k : 0;
    uint32_t first = 0u;
    bool uni = true;
    for (uint32_t i = 0; i < 8u; i++) {
        const uint32_t u = paste_mapped(R, src_cell(S, depth, (i & 1u) ? a1[0] : a0[0], (i & 2u) ? a1[1] : a0[1], (i & 4u) ? a1[2] : a0[2]));
        first = i == 0u ? u : first;
        uni = uni && u != kPasteMixed && u == first;
    }
    // the cell itself in dst (k <= dst's levels - 1: the descent starts below the root)
    const uint32_t d = src_cell(R.dst, R.dst.levels - k, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    const uint32_t A = R.rule & 3u, B = (R.rule >> 2) & 3u, C = (R.rule >> 4) & 3u;
    const bool d_empty = d == 0u, d_uni = d != 0u && d != kPasteMixed;
    const uint32_t took = uni ? paste_resolve(R, first) : 0u;
    if (uni && first == 0u) {
        if (C == RULE_KEEP || d_empty) return PASTE_OUT;
        return in ? PASTE_IN : PASTE_CUT;  // cleared
    }
    if (d_empty) {
        if (A == RULE_KEEP) return PASTE_OUT;
        *id = took;
        return uni && in ? PASTE_IN : PASTE_CUT;
    }
    if (!uni) return d_uni && B == RULE_KEEP && C == RULE_KEEP ? PASTE_OUT : PASTE_CUT;
    if (d_uni) {
        if (B == RULE_KEEP) return PASTE_OUT;
        *id = B == RULE_TAKE ? took : 0u;
        return in ? PASTE_IN : PASTE_CUT;
    }
    // dst mixed under one src id: decided at the cell only where d == 0 and d != 0 end alike
    if (A == RULE_KEEP && B == RULE_KEEP) return PASTE_OUT;
    if (A == RULE_TAKE && B == RULE_TAKE) {
        *id = took;
        return in ? PASTE_IN : PASTE_CUT;
    }
    if (A == RULE_KEEP && B == RULE_CLEAR) return in ? PASTE_IN : PASTE_CUT;
    return PASTE_CUT;
}

// one destination voxel under a rule: true when the rule changes or decides it, *id then what dst stores there.  d is
// read from dst's arrays as they were on entry
SVO_HD bool rule_takes(const PasteRule& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, uint32_t* id) {
    *id = 0u;
    if (x < R.lo[0] || x >= R.hi[0] || y < R.lo[1] || y >= R.hi[1] || z < R.lo[2] || z >= R.hi[2]) return false;
    const int32_t q[3] = {x, y, z};
    uint32_t p[3] = {0u, 0u, 0u};
    paste_source(R, q, p);
    const uint32_t s = paste_mapped(R, tree_voxel(S, p[0], p[1], p[2]));
    const uint32_t d = tree_voxel(R.dst, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    if (s == 0u) return d != 0u && ((R.rule >> 4) & 3u) == RULE_CLEAR;
    const uint32_t f = d == 0u ? R.rule & 3u : (R.rule >> 2) & 3u;
    if (f == RULE_KEEP) return false;
    *id = f == RULE_TAKE ? paste_resolve(R, s) : 0u;
    return true;
}

// the composite voxel after a rule paste
SVO_HD uint32_t rule_voxel(const PasteRule& R, const PasteTree& S, int32_t x, int32_t y, int32_t z) {
    uint32_t id;
    return rule_takes(R, S, x, y, z, &id) ? id : tree_voxel(R.dst, (uint32_t)x, (uint32_t)y, (uint32_t)z);
}

// The question a record asks of a cell and of a voxel, by record type: the patch's device class and the host's garbage
// walk are written once over these
template <class Rec>
SVO_HD uint32_t relation_of(const Rec& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) {
    return paste_relation(R, S, x, y, z, cs, k, id);
}
SVO_HD uint32_t relation_of(const PasteRule& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, int32_t cs, int k, uint32_t* id) {
    return rule_relation(R, S, x, y, z, cs, k, id);
}
template <class Rec>
SVO_HD bool takes_of(const Rec& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, uint32_t* id) {
    return paste_takes(R, S, x, y, z, id);
}
SVO_HD bool takes_of(const PasteRule& R, const PasteTree& S, int32_t x, int32_t y, int32_t z, uint32_t* id) {
    return rule_takes(R, S, x, y, z, id);
}

}  // namespace svo
