// points_patch_plan_sanitize.cpp — svo_plan.cpp's host half of svo_tree_patch_points_gpu under AddressSanitizer + UBSan:
// points_anchor (where the device descent starts, from the first and last key of the sorted edit list) and
// ceil_block_rects (the touched 16 x 16-column blocks merged into rectangles) on small hand-built node arrays and block
// lists, each in a heap array of its exact size so that a read past it is reported.
// Built and run by tests/test_points_patch_plan_host.py.
#include <stdio.h>
#include <stdlib.h>

#include <array>
#include <vector>

#include "../../raytracing_test_amd/csrc/svo_plan.h"

using namespace svo;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            fails++;                                                \
        }                                                           \
    } while (0)

static Node interior(uint64_t mask, uint32_t ref) { return Node{mask, ref, K_INTERIOR}; }
static Node solid(uint32_t m) { return Node{~0ull, 0u, K_SOLID | (m << 16)}; }
static uint32_t slot(int x, int y, int z) { return (uint32_t)((z << 4) | (y << 2) | x); }

// svo_points_source.h voxel_key, restated: 6 bits per level, z<<4 | y<<2 | x, the top level first
static uint64_t key(uint32_t x, uint32_t y, uint32_t z, int32_t levels) {
    uint64_t k = 0;
    for (int d = 0; d < levels; d++) {
        const uint32_t sh = (uint32_t)(2 * (levels - 1 - d));
        k = (k << 6) | (uint64_t)((((z >> sh) & 3u) << 4) | (((y >> sh) & 3u) << 2) | ((x >> sh) & 3u));
    }
    return k;
}

static uint64_t blk(int64_t bx, int64_t bz) { return ((uint64_t)bz << 32) | (uint64_t)bx; }
typedef std::array<int64_t, 4> Rect;
static bool same(const std::vector<Rect>& got, std::vector<Rect> want) {
    if (got.size() != want.size()) return false;
    for (const Rect& w : want) {
        bool found = false;
        for (const Rect& g : got) found = found || g == w;
        if (!found) return false;
    }
    return true;
}

int main() {
    // 3 levels (64^3).  Root: child (0,0,0) interior (node 1), child (1,0,0) SOLID 3 (node 2), child (1,1,1) interior (node 3).
    // node 1 (0..16)^3: brick (0,0,0) uniform (node 4), brick (1,1,0) uniform with a hole (node 5).
    // node 3 (16..32)^3: brick (3,3,3) = (28..32)^3 with a material run of 3 entries (node 6).
    std::vector<Node> t3;
    t3.push_back(interior((1ull << slot(0, 0, 0)) | (1ull << slot(1, 0, 0)) | (1ull << slot(1, 1, 1)), 1));
    t3.push_back(interior((1ull << slot(0, 0, 0)) | (1ull << slot(1, 1, 0)), 4));
    t3.push_back(solid(3));
    t3.push_back(interior(1ull << slot(3, 3, 3), 6));
    t3.push_back(Node{~0ull, 0u, K_BRICK | K_UNIFORM | (2u << 16)});
    t3.push_back(Node{~0ull ^ 2ull, 0u, K_BRICK | K_UNIFORM | (1u << 16)});
    t3.push_back(Node{0x8000000000000003ull, 0u, K_BRICK});

    {  // one edit: the anchor is the brick's parent, whatever the brick holds (here: an absent brick of node 1)
        const uint64_t k = key(9, 2, 13, 3);
        const PatchAnchor a = points_anchor(t3.data(), 3, k, k);
        CHECK(a.node == 1 && a.depth == 1 && a.kind == P_NODE && a.old == 1 && !a.whole);
        CHECK(a.o[0] == 0 && a.o[1] == 0 && a.o[2] == 0);
    }
    {  // one edit in the last region with an interior record: the origin is carried down
        const uint64_t k = key(31, 31, 31, 3);
        const PatchAnchor a = points_anchor(t3.data(), 3, k, k);
        CHECK(a.node == 3 && a.depth == 1 && a.kind == P_NODE && !a.whole);
        CHECK(a.o[0] == 16 && a.o[1] == 16 && a.o[2] == 16);
    }
    {  // two edits in one brick
        const PatchAnchor a = points_anchor(t3.data(), 3, key(4, 4, 0, 3), key(7, 7, 3, 3));
        CHECK(a.node == 1 && a.depth == 1 && !a.whole);
    }
    {  // two edits in two bricks of one depth-1 child: the digits part at the brick level, below the anchor's depth
        const PatchAnchor a = points_anchor(t3.data(), 3, key(0, 0, 0, 3), key(15, 15, 15, 3));
        CHECK(a.node == 1 && a.depth == 1 && !a.whole);
    }
    {  // two edits in opposite corners of the world: the anchor is the root, and never whole
        const PatchAnchor a = points_anchor(t3.data(), 3, key(0, 0, 0, 3), key(63, 63, 63, 3));
        CHECK(a.node == 0 && a.depth == 0 && a.kind == P_NODE && a.old == 0 && !a.whole);
        CHECK(a.o[0] == 0 && a.o[1] == 0 && a.o[2] == 0);
    }
    {  // the path meets a SOLID child
        const uint64_t k = key(18, 2, 2, 3);
        const PatchAnchor a = points_anchor(t3.data(), 3, k, k);
        CHECK(a.node == 0 && a.depth == 0 && a.kind == P_NODE && !a.whole);
    }
    {  // the path meets an empty slot
        const uint64_t k = key(40, 40, 40, 3);
        const PatchAnchor a = points_anchor(t3.data(), 3, k, k);
        CHECK(a.node == 0 && a.depth == 0 && a.kind == P_NODE && !a.whole);
    }
    std::vector<Node> lone{solid(7)};
    {  // a lone SOLID root becomes interior: the anchor is the root, holding material 7 throughout
        const uint64_t k = key(5, 6, 7, 3);
        const PatchAnchor a = points_anchor(lone.data(), 3, k, k);
        CHECK(a.node == 0 && a.depth == 0 && a.kind == P_UNIFORM && a.old == 7 && !a.whole);
    }
    std::vector<Node> empty{interior(0, 0)};
    {  // the empty tree's lone record, at 2 levels: the root is the only anchor there is
        const uint64_t k = key(3, 3, 3, 2);
        const PatchAnchor a = points_anchor(empty.data(), 2, k, k);
        CHECK(a.node == 0 && a.depth == 0 && a.kind == P_NODE);
        const PatchAnchor b = points_anchor(empty.data(), 2, key(0, 0, 0, 2), key(15, 15, 15, 2));
        CHECK(b.node == 0 && b.depth == 0);
    }
    // 4 levels (256^3): root -> (3,3,3) interior (node 1, 192..256) -> (0,0,0) interior (node 2, 192..208) -> brick (0,0,0)
    std::vector<Node> t4;
    t4.push_back(interior(1ull << 63, 1));
    t4.push_back(interior(1ull, 2));
    t4.push_back(interior(1ull, 3));
    t4.push_back(Node{0xFFull, 0u, K_BRICK});
    {  // the walk stops above the brick level, although the brick's record is there
        const uint64_t k = key(193, 193, 193, 4);
        const PatchAnchor a = points_anchor(t4.data(), 4, k, k);
        CHECK(a.node == 2 && a.depth == 2 && a.o[0] == 192 && a.o[1] == 192 && a.o[2] == 192);
    }
    {  // edits in two depth-2 regions stop one level higher
        const PatchAnchor a = points_anchor(t4.data(), 4, key(193, 193, 193, 4), key(210, 193, 193, 4));
        CHECK(a.node == 1 && a.depth == 1 && a.o[0] == 192 && a.o[1] == 192 && a.o[2] == 192);
    }

    // the merge of touched column blocks (16 columns wide) into rectangles {x0, z0, x1, z1}
    {
        std::vector<uint64_t> b{blk(5, 9)};
        CHECK(same(ceil_block_rects(b), {Rect{80, 144, 96, 160}}));
    }
    {  // one run
        std::vector<uint64_t> b{blk(2, 1), blk(3, 1), blk(4, 1)};
        CHECK(same(ceil_block_rects(b), {Rect{32, 16, 80, 32}}));
    }
    {  // two runs in a row
        std::vector<uint64_t> b{blk(0, 3), blk(1, 3), blk(3, 3), blk(4, 3), blk(5, 3)};
        CHECK(same(ceil_block_rects(b), {Rect{0, 48, 32, 64}, Rect{48, 48, 96, 64}}));
    }
    {  // a full row of a 3-level world (4 blocks)
        std::vector<uint64_t> b{blk(0, 2), blk(1, 2), blk(2, 2), blk(3, 2)};
        CHECK(same(ceil_block_rects(b), {Rect{0, 32, 64, 48}}));
    }
    {  // unsorted, with duplicates
        std::vector<uint64_t> b{blk(4, 1), blk(2, 1), blk(3, 1), blk(2, 1), blk(9, 0), blk(4, 1), blk(9, 0)};
        CHECK(same(ceil_block_rects(b), {Rect{144, 0, 160, 16}, Rect{32, 16, 80, 32}}));
    }
    {  // every block of a 64^3 world: equal runs in consecutive rows join into one rectangle
        std::vector<uint64_t> b;
        for (int z = 3; z >= 0; z--)
            for (int x = 0; x < 4; x++) b.push_back(blk(x, z));
        CHECK(same(ceil_block_rects(b), {Rect{0, 0, 64, 64}}));
    }
    {  // runs of different spans in consecutive rows stay apart; a gap of one row ends a rectangle
        std::vector<uint64_t> b{blk(1, 0), blk(2, 0), blk(1, 1), blk(1, 2), blk(7, 0), blk(7, 1), blk(7, 3), blk(1000, 1023)};
        CHECK(same(ceil_block_rects(b), {Rect{16, 0, 48, 16}, Rect{16, 16, 32, 48}, Rect{112, 0, 128, 32}, Rect{112, 48, 128, 64},
                                         Rect{16000, 16368, 16016, 16384}}));
    }
    {
        std::vector<uint64_t> b;
        CHECK(ceil_block_rects(b).empty());
    }
    if (fails) return 1;
    printf("points patch plan sanitize ok\n");
    return 0;
}
