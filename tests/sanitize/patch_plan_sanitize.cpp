// patch_plan_sanitize.cpp — svo_plan.cpp's host half of svo_tree_patch_volume_gpu under AddressSanitizer + UBSan:
// patch_anchor (where the device descent starts) and patch_superseded (what the patch leaves unreachable) on small
// hand-built node arrays, each in a heap array of its exact size so that a read past it is reported.
// Built and run by tests/test_patch_plan_host.py.
#include <stdio.h>
#include <stdlib.h>

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

struct Got {
    PatchAnchor a;
    uint64_t gn, gm;
};
static Got plan(const std::vector<Node>& nodes, int32_t levels, int x0, int y0, int z0, int x1, int y1, int z1) {
    const int32_t lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
    Got g{patch_anchor(nodes.data(), levels, lo, hi), 0, 0};
    patch_superseded(nodes.data(), levels, g.a, lo, hi, &g.gn, &g.gm);
    return g;
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

    {  // a box inside one brick: the anchor is the brick's parent
        const Got g = plan(t3, 3, 1, 1, 1, 3, 3, 3);
        CHECK(g.a.node == 1 && g.a.depth == 1 && g.a.kind == P_NODE && g.a.old == 1 && !g.a.whole);
        CHECK(g.a.o[0] == 0 && g.a.o[1] == 0 && g.a.o[2] == 0);
        CHECK(g.gn == 2 && g.gm == 0);  // node 1's child block; the brick is uniform
    }
    {  // a box inside one depth-1 child, across its bricks
        const Got g = plan(t3, 3, 2, 2, 2, 10, 10, 3);
        CHECK(g.a.node == 1 && g.a.depth == 1 && !g.a.whole);
        CHECK(g.gn == 2 && g.gm == 0);
    }
    {  // a box that fills a depth-1 child: that child is wholly inside, the anchor is its parent
        const Got g = plan(t3, 3, 0, 0, 0, 16, 16, 16);
        CHECK(g.a.node == 0 && g.a.depth == 0 && !g.a.whole);
        CHECK(g.gn == 3 + 2 && g.gm == 0);  // the root's block and the whole subtree of node 1
    }
    {  // a box across the world centre: the anchor is the root
        const Got g = plan(t3, 3, 28, 28, 28, 37, 37, 37);
        CHECK(g.a.node == 0 && g.a.depth == 0 && g.a.kind == P_NODE && !g.a.whole);
        CHECK(g.gn == 3 + 1 && g.gm == 3);  // the root's block, node 3's block, the run of the brick at (28..32)^3
    }
    {  // the path meets a SOLID child early
        const Got g = plan(t3, 3, 18, 2, 2, 20, 4, 4);
        CHECK(g.a.node == 0 && g.a.depth == 0 && g.a.kind == P_NODE);
        CHECK(g.gn == 3 && g.gm == 0);
    }
    {  // the path meets an empty slot early
        const Got g = plan(t3, 3, 40, 40, 40, 42, 42, 42);
        CHECK(g.a.node == 0 && g.a.depth == 0 && g.a.kind == P_NODE);
        CHECK(g.gn == 3 && g.gm == 0);
    }
    {  // the whole extent: the root itself is replaced
        const Got g = plan(t3, 3, 0, 0, 0, 64, 64, 64);
        CHECK(g.a.whole && g.a.node == 0 && g.a.depth == 0);
        CHECK(g.gn == 6 && g.gm == 3);  // every record below the root
    }
    {  // one voxel in the last brick of the extent
        const Got g = plan(t3, 3, 63, 63, 63, 64, 64, 64);
        CHECK(g.a.node == 0 && !g.a.whole);
    }

    std::vector<Node> lone{solid(7)};
    {  // a lone SOLID root becomes interior: the anchor is the root, holding material 7 throughout
        const Got g = plan(lone, 3, 5, 6, 7, 10, 11, 12);
        CHECK(g.a.node == 0 && g.a.depth == 0 && g.a.kind == P_UNIFORM && g.a.old == 7 && !g.a.whole);
        CHECK(g.gn == 0 && g.gm == 0);
        const Got w = plan(lone, 3, 0, 0, 0, 64, 64, 64);
        CHECK(w.a.whole && w.a.kind == P_UNIFORM);
    }
    std::vector<Node> empty{interior(0, 0)};
    {  // the empty tree's lone record
        const Got g = plan(empty, 2, 3, 3, 3, 4, 4, 4);
        CHECK(g.a.node == 0 && g.a.depth == 0 && g.a.kind == P_NODE && g.gn == 0 && g.gm == 0);
    }

    // 4 levels (256^3): root -> (3,3,3) interior (node 1, 192..256) -> (0,0,0) interior (node 2, 192..208) -> brick (0,0,0)
    std::vector<Node> t4;
    t4.push_back(interior(1ull << 63, 1));
    t4.push_back(interior(1ull, 2));
    t4.push_back(interior(1ull, 3));
    t4.push_back(Node{0xFFull, 0u, K_BRICK});
    {  // the walk stops above the brick level, with the region's origin carried down
        const Got g = plan(t4, 4, 193, 193, 193, 195, 195, 195);
        CHECK(g.a.node == 2 && g.a.depth == 2 && g.a.o[0] == 192 && g.a.o[1] == 192 && g.a.o[2] == 192);
        CHECK(g.gn == 1 && g.gm == 8);
    }
    {  // a box over two depth-2 regions stops one level higher
        const Got g = plan(t4, 4, 200, 193, 193, 210, 195, 195);
        CHECK(g.a.node == 1 && g.a.depth == 1 && g.a.o[0] == 192);
        CHECK(g.gn == 1 + 1 && g.gm == 0);  // node 1's block, node 2's block (cut); the brick at 192..196 is outside
    }
    if (fails) return 1;
    printf("patch plan sanitize ok\n");
    return 0;
}
