// shapes_patch_plan_sanitize.cpp — the host half of svo_tree_patch_shapes_gpu under AddressSanitizer + UBSan:
// svo_shape_cell.h's shape_relation, cell_relation and shape_voxel against brute force over the voxels of a 64^3 extent
// (every aligned cell at the three cell sizes 4, 16 and 64), svo_plan.cpp's shapes_plan (the checks, the clipping, the
// view's ids) and shapes_superseded (the garbage walk) on a small hand-built node array held in a heap array of its exact
// size, so that a read past it is reported.
// Built and run by tests/test_shapes_patch_plan_host.py.
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

static const int E = 64;

static ShapeRec box(int x0, int y0, int z0, int x1, int y1, int z1, uint32_t id) {
    return ShapeRec{kShapeBox, {x0, y0, z0}, {x1, y1, z1}, id, 0};
}
static ShapeRec ball(int cx, int cy, int cz, int64_t r2, uint32_t id) { return ShapeRec{kShapeBall, {cx, cy, cz}, {0, 0, 0}, id, r2}; }

// the definition, voxel by voxel
static bool holds(const ShapeRec& s, int x, int y, int z) {
    if (s.kind == kShapeBox) return x >= s.a[0] && x < s.b[0] && y >= s.a[1] && y < s.b[1] && z >= s.a[2] && z < s.b[2];
    const int64_t dx = (int64_t)x - s.a[0], dy = (int64_t)y - s.a[1], dz = (int64_t)z - s.a[2];
    return dx * dx + dy * dy + dz * dz <= s.r2;
}

static uint32_t brute_relation(const std::vector<uint8_t>& in, int x, int y, int z, int cs) {
    int64_t n = 0;
    for (int k = z; k < z + cs; k++)
        for (int j = y; j < y + cs; j++)
            for (int i = x; i < x + cs; i++) n += in[((size_t)k * E + j) * E + i];
    return n == 0 ? SHAPE_OUT : (n == (int64_t)cs * cs * cs ? SHAPE_IN : SHAPE_CUT);
}

// every aligned cell of the extent at the three sizes, and every voxel, for one table; returns how many cells were IN, CUT
static void check_table(const std::vector<ShapeRec>& tab, int64_t counts[3]) {
    const int n = (int)tab.size();
    ShapeRec* heap = (ShapeRec*)malloc(sizeof(ShapeRec) * (size_t)(n > 0 ? n : 1));  // exact size: a read past it is reported
    for (int i = 0; i < n; i++) heap[i] = tab[(size_t)i];
    std::vector<std::vector<uint8_t>> in((size_t)n, std::vector<uint8_t>((size_t)E * E * E));
    for (int s = 0; s < n; s++)
        for (int z = 0; z < E; z++)
            for (int y = 0; y < E; y++)
                for (int x = 0; x < E; x++) in[(size_t)s][((size_t)z * E + y) * E + x] = holds(tab[(size_t)s], x, y, z) ? 1 : 0;
    counts[0] = counts[1] = counts[2] = 0;
    for (int cs = 4; cs <= E; cs *= 4)
        for (int z = 0; z < E; z += cs)
            for (int y = 0; y < E; y += cs)
                for (int x = 0; x < E; x += cs) {
                    uint32_t want = SHAPE_OUT, want_id = 0;
                    for (int s = 0; s < n; s++) {
                        const uint32_t b = brute_relation(in[(size_t)s], x, y, z, cs);
                        CHECK(shape_relation(heap[s], x, y, z, cs) == b);
                    }
                    for (int s = n - 1; s >= 0; s--) {
                        const uint32_t b = brute_relation(in[(size_t)s], x, y, z, cs);
                        if (b != SHAPE_OUT) {
                            want = b;
                            want_id = tab[(size_t)s].id;
                            break;
                        }
                    }
                    uint32_t id = 77u;
                    const uint32_t got = cell_relation(heap, n, x, y, z, cs, &id);
                    CHECK(got == want);
                    CHECK(got == SHAPE_CUT || id == want_id);
                    counts[got]++;
                }
    for (int z = 0; z < E; z++)
        for (int y = 0; y < E; y++)
            for (int x = 0; x < E; x++) {
                bool hit = false;
                uint32_t want_id = 0;
                for (int s = n - 1; s >= 0 && !hit; s--)
                    if (in[(size_t)s][((size_t)z * E + y) * E + x]) {
                        hit = true;
                        want_id = tab[(size_t)s].id;
                    }
                uint32_t id = 77u;
                const bool got = shape_voxel(heap, n, x, y, z, &id);
                CHECK(got == hit);
                CHECK(!got || id == want_id);
                // an IN cell is uniformly its id, an OUT cell holds no shape's voxel: the brick that holds the voxel
                uint32_t cid = 0;
                const uint32_t rel = cell_relation(heap, n, x & ~3, y & ~3, z & ~3, 4, &cid);
                if (rel == SHAPE_IN) CHECK(got && id == cid);
                if (rel == SHAPE_OUT) CHECK(!got);
            }
    free(heap);
}

static Node interior(uint64_t mask, uint32_t ref) { return Node{mask, ref, K_INTERIOR}; }
static Node solid(uint32_t m) { return Node{~0ull, 0u, K_SOLID | (m << 16)}; }
static uint32_t slot(int x, int y, int z) { return (uint32_t)((z << 4) | (y << 2) | x); }

static svo_shape abi_box(int x, int y, int z, int nx, int ny, int nz, uint16_t id) {
    svo_shape s;
    s.kind = SVO_SHAPE_BOX;
    s.a[0] = x, s.a[1] = y, s.a[2] = z;
    s.b[0] = nx, s.b[1] = ny, s.b[2] = nz;
    s.r2 = 0;
    s.id = id;
    return s;
}
static svo_shape abi_ball(int x, int y, int z, int64_t r2, uint16_t id) {
    svo_shape s;
    s.kind = SVO_SHAPE_BALL;
    s.a[0] = x, s.a[1] = y, s.a[2] = z;
    s.b[0] = s.b[1] = s.b[2] = -5;  // ignored
    s.r2 = r2;
    s.id = id;
    return s;
}

int main() {
    int64_t c[3];
    // boxes on and off the grid
    check_table({box(16, 16, 16, 32, 32, 32, 1)}, c);
    CHECK(c[SHAPE_IN] == 64 + 1 && c[SHAPE_CUT] == 1);  // 64 bricks and one 16^3 inside; the extent is cut
    check_table({box(0, 0, 0, 64, 64, 64, 2)}, c);
    CHECK(c[SHAPE_OUT] == 0 && c[SHAPE_CUT] == 0);
    check_table({box(5, 6, 7, 6, 7, 8, 3)}, c);
    CHECK(c[SHAPE_IN] == 0 && c[SHAPE_CUT] == 3);
    check_table({box(3, 9, 21, 50, 31, 64, 1)}, c);
    check_table({box(63, 0, 0, 64, 64, 1, 4)}, c);
    // balls: one voxel, 19 voxels (r2 = 2), 27 (r2 = 3), on a brick corner and inside a brick
    for (int64_t r2 : {0, 2, 3}) {
        check_table({ball(16, 16, 16, r2, 1)}, c);
        CHECK(c[SHAPE_IN] == 0 && c[SHAPE_CUT] == (r2 == 0 ? 3 : (r2 == 2 ? 7 + 7 + 1 : 8 + 8 + 1)));
        check_table({ball(21, 22, 41, r2, 1)}, c);
        CHECK(c[SHAPE_IN] == 0 && c[SHAPE_CUT] == 3);
    }
    check_table({ball(31, 32, 33, 20 * 20, 2)}, c);
    CHECK(c[SHAPE_IN] > 0 && c[SHAPE_CUT] > 0 && c[SHAPE_OUT] > 0);
    check_table({ball(32, 32, 32, 3 * 64 * 64, 2)}, c);  // covers the extent
    CHECK(c[SHAPE_OUT] == 0 && c[SHAPE_CUT] == 0);
    // centred outside the extent: through a face, and missing it altogether
    check_table({ball(-5, 30, 70, 30 * 30, 1)}, c);
    CHECK(c[SHAPE_CUT] > 0);
    check_table({ball(-40, -40, -40, 30 * 30, 1)}, c);
    CHECK(c[SHAPE_IN] == 0 && c[SHAPE_CUT] == 0);
    // at the limits: |c| = 2^20 with r2 = 2^42 holds the whole extent; r2 just past the x = 31 plane cuts it
    check_table({ball(kShapeCentreMax, -kShapeCentreMax, kShapeCentreMax, kShapeR2Max, 1)}, c);
    CHECK(c[SHAPE_OUT] == 0 && c[SHAPE_CUT] == 0);
    {
        const int64_t d = (int64_t)kShapeCentreMax + 31;
        check_table({ball(-kShapeCentreMax, 30, 30, d * d, 1)}, c);
        CHECK(c[SHAPE_IN] > 0 && c[SHAPE_CUT] > 0 && c[SHAPE_OUT] > 0);
    }
    // lists where the order matters: box A, an erasing ball inside it, an overlapping box B — and reversed
    const std::vector<ShapeRec> abc = {box(8, 8, 8, 40, 40, 40, 1), ball(24, 24, 24, 100, 0), box(20, 20, 20, 52, 30, 52, 3)};
    check_table(abc, c);
    int64_t r[3];
    check_table({abc[2], abc[1], abc[0]}, r);
    CHECK(c[SHAPE_IN] != r[SHAPE_IN] || c[SHAPE_CUT] != r[SHAPE_CUT]);
    {  // a cell cut by the late shape and covered by the early one stays CUT: the scan is conservative
        uint32_t id;
        CHECK(cell_relation(abc.data(), 3, 16, 16, 16, 16, &id) == SHAPE_CUT);
        CHECK(cell_relation(abc.data(), 1, 16, 16, 16, 16, &id) == SHAPE_IN && id == 1);
        CHECK(cell_relation(abc.data(), 0, 16, 16, 16, 16, &id) == SHAPE_OUT);
    }
    check_table({}, c);
    CHECK(c[SHAPE_OUT] == 4096 + 64 + 1);

    // ---------------------------------------------------------------------------------------------- shapes_plan
    const std::vector<Material> pal = {Material{0, ~0ull, 0.0f}, Material{1, 5, 0.0f}, Material{1 | 0x10, 6, 0.0f}};  // 2: liquid
    ShapesPlan plan;
    int32_t bad = 99;
    {
        const svo_shape s[] = {abi_box(3, 9, 21, 47, 22, 43, 1), abi_ball(-5, 30, 70, 900, 2), abi_ball(-40, -40, -40, 900, 1),
                               abi_ball(32, 32, 32, 0, 2)};
        CHECK(shapes_plan(3, SVO_VIEW_SOLID, pal, s, 4, &plan, &bad) == SHAPES_OK && bad == -1);
        CHECK(plan.table.size() == 3 && plan.rects.size() == 3);  // the ball that misses the extent is dropped
        CHECK(plan.table[0].kind == kShapeBox && plan.table[0].b[0] == 50 && plan.table[0].b[1] == 31 && plan.table[0].b[2] == 64);
        CHECK(plan.table[0].id == 1 && plan.table[1].id == 0 && plan.table[2].id == 0);  // liquid is stored empty in the solid view
        CHECK((plan.rects[0] == std::array<int64_t, 4>{3, 21, 50, 64}));
        CHECK((plan.rects[1] == std::array<int64_t, 4>{0, 40, 26, 64}));
        CHECK((plan.rects[2] == std::array<int64_t, 4>{32, 32, 33, 33}));
        CHECK(plan.lo[0] == 0 && plan.lo[1] == 0 && plan.lo[2] == 21 && plan.hi[0] == 50 && plan.hi[1] == 61 && plan.hi[2] == 64);
        CHECK(shapes_plan(3, SVO_VIEW_ALL, pal, s, 4, &plan, &bad) == SHAPES_OK && plan.table[1].id == 2);
        CHECK(shapes_plan(3, SVO_VIEW_SOLID, pal, s, 0, &plan, &bad) == SHAPES_OK && plan.table.empty());
    }
    {
        svo_shape s[2] = {abi_box(0, 0, 0, 64, 64, 64, 1), abi_box(0, 0, 0, 64, 64, 64, 1)};
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_OK);
        s[1].kind = 2;
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_KIND && bad == 1);
        s[1] = abi_box(0, 0, 0, 64, 0, 64, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_BOX_DIM && bad == 1);
        s[1] = abi_box(1, 0, 0, 64, 64, 64, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_BOX_EXTENT);
        s[1] = abi_box(0, -1, 0, 4, 4, 4, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_BOX_EXTENT);
        s[1] = abi_box(0x7FFFFFFF, 0, 0, 0x7FFFFFFF, 4, 4, 1);  // no int32 wrap
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_BOX_EXTENT);
        s[1] = abi_box(0, 0, 0, 4, 4, 4, 3);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_ID);
        s[0] = abi_ball(0, 0, 0, -1, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_R2_NEG && bad == 0);
        s[0] = abi_ball(0, kShapeCentreMax + 1, 0, 1, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_CENTRE);
        s[0] = abi_ball(0, 0, -kShapeCentreMax - 1, 1, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_CENTRE);
        s[0] = abi_ball(0, 0, 0, kShapeR2Max + 1, 1);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_R2_BIG);
        s[0] = abi_ball(kShapeCentreMax, -kShapeCentreMax, kShapeCentreMax, kShapeR2Max, 1);
        s[1] = abi_ball(0, 0, 0, 0x7FFFFFFFFFFFFFFFll, 1);
        CHECK(shapes_plan(3, 0, pal, s, 1, &plan, &bad) == SHAPES_OK && plan.table.size() == 1 && plan.hi[0] == 64 && plan.lo[1] == 0);
        CHECK(shapes_plan(3, 0, pal, s, 2, &plan, &bad) == SHAPES_R2_BIG && bad == 1);
    }

    // ---------------------------------------------------------------------------------------- shapes_superseded
    // 3 levels (64^3).  Root: child (0,0,0) interior (node 1), child (1,0,0) SOLID 3 (node 2), child (1,1,1) interior (node 3).
    // node 1 (0..16)^3: brick (0,0,0) uniform (node 4), brick (1,1,0) uniform with a hole (node 5).
    // node 3 (16..32)^3: brick (3,3,3) = (28..32)^3 with a material run of 3 entries (node 6).
    const size_t NT = 7;
    Node* t3 = (Node*)aligned_alloc(16, NT * sizeof(Node));
    t3[0] = interior((1ull << slot(0, 0, 0)) | (1ull << slot(1, 0, 0)) | (1ull << slot(1, 1, 1)), 1);
    t3[1] = interior((1ull << slot(0, 0, 0)) | (1ull << slot(1, 1, 0)), 4);
    t3[2] = solid(3);
    t3[3] = interior(1ull << slot(3, 3, 3), 6);
    t3[4] = Node{~0ull, 0u, K_BRICK | K_UNIFORM | (2u << 16)};
    t3[5] = Node{~0ull ^ 2ull, 0u, K_BRICK | K_UNIFORM | (1u << 16)};
    t3[6] = Node{0x8000000000000003ull, 0u, K_BRICK};
    const auto superseded = [&](const std::vector<ShapeRec>& tab, const int32_t lo[3], const int32_t hi[3], uint64_t* gn, uint64_t* gm) {
        PatchAnchor a = patch_anchor(t3, 3, lo, hi);
        a.whole = false;
        shapes_superseded(t3, 3, a, tab.data(), (int32_t)tab.size(), gn, gm);
        return a;
    };
    uint64_t gn = 0, gm = 0;
    {  // a box that is exactly the first 16^3: the root's block, and the whole subtree of node 1
        const int32_t lo[3] = {0, 0, 0}, hi[3] = {16, 16, 16};
        const PatchAnchor a = superseded({box(0, 0, 0, 16, 16, 16, 1)}, lo, hi, &gn, &gm);
        CHECK(a.node == 0 && a.depth == 0 && gn == 3 + 2 && gm == 0);
    }
    {  // one voxel in the brick with a material run: the anchor is its parent
        const int32_t lo[3] = {29, 29, 29}, hi[3] = {30, 30, 30};
        const PatchAnchor a = superseded({box(29, 29, 29, 30, 30, 30, 0)}, lo, hi, &gn, &gm);
        CHECK(a.node == 3 && a.depth == 1 && a.o[0] == 16 && gn == 1 && gm == 3);
    }
    {  // a ball around the corner (16, 16, 16): cuts nodes 1 and 3 and the SOLID child, reaches none of their bricks
        const int32_t lo[3] = {15, 15, 15}, hi[3] = {18, 18, 18};
        const PatchAnchor a = superseded({ball(16, 16, 16, 3, 2)}, lo, hi, &gn, &gm);
        CHECK(a.node == 0 && gn == 3 + 2 + 1 && gm == 0);
    }
    {  // a bounding box equal to the extent with nothing inside the early shape's reach but node 3's brick
        const int32_t lo[3] = {0, 0, 0}, hi[3] = {64, 64, 64};
        const PatchAnchor a = superseded({ball(32, 32, 32, 27, 1), box(0, 0, 0, 64, 64, 64, 0), ball(40, 40, 40, 16 * 16 * 3 - 1, 0)}, lo, hi,
                                         &gn, &gm);
        // the last ball cuts the root child (1,1,1) alone among the stored ones — the box behind it is never reached
        // there — and holds its brick (28..32)^3; the children it does not touch fall to the box, which holds them whole
        CHECK(a.node == 0 && gn == 3 + 2 + 1 && gm == 3);
    }
    free(t3);

    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("shapes patch plan sanitize ok\n");
    return 0;
}
