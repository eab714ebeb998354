// diff_voxels_plan_sanitize.cpp — the host half of svo_tree_diff_gpu under AddressSanitizer + UBSan: svo_diff_pair.h's pair
// logic (the side state, the state of a child slot, the id of a brick-depth voxel, the classification "both uniform"),
// which the kernels share, walked by a plain recursive driver over record arrays built by hand, against brute force over
// all 16^3 voxels.  Two 2-level trees carry every ordered pair of seven side shapes at one slot each (49 of the 64 slots):
// empty, a K_SOLID child of id 2, one of id 3, a partial one-material brick, a mixed brick, a brick with mask 0 under a set
// slot, and a full one-material brick that stayed a brick; then a K_SOLID root, an empty root and a tree against itself.
// The count and the list are compared for the whole extent and for boxes off the grid.  The arrays are allocated at their
// exact sizes, so a read past a child block or a material run is reported.  Built and run by
// tests/test_diff_voxels_plan_host.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../raytracing_test_amd/csrc/svo_diff_pair.h"
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

constexpr int32_t L = 2, E = 16;
enum Shape { EMPTY = 0, SOLID2, SOLID3, PARTIAL, MIXED, ZERO, FULL_BRICK, N_SHAPES };

// the ids of the 64 voxels of shape `sh` at slot `slot` of tree `side` (0: a, 1: b): the content, stated apart from the records
static void shape_ids(int sh, int slot, int side, uint16_t id[64]) {
    for (int v = 0; v < 64; v++) {
        const uint64_t partial = 0x0F0F00FF00F0F0F1ull, mixed = 0x8123456789ABCDEFull ^ (side ? (1ull << 5) | (1ull << 40) : 0ull);
        switch (sh) {
            case SOLID2: id[v] = 2; break;
            case SOLID3: id[v] = 3; break;
            case PARTIAL: id[v] = ((partial >> v) & 1ull) ? 4 : 0; break;
            case MIXED: id[v] = ((mixed >> v) & 1ull) ? (uint16_t)(1 + (v + slot * side) % 5) : 0; break;
            case FULL_BRICK: id[v] = 2; break;
            default: id[v] = 0;
        }
    }
}

struct Tree {  // exact-size arrays
    Node* nodes = nullptr;
    uint16_t* mats = nullptr;
    uint16_t dense[E][E][E];  // [z][y][x]
    ~Tree() {
        free(nodes);
        free(mats);
    }
};

// a 2-level tree whose slot s holds shapes[s]
static void build(Tree& t, const int shapes[64], int side) {
    std::vector<Node> nodes(1);
    std::vector<uint16_t> mats;
    uint64_t rmask = 0;
    memset(t.dense, 0, sizeof(t.dense));
    for (int s = 0; s < 64; s++) {
        uint16_t id[64];
        shape_ids(shapes[s], s, side, id);
        for (int v = 0; v < 64; v++)
            t.dense[(s >> 4) * 4 + (v >> 4)][((s >> 2) & 3) * 4 + ((v >> 2) & 3)][(s & 3) * 4 + (v & 3)] = id[v];
        if (shapes[s] == EMPTY) continue;
        rmask |= 1ull << s;
        uint64_t mask = 0;
        for (int v = 0; v < 64; v++)
            if (id[v]) mask |= 1ull << v;
        switch (shapes[s]) {
            case SOLID2: nodes.push_back(Node{~0ull, 0u, K_SOLID | (2u << 16)}); break;
            case SOLID3: nodes.push_back(Node{~0ull, 0u, K_SOLID | (3u << 16)}); break;
            case PARTIAL: nodes.push_back(Node{mask, 0u, K_BRICK | K_UNIFORM | (4u << 16)}); break;
            case FULL_BRICK: nodes.push_back(Node{~0ull, 0u, K_BRICK | K_UNIFORM | (2u << 16)}); break;
            case ZERO: nodes.push_back(Node{0ull, 0u, K_BRICK}); break;
            default:  // MIXED
                nodes.push_back(Node{mask, (uint32_t)mats.size(), K_BRICK});
                for (int v = 0; v < 64; v++)
                    if (id[v]) mats.push_back(id[v]);
        }
    }
    nodes[0] = Node{rmask, 1u, K_INTERIOR};
    t.nodes = (Node*)malloc(sizeof(Node) * nodes.size());
    memcpy(t.nodes, nodes.data(), sizeof(Node) * nodes.size());
    t.mats = (uint16_t*)malloc(sizeof(uint16_t) * (mats.size() ? mats.size() : 1));
    if (!mats.empty()) memcpy(t.mats, mats.data(), sizeof(uint16_t) * mats.size());
}

// a one-record tree: a K_SOLID root of id u, or (u = 0) an interior root with mask 0
static void build_root(Tree& t, uint32_t u) {
    t.nodes = (Node*)malloc(sizeof(Node));
    t.nodes[0] = u ? Node{~0ull, 0u, K_SOLID | (u << 16)} : Node{0ull, 0u, K_INTERIOR};
    for (auto& plane : t.dense)
        for (auto& row : plane)
            for (auto& x : row) x = (uint16_t)u;
}

struct Ent {
    int32_t x, y, z;
    uint32_t id;
    bool operator==(const Ent& o) const { return x == o.x && y == o.y && z == o.z && id == o.id; }
};

// the driver: the pair (a, b) of the region of edge s at (x, y, z), depth d; appends its differing voxels in key order
static uint64_t walk(const Tree& A, const Tree& Bt, const Node& a, const Node& b, int32_t x, int32_t y, int32_t z, int32_t s, int d,
                     const ListBox& B, std::vector<Ent>& out) {
    const bool brick_depth = d == L - 1;
    uint32_t ua, ub;
    if (diff_both_uniform(a, b, brick_depth, &ua, &ub)) {  // closed form, unranked
        if (ua == ub) return 0;
        const uint64_t n = list_clip_volume(x, y, z, s, B);
        for (uint64_t q = 0; q < n; q++) {
            int32_t p[3] = {x, y, z};
            list_unrank(p, s, B, q);
            out.push_back(Ent{p[0], p[1], p[2], ub});
        }
        return n;
    }
    uint64_t total = 0;
    if (brick_depth) {
        for (uint32_t v = 0; v < 64; v++) {
            const int32_t px = x + (int32_t)(v & 3u), py = y + (int32_t)((v >> 2) & 3u), pz = z + (int32_t)(v >> 4);
            if (!list_clip_volume(px, py, pz, 1, B)) continue;
            const uint32_t ia = diff_voxel_id(a, A.mats, v), ib = diff_voxel_id(b, Bt.mats, v);
            if (ia != ib) {
                out.push_back(Ent{px, py, pz, ib});
                total++;
            }
        }
        return total;
    }
    const uint64_t cand = diff_slot_mask(a) | diff_slot_mask(b);
    const int32_t cs = s / 4;
    for (uint32_t sl = 0; sl < 64; sl++) {
        const int32_t cx = x + (int32_t)(sl & 3u) * cs, cy = y + (int32_t)((sl >> 2) & 3u) * cs, cz = z + (int32_t)(sl >> 4) * cs;
        if (!((cand >> sl) & 1ull) || !list_clip_volume(cx, cy, cz, cs, B)) continue;
        total += walk(A, Bt, diff_child(a, A.nodes, sl), diff_child(b, Bt.nodes, sl), cx, cy, cz, cs, d + 1, B, out);
    }
    return total;
}

static uint64_t key(int32_t x, int32_t y, int32_t z) {
    uint64_t k = 0;
    for (int d = 0; d < L; d++) {
        const int sh = 2 * (L - 1 - d);
        k = (k << 6) | (uint64_t)((((z >> sh) & 3) << 4) | (((y >> sh) & 3) << 2) | ((x >> sh) & 3));
    }
    return k;
}

static void check(const Tree& A, const Tree& Bt, const int32_t* o, int32_t nx, int32_t ny, int32_t nz, int64_t expect = -1) {
    ListBox B;
    CHECK(list_box(L, o, nx, ny, nz, &B) == LIST_BOX_OK);
    std::vector<Ent> want;
    for (int32_t z = B.lo[2]; z < B.hi[2]; z++)
        for (int32_t y = B.lo[1]; y < B.hi[1]; y++)
            for (int32_t x = B.lo[0]; x < B.hi[0]; x++)
                if (A.dense[z][y][x] != Bt.dense[z][y][x]) want.push_back(Ent{x, y, z, Bt.dense[z][y][x]});
    std::sort(want.begin(), want.end(), [](const Ent& p, const Ent& q) { return key(p.x, p.y, p.z) < key(q.x, q.y, q.z); });
    std::vector<Ent> got;
    const uint64_t n = walk(A, Bt, A.nodes[0], Bt.nodes[0], 0, 0, 0, E, 0, B, got);
    CHECK(n == want.size() && got.size() == want.size());
    CHECK(got == want);
    if (expect >= 0) CHECK((int64_t)n == expect);
}

int main() {
    {  // the synthesised sides and the classification
        uint32_t u = 9, ua, ub;
        CHECK(diff_side_uniform(diff_uniform(0), false, &u) && u == 0);
        CHECK(diff_side_uniform(diff_uniform(5), true, &u) && u == 5);
        CHECK(diff_slot_mask(diff_uniform(0)) == 0 && diff_slot_mask(diff_uniform(7)) == ~0ull);
        const Node zero_brick{0ull, 0u, K_BRICK}, zero_interior{0ull, 0u, K_INTERIOR}, full_brick{~0ull, 0u, K_BRICK | K_UNIFORM | (2u << 16)};
        CHECK(diff_side_uniform(zero_brick, true, &u) && u == 0 && diff_side_uniform(zero_interior, false, &u) && u == 0);
        CHECK(!diff_side_uniform(full_brick, true, &u));  // read for what it stores
        CHECK(diff_voxel_id(full_brick, nullptr, 63) == 2 && diff_voxel_id(zero_brick, nullptr, 0) == 0);
        CHECK(diff_both_uniform(zero_brick, diff_uniform(3), true, &ua, &ub) && ua == 0 && ub == 3);
        CHECK(!diff_both_uniform(full_brick, diff_uniform(2), true, &ua, &ub));
        const Node child = diff_child(diff_uniform(6), nullptr, 17);  // below a uniform side nothing is read
        CHECK(diff_side_uniform(child, true, &u) && u == 6);
    }
    int sa[64], sb[64];
    for (int s = 0; s < 64; s++) {
        sa[s] = s < N_SHAPES * N_SHAPES ? s / N_SHAPES : EMPTY;
        sb[s] = s < N_SHAPES * N_SHAPES ? s % N_SHAPES : EMPTY;
    }
    sa[63] = MIXED;  // and a mixed brick in the last slot of a alone: the end of both arrays
    Tree A, B2, R2, R3, Z;
    build(A, sa, 0);
    build(B2, sb, 1);
    build_root(R2, 2);
    build_root(R3, 3);
    build_root(Z, 0);
    const int32_t boxes[][6] = {{1, 2, 3, 13, 11, 9}, {5, 5, 5, 1, 1, 1}, {3, 0, 7, 6, 16, 2}, {4, 8, 12, 4, 4, 4}, {0, 0, 0, 16, 16, 16},
                                {15, 15, 15, 1, 1, 1}, {2, 6, 1, 11, 3, 14}};
    const Tree* trees[] = {&A, &B2, &R2, &R3, &Z};
    for (const Tree* p : trees)
        for (const Tree* q : trees) {
            check(*p, *q, nullptr, 0, 0, 0, p == q ? 0 : -1);
            for (const auto& b : boxes) check(*p, *q, b, b[3], b[4], b[5], p == q ? 0 : -1);
        }
    check(R2, R3, nullptr, 0, 0, 0, 4096);  // two uniform roots: the clipped volume
    check(R3, Z, nullptr, 0, 0, 0, 4096);
    const int32_t off[3] = {1, 2, 3};
    check(R2, Z, off, 13, 11, 9, 13 * 11 * 9);
    if (fails) return 1;
    printf("diff voxels plan sanitize ok\n");
    return 0;
}
