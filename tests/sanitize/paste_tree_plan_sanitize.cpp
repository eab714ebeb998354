// paste_tree_plan_sanitize.cpp — the host half of svo_tree_patch_tree_gpu under AddressSanitizer + UBSan:
// svo_paste_cell.h's paste_relation and paste_voxel against brute force over the voxels, for every aligned cell of every
// level of a 64^3 destination against a 64^3 and a 16^3 source — offsets of 0, of a multiple of 16, of a multiple of 4
// only, of 1 / 2 / 3 mixed per axis and negative ones, both modes, with every id in view and with one id out of it — and
// svo_plan.cpp's paste_plan (the checks) and paste_superseded (the garbage walk) over the same host images.  The trees are
// built by the host builder from svo_world puts; their arrays are copied into heap arrays of their exact sizes, so that a
// read past them is reported.  The model is dense: what svo_tree_get_block reads from the trees, voxel by voxel.
// Built and run by tests/test_paste_tree_plan_host.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../raytracing_test_amd/csrc/svo_plan.h"

using namespace svo;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (fails < 50) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// a host tree with its arrays in exact-size heap copies and its content as a dense array of the tree's own ids
struct HostTree {
    svo_tree* t = nullptr;
    Node* nodes = nullptr;
    uint16_t* mats = nullptr;
    int E = 0;
    std::vector<uint16_t> dense;
    PasteTree view() const { return PasteTree{nodes, mats, t->levels}; }
    uint16_t at(int x, int y, int z) const { return dense[((size_t)z * E + y) * E + x]; }
    ~HostTree() {
        free(nodes);
        free(mats);
        delete t;  // (never uploaded: svo_tree_destroy, which also releases the device side, lives in a HIP file)
    }
};

// fill: per voxel, the material 1..4 to put (0: none).  The trees number their materials in the order of first use, each its
// own way: ids are numbers and the palettes are not compared, in the model as in the paste
template <class F>
static void build(HostTree& h, int levels, F fill) {
    svo_world* w = nullptr;
    CHECK(svo_world_create(levels, &w) == SVO_OK);
    h.E = 1 << (2 * levels);
    const auto put = [&](int x, int y, int z, uint32_t m) {
        const svo_block b{0u, (uint64_t)(1000 + m), 0.0f};
        CHECK(svo_put_block(w, x, y, z, &b, levels + 1) == SVO_OK);
    };
    std::vector<uint16_t> want((size_t)h.E * h.E * h.E);
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) want[((size_t)z * h.E + y) * h.E + x] = (uint16_t)fill(x, y, z);
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) {
                const uint16_t m = want[((size_t)z * h.E + y) * h.E + x];
                if (m) put(x, y, z, m);
            }
    CHECK(svo_build(w, &h.t) == SVO_OK);
    svo_world_destroy(w);
    h.nodes = (Node*)aligned_alloc(16, h.t->nodes.size() * sizeof(Node));
    memcpy(h.nodes, h.t->nodes.data(), h.t->nodes.size() * sizeof(Node));
    h.mats = (uint16_t*)malloc(h.t->mats.empty() ? 1 : h.t->mats.size() * sizeof(uint16_t));
    if (!h.t->mats.empty()) memcpy(h.mats, h.t->mats.data(), h.t->mats.size() * sizeof(uint16_t));
    h.dense.resize(want.size());
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) {
                svo_block b;
                uint32_t id = 0;
                CHECK(svo_tree_get_block(h.t, x, y, z, &b, &id) == SVO_OK);
                h.dense[((size_t)z * h.E + y) * h.E + x] = (uint16_t)id;
                CHECK(tree_voxel(h.view(), (uint32_t)x, (uint32_t)y, (uint32_t)z) == id);
            }
}

static int count_kind(const HostTree& h, uint32_t kind) {
    int n = 0;
    for (const Node& nd : h.t->nodes) n += node_kind(nd.info) == kind;
    return n;
}

// records and material entries of the subtree of node ni, the node itself not counted
static void subtree(const Node* nodes, uint32_t ni, uint64_t* nn, uint64_t* nm) {
    const Node& n = nodes[ni];
    if (node_kind(n.info) == K_SOLID) return;
    if (node_kind(n.info) == K_BRICK) {
        if (!(n.info & K_UNIFORM)) *nm += (uint64_t)__builtin_popcountll(n.mask);
        return;
    }
    const int c = __builtin_popcountll(n.mask);
    *nn += (uint64_t)c;
    for (int i = 0; i < c; i++) subtree(nodes, n.ref + (uint32_t)i, nn, nm);
}

struct Case {
    bool whole_src;
    int so[3], n[3], d[3];
};

static int64_t seen[3];  // OUT / IN / CUT over everything checked
static int64_t in_nonzero, in_zero, out_in_box;

// every aligned cell of every level of dst, and every voxel, for one paste
static void check_paste(const HostTree& D, const HostTree& S, const Case& c, uint32_t flags, const uint32_t* bits) {
    PastePlan plan;
    CHECK(paste_plan(D.t->levels, S.t->levels, c.whole_src ? nullptr : c.so, c.n[0], c.n[1], c.n[2], c.d, flags, &plan) == PASTE_OK);
    PasteRec R = plan.rec;
    R.in_view = bits;
    const int E = D.E;
    const bool keep = flags & SVO_PASTE_KEEP_EMPTY;
    // the model, voxel by voxel
    std::vector<uint16_t> model(D.dense), decided((size_t)E * E * E, 0);
    for (int z = R.lo[2]; z < R.hi[2]; z++)
        for (int y = R.lo[1]; y < R.hi[1]; y++)
            for (int x = R.lo[0]; x < R.hi[0]; x++) {
                const uint16_t s = S.at(x + R.shift[0], y + R.shift[1], z + R.shift[2]);
                if (keep && s == 0) continue;
                const bool in_view = !bits || ((bits[s >> 5] >> (s & 31u)) & 1u);
                model[((size_t)z * E + y) * E + x] = in_view ? s : 0;
                decided[((size_t)z * E + y) * E + x] = 1;
            }
    const PasteTree sv = S.view(), dv = D.view();
    int k = 1;
    for (int cs = 4; cs <= E; cs *= 4, k++)
        for (int z = 0; z < E; z += cs)
            for (int y = 0; y < E; y += cs)
                for (int x = 0; x < E; x += cs) {
                    uint32_t id = 77u;
                    const uint32_t rel = paste_relation(R, sv, x, y, z, cs, k, &id);
                    seen[rel]++;
                    if (rel == PASTE_CUT) continue;
                    bool agree = true, unchanged = true, all_decided = true;
                    for (int c2 = z; c2 < z + cs; c2++)
                        for (int b = y; b < y + cs; b++)
                            for (int a = x; a < x + cs; a++) {
                                const size_t i = ((size_t)c2 * E + b) * E + a;
                                agree = agree && model[i] == id;
                                unchanged = unchanged && model[i] == D.dense[i];
                                all_decided = all_decided && decided[i];
                            }
                    if (rel == PASTE_IN) {
                        CHECK(agree && all_decided);
                        (id ? in_nonzero : in_zero)++;
                    } else {
                        CHECK(unchanged);
                        bool meets = true;
                        for (int a = 0; a < 3; a++) {
                            const int o = a == 0 ? x : (a == 1 ? y : z);
                            meets = meets && o + cs > R.lo[a] && o < R.hi[a];
                        }
                        out_in_box += meets;
                    }
                }
    for (int z = 0; z < E; z++)
        for (int y = 0; y < E; y++)
            for (int x = 0; x < E; x++) {
                const size_t i = ((size_t)z * E + y) * E + x;
                CHECK(paste_voxel(R, sv, dv, x, y, z) == model[i]);
                uint32_t id = 77u;
                CHECK(paste_takes(R, sv, x, y, z, &id) == (bool)decided[i]);
            }
    // the garbage walk over the same cells: it reads nothing outside the arrays and counts no more than the tree holds
    PatchAnchor a = patch_anchor(D.nodes, D.t->levels, R.lo, R.hi);
    a.whole = false;
    uint64_t gn = 0, gm = 0, an = 0, am = 0;
    paste_superseded(D.nodes, D.t->levels, a, R, sv, &gn, &gm);
    subtree(D.nodes, a.node, &an, &am);
    CHECK(gn <= an && gm <= am);
    CHECK(gn >= (uint64_t)__builtin_popcountll(D.nodes[a.node].mask));  // the anchor's child block at least
    if (plan.whole) CHECK(gn == an && gm == am);                          // REPLACE over the extent: IN or CUT everywhere
}

int main() {
    // dst: random content, a 16^3 of material 3, an empty 16^3, a full brick
    HostTree D, S64, S16, SE;
    build(D, 3, [](int x, int y, int z) -> uint32_t {
        if (x >= 16 && x < 32 && y >= 32 && y < 48 && z >= 0 && z < 16) return 3u;
        if (x >= 48 && y >= 48 && z >= 48) return 0u;
        if (x >= 8 && x < 12 && y >= 4 && y < 8 && z >= 40 && z < 44) return 2u;
        const uint32_t r = rnd();
        return (r & 7u) < 2u ? 1u + ((r >> 3) & 3u) : 0u;
    });
    // src: a 16^3 of material 4 at the origin, an empty 32 x 16 x 16, a 4^3 of material 1, a sparse octant, random elsewhere
    build(S64, 3, [](int x, int y, int z) -> uint32_t {
        if (x < 16 && y < 16 && z < 16) return 4u;
        if (x >= 32 && y >= 16 && y < 32 && z >= 32 && z < 48) return 0u;
        if (x >= 20 && x < 24 && y >= 20 && y < 24 && z >= 20 && z < 24) return 1u;
        const uint32_t r = rnd();
        if (x >= 32 && y >= 32 && z >= 32) return (r & 255u) == 0u ? 2u : 0u;
        return (r & 3u) == 0u ? 1u + ((r >> 3) & 3u) : 0u;
    });
    // the prefab: a solid 8 x 8 x 8 corner, an empty brick row, random elsewhere
    build(S16, 2, [](int x, int y, int z) -> uint32_t {
        if (x < 8 && y < 8 && z < 8) return 2u;
        if (y >= 12) return 0u;
        const uint32_t r = rnd();
        return (r & 1u) ? 1u + ((r >> 3) & 3u) : 0u;
    });
    build(SE, 2, [](int, int, int) -> uint32_t { return 0u; });
    CHECK(count_kind(D, K_SOLID) > 0 && count_kind(S64, K_SOLID) > 0 && count_kind(S16, K_SOLID) > 0);
    CHECK(D.t->palette.size() == 5 && S64.t->palette.size() == 5 && S16.t->palette.size() == 5 && SE.t->palette.size() == 1);

    const Case c64[] = {
        {true, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}},                // the extent, offset 0 on every grid
        {false, {8, 12, 16}, {24, 20, 28}, {8, 12, 16}},        // offset 0, a box on no grid
        {false, {0, 16, 0}, {32, 32, 48}, {32, 0, 16}},         // a multiple of 16
        {false, {0, 0, 0}, {16, 16, 16}, {48, 32, 16}},         // the K_SOLID 16^3 onto an aligned cell
        {false, {4, 8, 12}, {28, 24, 20}, {16, 12, 24}},        // a multiple of 4 only
        {false, {10, 9, 8}, {30, 29, 31}, {11, 11, 11}},        // (1, 2, 3)
        {false, {0, 0, 0}, {16, 16, 16}, {25, 23, 26}},         // the K_SOLID 16^3 across the centre, off every grid
        {false, {33, 30, 21}, {25, 30, 40}, {2, 7, 18}},        // negative, mixed per axis
        {false, {32, 16, 32}, {32, 16, 16}, {5, 41, 3}},        // src's empty region
        {false, {21, 22, 20}, {1, 1, 1}, {38, 5, 19}},          // one voxel
        {false, {1, 2, 3}, {63, 62, 61}, {0, 1, 2}},            // nearly everything, shifted by (-1, -1, -1)
    };
    const Case c16[] = {
        {true, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}},   {true, {0, 0, 0}, {0, 0, 0}, {16, 32, 48}}, {true, {0, 0, 0}, {0, 0, 0}, {20, 8, 36}},
        {true, {0, 0, 0}, {0, 0, 0}, {21, 6, 35}}, {true, {0, 0, 0}, {0, 0, 0}, {48, 47, 1}},  {false, {3, 2, 1}, {9, 10, 11}, {30, 31, 29}},
        {false, {0, 0, 0}, {8, 8, 8}, {13, 22, 7}},
    };
    const uint32_t no2 = 0x1Bu;  // ids 0, 1, 3, 4 in view: 2 is stored empty
    for (uint32_t flags : {(uint32_t)SVO_PASTE_REPLACE, (uint32_t)SVO_PASTE_KEEP_EMPTY})
        for (const uint32_t* bits : {(const uint32_t*)nullptr, &no2}) {
            for (const Case& c : c64) check_paste(D, S64, c, flags, bits);
            for (const Case& c : c16) check_paste(D, S16, c, flags, bits);
            check_paste(D, SE, c16[3], flags, bits);
            check_paste(D, D, c64[5], flags, bits);  // src == dst
        }
    CHECK(seen[PASTE_OUT] > 0 && seen[PASTE_IN] > 0 && seen[PASTE_CUT] > 0);
    CHECK(in_nonzero > 0 && in_zero > 0 && out_in_box > 0);  // uniform regions were recognised off the grid, and KEEP_EMPTY's OUT

    {  // exact garbage counts: the aligned K_SOLID 16^3 over an aligned cell supersedes the root's block and that cell's subtree
        PastePlan plan;
        const int32_t so[3] = {0, 0, 0}, d[3] = {48, 32, 16};
        CHECK(paste_plan(3, 3, so, 16, 16, 16, d, SVO_PASTE_REPLACE, &plan) == PASTE_OK && !plan.whole);
        PatchAnchor a = patch_anchor(D.nodes, 3, plan.rec.lo, plan.rec.hi);
        a.whole = false;
        CHECK(a.node == 0 && a.depth == 0);
        uint64_t gn = 0, gm = 0, sn = 0, sm = 0;
        paste_superseded(D.nodes, 3, a, plan.rec, S64.view(), &gn, &gm);
        const uint32_t sl = (1u << 4) | (2u << 2) | 3u;
        CHECK((D.nodes[0].mask >> sl) & 1ull);
        subtree(D.nodes, D.nodes[0].ref + (uint32_t)__builtin_popcountll(D.nodes[0].mask & ((1ull << sl) - 1ull)), &sn, &sm);
        CHECK(sn > 0 && gn == (uint64_t)__builtin_popcountll(D.nodes[0].mask) + sn && gm == sm);
        // src's empty region (two absent 16^3) under KEEP_EMPTY, off every grid: the anchor's block alone
        const int32_t eo[3] = {32, 16, 32}, ed[3] = {5, 41, 3};
        CHECK(paste_plan(3, 3, eo, 32, 16, 16, ed, SVO_PASTE_KEEP_EMPTY, &plan) == PASTE_OK);
        a = patch_anchor(D.nodes, 3, plan.rec.lo, plan.rec.hi);
        a.whole = false;
        paste_superseded(D.nodes, 3, a, plan.rec, S64.view(), &gn, &gm);
        CHECK(a.node == 0);
        CHECK(gn == (uint64_t)__builtin_popcountll(D.nodes[a.node].mask) && gm == 0);
        // an empty prefab is a root with mask 0, which counts as mixed at its own level: its 16^3 descends, and comes out
        // untouched at the bricks (conservative on purpose)
        CHECK(paste_plan(3, 2, nullptr, 0, 0, 0, d, SVO_PASTE_KEEP_EMPTY, &plan) == PASTE_OK);
        uint32_t id;
        CHECK(paste_relation(plan.rec, SE.view(), 48, 32, 16, 16, 2, &id) == PASTE_CUT);
        CHECK(paste_relation(plan.rec, SE.view(), 52, 36, 20, 4, 1, &id) == PASTE_OUT);
    }

    {  // paste_plan's checks
        PastePlan plan;
        const int32_t o[3] = {0, 0, 0}, p[3] = {60, 0, 0}, neg[3] = {0, -1, 0}, far[3] = {0x7FFFFFFF, 0, 0};
        CHECK(paste_plan(3, 3, nullptr, -5, 0, 7, o, SVO_PASTE_REPLACE, &plan) == PASTE_OK && plan.whole);
        CHECK(plan.rec.hi[0] == 64 && plan.rec.hi[2] == 64 && plan.rec.shift[1] == 0 && plan.rec.keep_empty == 0);
        CHECK(paste_plan(3, 3, nullptr, 0, 0, 0, o, SVO_PASTE_KEEP_EMPTY, &plan) == PASTE_OK && !plan.whole && plan.rec.keep_empty == 1);
        CHECK(paste_plan(3, 2, nullptr, 0, 0, 0, p, 0, &plan) == PASTE_DST_EXTENT);
        CHECK(paste_plan(3, 2, nullptr, 0, 0, 0, neg, 0, &plan) == PASTE_DST_EXTENT);
        CHECK(paste_plan(2, 3, nullptr, 0, 0, 0, o, 0, &plan) == PASTE_DST_EXTENT);  // src's extent does not fit dst
        CHECK(paste_plan(3, 3, o, 4, 0, 4, o, 0, &plan) == PASTE_DIM);
        CHECK(paste_plan(3, 3, o, 4, 4, -4, o, 0, &plan) == PASTE_DIM);
        CHECK(paste_plan(3, 3, p, 5, 4, 4, o, 0, &plan) == PASTE_SRC_EXTENT);
        CHECK(paste_plan(3, 3, neg, 4, 4, 4, o, 0, &plan) == PASTE_SRC_EXTENT);
        CHECK(paste_plan(3, 3, far, 0x7FFFFFFF, 4, 4, o, 0, &plan) == PASTE_SRC_EXTENT);  // no int32 wrap
        CHECK(paste_plan(3, 3, o, 4, 4, 4, far, 0, &plan) == PASTE_DST_EXTENT);
        CHECK(paste_plan(3, 3, o, 4, 4, 4, o, 2, &plan) == PASTE_FLAGS);
        CHECK(paste_plan(3, 3, o, 4, 4, 4, o, 0x80000001u, &plan) == PASTE_FLAGS);
        CHECK(paste_plan(3, 3, p, 4, 64, 64, o, 0, &plan) == PASTE_OK && plan.rec.shift[0] == 60 && plan.rec.hi[0] == 4 && !plan.whole);
        std::vector<uint32_t> bits;
        const std::vector<Material> pal = {Material{0, ~0ull, 0.0f}, Material{1, 5, 0.0f}, Material{1 | 0x10, 6, 0.0f}};  // 2: liquid
        CHECK(!paste_view_bits(pal, SVO_VIEW_SOLID, &bits) && bits.size() == 1 && bits[0] == 3u);
        CHECK(paste_view_bits(pal, SVO_VIEW_ALL, &bits) && bits[0] == 7u);
    }

    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("paste tree plan sanitize ok: %lld OUT, %lld IN, %lld CUT cells\n", (long long)seen[0], (long long)seen[1], (long long)seen[2]);
    return 0;
}
