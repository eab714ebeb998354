// paste_oriented_plan_sanitize.cpp — the host half of svo_tree_patch_tree_oriented_gpu under AddressSanitizer + UBSan:
// svo_paste_cell.h's paste_relation, paste_takes and paste_voxel over a PasteTurn against brute force over the voxels, for
// every aligned cell of every level of a 64^3 destination: all 48 orientations of an off-grid box with three different
// dimensions out of a 16^3 source (both modes, with and without a map that merges two ids and drops one, with every id in
// view and with one out of it) and out of a 64^3 source (the combinations taken in turn), directed boxes over uniform
// regions, src == dst — and svo_plan.cpp's paste_plan (the orientation's checks, dn, the affine map) and paste_superseded
// (the garbage walk) against a walk of the exported image written here.  The trees are built by the host builder from
// svo_world puts; their arrays are copied into heap arrays of their exact sizes, so that a read past them is reported, and
// so is the id map.  The model is dense and written from the content rule: what svo_tree_get_block reads from the trees,
// voxel by voxel, through the index arithmetic of include/svo_rt.h.
// Built and run by tests/test_paste_oriented_plan_host.py.
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

static uint32_t rng_state = 4321u;
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

// fill: per voxel, the material 1..4 to put (0: none); every tree is given all four in the order 1, 2, 3, 4 first, so that
// the ids are the materials
template <class F>
static void build(HostTree& h, int levels, F fill) {
    svo_world* w = nullptr;
    CHECK(svo_world_create(levels, &w) == SVO_OK);
    h.E = 1 << (2 * levels);
    const auto put = [&](int x, int y, int z, uint32_t m) {
        const svo_block b{0u, (uint64_t)(1000 + m), 0.0f};
        CHECK(svo_put_block(w, x, y, z, &b, levels + 1) == SVO_OK);
    };
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) {
                const uint32_t m = fill(x, y, z);
                if (m) put(x, y, z, m);
            }
    CHECK(svo_build(w, &h.t) == SVO_OK);
    svo_world_destroy(w);
    h.nodes = (Node*)aligned_alloc(16, h.t->nodes.size() * sizeof(Node));
    memcpy(h.nodes, h.t->nodes.data(), h.t->nodes.size() * sizeof(Node));
    h.mats = (uint16_t*)malloc(h.t->mats.empty() ? 1 : h.t->mats.size() * sizeof(uint16_t));
    if (!h.t->mats.empty()) memcpy(h.mats, h.t->mats.data(), h.t->mats.size() * sizeof(uint16_t));
    h.dense.resize((size_t)h.E * h.E * h.E);
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) {
                svo_block b;
                uint32_t id = 0;
                CHECK(svo_tree_get_block(h.t, x, y, z, &b, &id) == SVO_OK);
                h.dense[((size_t)z * h.E + y) * h.E + x] = (uint16_t)id;
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

// What the device pass supersedes below node ni, whose record it replaces, counted over the exported image: the node's
// child block; below a child whose cell is IN everything; below one that is CUT the same again; below one that is OUT
// nothing (its record is copied and keeps its subtree).  A brick's material run goes with its record.
static void superseded(const Node* nodes, int levels, const PasteTurn& R, const PasteTree& S, uint32_t ni, int x, int y, int z, int depth,
                       uint64_t* nn, uint64_t* nm) {
    const Node& n = nodes[ni];
    if (node_kind(n.info) == K_SOLID) return;
    if (node_kind(n.info) == K_BRICK) {
        if (!(n.info & K_UNIFORM)) *nm += (uint64_t)__builtin_popcountll(n.mask);
        return;
    }
    const int k = levels - 1 - depth, cs = 1 << (2 * k);
    uint32_t child = n.ref;
    for (int sl = 0; sl < 64; sl++) {
        if (!((n.mask >> sl) & 1ull)) continue;
        const uint32_t c = child++;
        *nn += 1;
        const int cx = x + (sl & 3) * cs, cy = y + ((sl >> 2) & 3) * cs, cz = z + (sl >> 4) * cs;
        uint32_t id;
        const uint32_t rel = paste_relation(R, S, cx, cy, cz, cs, k, &id);
        if (rel == PASTE_IN) subtree(nodes, c, nn, nm);
        else if (rel == PASTE_CUT) superseded(nodes, levels, R, S, c, cx, cy, cz, depth + 1, nn, nm);
    }
}

struct Case {
    int so[3], n[3], d[3];
};

static int64_t seen[3];  // OUT / IN / CUT over everything checked
static int64_t in_nonzero, in_zero, out_in_box, in_by_map, out_by_map, flipped_in;

// every aligned cell of every level of dst, and every voxel, for one paste
static void check_paste(const HostTree& D, const HostTree& S, const Case& c, int o, uint32_t flags, const uint32_t* bits, const uint16_t* map) {
    static const uint8_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const uint8_t* axis = perms[o >> 3];
    const uint8_t flip[3] = {(uint8_t)(o & 1), (uint8_t)((o >> 1) & 1), (uint8_t)((o >> 2) & 1)};
    PastePlan plan;
    CHECK(paste_plan(D.t->levels, S.t->levels, c.so, c.n[0], c.n[1], c.n[2], c.d, flags, &plan, axis, flip) == PASTE_OK);
    PasteTurn R = plan.rec;
    CHECK(R.id_map == nullptr && R.in_view == nullptr);
    R.in_view = bits;
    R.id_map = map;
    const int E = D.E;
    const bool keep = flags & SVO_PASTE_KEEP_EMPTY;
    for (int a = 0; a < 3; a++) CHECK(R.lo[a] == c.d[a] && R.hi[a] == c.d[a] + c.n[axis[a]] && R.axis[a] == axis[a] && R.sign[a] == (flip[a] ? -1 : 1));
    // the model, voxel by voxel, from the content rule
    std::vector<uint16_t> model(D.dense), decided((size_t)E * E * E, 0);
    for (int z = R.lo[2]; z < R.hi[2]; z++)
        for (int y = R.lo[1]; y < R.hi[1]; y++)
            for (int x = R.lo[0]; x < R.hi[0]; x++) {
                const int d[3] = {x - c.d[0], y - c.d[1], z - c.d[2]};
                int s[3] = {-1, -1, -1};
                for (int a = 0; a < 3; a++) s[axis[a]] = c.so[axis[a]] + (flip[a] ? c.n[axis[a]] - 1 - d[a] : d[a]);
                uint16_t id = S.at(s[0], s[1], s[2]);
                if (map) id = map[id];
                if (keep && id == 0) continue;
                const bool in_view = !bits || ((bits[id >> 5] >> (id & 31u)) & 1u);
                model[((size_t)z * E + y) * E + x] = in_view ? id : 0;
                decided[((size_t)z * E + y) * E + x] = 1;
            }
    const PasteTree sv = S.view(), dv = D.view();
    PasteTurn unmapped = R;
    unmapped.id_map = nullptr;
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
                    uint32_t id2;
                    const uint32_t plain = map ? paste_relation(unmapped, sv, x, y, z, cs, k, &id2) : rel;
                    if (rel == PASTE_IN) {
                        CHECK(agree && all_decided);
                        (id ? in_nonzero : in_zero)++;
                        in_by_map += plain == PASTE_CUT;
                        flipped_in += (o & 7) != 0;
                    } else {
                        CHECK(unchanged);
                        bool meets = true;
                        for (int a = 0; a < 3; a++) {
                            const int org = a == 0 ? x : (a == 1 ? y : z);
                            meets = meets && org + cs > R.lo[a] && org < R.hi[a];
                        }
                        out_in_box += meets;
                        out_by_map += plain != PASTE_OUT;
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
    // the garbage walk against the count over the image
    PatchAnchor a = patch_anchor(D.nodes, D.t->levels, R.lo, R.hi);
    a.whole = false;
    uint64_t gn = 0, gm = 0, wn = 0, wm = 0, an = 0, am = 0;
    paste_superseded(D.nodes, D.t->levels, a, R, sv, &gn, &gm);
    superseded(D.nodes, D.t->levels, R, sv, a.node, a.o[0], a.o[1], a.o[2], a.depth, &wn, &wm);
    subtree(D.nodes, a.node, &an, &am);
    CHECK(gn == wn && gm == wm);
    CHECK(gn <= an && gm <= am);
    CHECK(gn >= (uint64_t)__builtin_popcountll(D.nodes[a.node].mask));  // the anchor's child block at least
    if (plan.whole) CHECK(gn == an && gm == am);                          // REPLACE over the extent: IN or CUT everywhere
    if (o == 0 && !map) {  // the identity is the plain paste: the same record, the same answers
        PastePlan pp;
        CHECK(paste_plan(D.t->levels, S.t->levels, c.so, c.n[0], c.n[1], c.n[2], c.d, flags, &pp) == PASTE_OK);
        PasteRec P = pp.rec;
        for (int i = 0; i < 3; i++) CHECK(P.lo[i] == R.lo[i] && P.hi[i] == R.hi[i] && P.shift[i] == R.shift[i] && P.shift[i] == c.so[i] - c.d[i]);
        P.in_view = bits;
        uint64_t pn = 0, pm = 0;
        paste_superseded(D.nodes, D.t->levels, a, P, sv, &pn, &pm);
        CHECK(pn == gn && pm == gm);
        for (int z = 0; z < E; z += 4)
            for (int y = 0; y < E; y += 4)
                for (int x = 0; x < E; x += 4) {
                    uint32_t i1, i2;
                    CHECK(paste_relation(P, sv, x, y, z, 4, 1, &i1) == paste_relation(R, sv, x, y, z, 4, 1, &i2) && i1 == i2);
                }
    }
}

int main() {
    // dst: random content, a 16^3 of material 3, an empty 16^3, a full brick
    HostTree D, S64, S16;
    build(D, 3, [&](int x, int y, int z) -> uint32_t {
        if (x < 4 && y == 0 && z == 0) return (uint32_t)(x + 1);
        if (x >= 16 && x < 32 && y >= 32 && y < 48 && z >= 0 && z < 16) return 3u;
        if (x >= 48 && y >= 48 && z >= 48) return 0u;
        if (x >= 8 && x < 12 && y >= 4 && y < 8 && z >= 40 && z < 44) return 2u;
        const uint32_t r = rnd();
        return (r & 7u) < 2u ? 1u + ((r >> 3) & 3u) : 0u;
    });
    // src: 16^3 of materials 1, 2 and 3 side by side along x at y = z = 16 (the map merges 1 and 2 and drops 3), a 16^3 of
    // 4 beside them, an empty 32 x 16 x 16, a 4^3 of material 1, a sparse octant, random elsewhere
    build(S64, 3, [&](int x, int y, int z) -> uint32_t {
        if (x < 4 && y == 0 && z == 0) return (uint32_t)(x + 1);
        if (y >= 16 && y < 32 && z >= 16 && z < 32) return 1u + (uint32_t)(x >> 4);
        if (x >= 32 && y >= 16 && y < 32 && z >= 32 && z < 48) return 0u;
        if (x >= 20 && x < 24 && y >= 40 && y < 44 && z >= 20 && z < 24) return 1u;
        const uint32_t r = rnd();
        if (x >= 32 && y >= 32 && z >= 32) return (r & 255u) == 0u ? 2u : 0u;
        return (r & 3u) == 0u ? 1u + ((r >> 3) & 3u) : 0u;
    });
    // the prefab: bricks of materials 1 and 2 side by side, a solid 8 x 8 x 8 corner of 3, an empty brick row, random elsewhere
    build(S16, 2, [&](int x, int y, int z) -> uint32_t {
        if (x < 4 && y == 0 && z == 0) return (uint32_t)(x + 1);
        if (x >= 8 && y < 4 && z >= 4 && z < 8) return x < 12 ? 1u : 2u;
        if (x < 8 && y >= 4 && y < 12 && z >= 8) return 3u;
        if (y >= 12) return 0u;
        const uint32_t r = rnd();
        return (r & 1u) ? 1u + ((r >> 3) & 3u) : 0u;
    });
    CHECK(count_kind(D, K_SOLID) > 0 && count_kind(S64, K_SOLID) >= 4 && count_kind(S16, K_SOLID) > 0);
    CHECK(D.t->palette.size() == 5 && S64.t->palette.size() == 5 && S16.t->palette.size() == 5);
    for (const HostTree* h : {&D, &S64, &S16})
        for (int i = 0; i < 4; i++) CHECK(h->at(i, 0, 0) == i + 1);  // ids are the materials

    // the map in a heap array of its exact size: 1 and 2 merge into 1, 3 is dropped, 4 becomes 2
    uint16_t* map = (uint16_t*)malloc(5 * sizeof(uint16_t));
    const uint16_t map_init[5] = {0, 1, 1, 0, 2};
    memcpy(map, map_init, sizeof(map_init));
    const uint32_t no2 = 0x1Bu;  // ids 0, 1, 3, 4 in view: 2 is stored empty

    const Case box16 = {{3, 2, 1}, {9, 10, 11}, {30, 31, 29}}, box16b = {{2, 0, 1}, {13, 11, 14}, {21, 6, 35}};
    const Case box64 = {{10, 9, 8}, {13, 22, 27}, {11, 11, 11}};
    // all 48 orientations of the off-grid box of three different dimensions out of the 16^3 source: both modes, with and
    // without the map; the view table and the second offset in turn
    for (int o = 0; o < 48; o++)
        for (uint32_t flags : {(uint32_t)SVO_PASTE_REPLACE, (uint32_t)SVO_PASTE_KEEP_EMPTY})
            for (const uint16_t* m : {(const uint16_t*)nullptr, (const uint16_t*)map})
                check_paste(D, S16, (o + (int)flags) & 1 ? box16b : box16, o, flags, ((o >> 1) + (m != nullptr)) & 1 ? &no2 : nullptr, m);
    // out of the 64^3 source: all 48, the four combinations of mode and map in turn
    for (int o = 0; o < 48; o++) check_paste(D, S64, box64, o, (o & 1) ? SVO_PASTE_KEEP_EMPTY : SVO_PASTE_REPLACE, (o & 4) ? &no2 : nullptr, (o & 2) ? map : nullptr);
    // directed boxes under a quarter turn about y, a mirror in x and the inversion (and the identity)
    const Case directed[] = {
        {{0, 16, 16}, {64, 16, 16}, {0, 24, 26}},    // the four K_SOLID 16^3 in a row, off the grid across them (quarter turn: along z)
        {{4, 16, 16}, {40, 16, 16}, {11, 33, 6}},    // parts of three of them, off every grid
        {{16, 16, 16}, {16, 16, 16}, {48, 32, 16}},  // one of them onto an aligned cell
        {{32, 16, 32}, {32, 16, 16}, {5, 41, 3}},    // src's empty region
        {{21, 22, 20}, {1, 1, 1}, {38, 5, 19}},      // one voxel
        {{20, 40, 20}, {4, 4, 4}, {17, 30, 41}},     // one src brick off dst's grid
        {{1, 2, 3}, {62, 62, 61}, {1, 0, 2}},        // nearly everything
        {{0, 0, 0}, {64, 64, 64}, {0, 0, 0}},        // the extent
    };
    const int turns[] = {0, 5 * 8 + 4, 1, 7};  // identity; axis (2, 1, 0), flip (0, 0, 1); flip (1, 0, 0); flip (1, 1, 1)
    for (const Case& c : directed)
        for (int o : turns) {
            Case cc = c;
            if (o == 44)  // the turned box, dn = (nz, ny, nx), is moved back inside where it would leave the extent
                for (int a = 0; a < 3; a += 2) cc.d[a] = c.d[a] < 64 - c.n[2 - a] ? c.d[a] : 64 - c.n[2 - a];
            for (uint32_t flags : {(uint32_t)SVO_PASTE_REPLACE, (uint32_t)SVO_PASTE_KEEP_EMPTY})
                check_paste(D, S64, cc, o, flags, nullptr, ((o + (int)flags) & 1) ? map : nullptr);
        }
    // src == dst: a cube turned in place, and onto an overlapping box
    const Case self[] = {{{20, 22, 18}, {20, 20, 20}, {20, 22, 18}}, {{20, 22, 18}, {20, 20, 20}, {27, 17, 25}}, {{10, 9, 8}, {13, 22, 27}, {11, 11, 11}}};
    for (const Case& c : self)
        for (int o : {44, 1, 7, 19, 34})
            check_paste(D, D, c, o, (o & 1) ? SVO_PASTE_KEEP_EMPTY : SVO_PASTE_REPLACE, (o & 2) ? &no2 : nullptr, (o & 4) ? map : nullptr);
    CHECK(seen[PASTE_OUT] > 0 && seen[PASTE_IN] > 0 && seen[PASTE_CUT] > 0);
    CHECK(in_nonzero > 0 && in_zero > 0 && out_in_box > 0 && flipped_in > 0);
    CHECK(in_by_map > 0);   // src cells of different ids that map to one id were one uniform region
    CHECK(out_by_map > 0);  // a region mapped to 0 was skipped under KEEP_EMPTY

    {  // exact garbage counts: a K_SOLID 16^3, turned, over an aligned cell supersedes the root's block and that cell's subtree
        PastePlan plan;
        const int32_t so[3] = {16, 16, 16}, d[3] = {48, 32, 16};
        const uint8_t axis[3] = {2, 1, 0}, flip[3] = {0, 0, 1};
        CHECK(paste_plan(3, 3, so, 16, 16, 16, d, SVO_PASTE_REPLACE, &plan, axis, flip) == PASTE_OK && !plan.whole);
        PatchAnchor a = patch_anchor(D.nodes, 3, plan.rec.lo, plan.rec.hi);
        a.whole = false;
        CHECK(a.node == 0 && a.depth == 0);
        uint64_t gn = 0, gm = 0, sn = 0, sm = 0;
        paste_superseded(D.nodes, 3, a, plan.rec, S64.view(), &gn, &gm);
        const uint32_t sl = (1u << 4) | (2u << 2) | 3u;
        CHECK((D.nodes[0].mask >> sl) & 1ull);
        subtree(D.nodes, D.nodes[0].ref + (uint32_t)__builtin_popcountll(D.nodes[0].mask & ((1ull << sl) - 1ull)), &sn, &sm);
        CHECK(sn > 0 && gn == (uint64_t)__builtin_popcountll(D.nodes[0].mask) + sn && gm == sm);
        uint32_t id = 0;
        CHECK(paste_relation(plan.rec, S64.view(), 48, 32, 16, 16, 2, &id) == PASTE_IN && id == 2u);
        // the same region dropped by the map under KEEP_EMPTY: the anchor's block alone
        const int32_t so3[3] = {32, 16, 16};
        CHECK(paste_plan(3, 3, so3, 16, 16, 16, d, SVO_PASTE_KEEP_EMPTY, &plan, axis, flip) == PASTE_OK);
        plan.rec.id_map = map;
        paste_superseded(D.nodes, 3, a, plan.rec, S64.view(), &gn, &gm);
        CHECK(gn == (uint64_t)__builtin_popcountll(D.nodes[0].mask) && gm == 0);
        CHECK(paste_relation(plan.rec, S64.view(), 48, 32, 16, 16, 2, &id) == PASTE_OUT);
    }

    {  // paste_plan's checks: flags, then the orientation, then the boxes
        PastePlan plan;
        const int32_t o[3] = {0, 0, 0}, p[3] = {60, 0, 0}, far[3] = {0x7FFFFFFF, 0, 0}, at50[3] = {50, 0, 0}, so[3] = {3, 5, 7}, d[3] = {20, 30, 40};
        const uint8_t id3[3] = {0, 1, 2}, none[3] = {0, 0, 0}, xy[3] = {1, 0, 2}, yz[3] = {0, 2, 1}, rep[3] = {0, 0, 2}, big[3] = {0, 1, 3}, f2[3] = {0, 2, 0},
                      all1[3] = {1, 1, 1}, cyc[3] = {1, 2, 0}, f101[3] = {1, 0, 1};
        CHECK(paste_plan(3, 3, o, 4, 4, 4, o, 2, &plan, rep, f2) == PASTE_FLAGS);
        CHECK(paste_plan(3, 3, o, 0, 4, 4, o, 0, &plan, rep, f2) == PASTE_AXIS);
        CHECK(paste_plan(3, 3, o, 0, 4, 4, o, 0, &plan, big, none) == PASTE_AXIS);
        CHECK(paste_plan(3, 3, o, 0, 4, 4, o, 0, &plan, id3, f2) == PASTE_FLIP);
        CHECK(paste_plan(3, 3, o, 0, 4, 4, o, 0, &plan, id3, none) == PASTE_DIM);
        CHECK(paste_plan(3, 3, p, 5, 4, 4, o, 0, &plan, xy, all1) == PASTE_SRC_EXTENT);
        CHECK(paste_plan(3, 3, far, 0x7FFFFFFF, 4, 4, o, 0, &plan, xy, all1) == PASTE_SRC_EXTENT);  // no int32 wrap
        CHECK(paste_plan(3, 3, o, 4, 4, 4, far, 0, &plan, cyc, all1) == PASTE_DST_EXTENT);
        // (2, 16, 2) at x = 50 fits as it is and with y and z exchanged, not with x and y exchanged
        CHECK(paste_plan(3, 3, o, 2, 16, 2, at50, 0, &plan, id3, none) == PASTE_OK);
        CHECK(paste_plan(3, 3, o, 2, 16, 2, at50, 0, &plan, yz, all1) == PASTE_OK && plan.rec.hi[0] == 52 && plan.rec.hi[1] == 2 && plan.rec.hi[2] == 16);
        CHECK(paste_plan(3, 3, o, 2, 16, 2, at50, 0, &plan, xy, none) == PASTE_DST_EXTENT);
        CHECK(paste_plan(3, 3, o, 16, 2, 2, at50, 0, &plan, id3, none) == PASTE_DST_EXTENT);
        CHECK(paste_plan(3, 3, o, 16, 2, 2, at50, 0, &plan, xy, none) == PASTE_OK && plan.rec.hi[0] == 52 && plan.rec.hi[1] == 16);
        // dn and the affine map: dst axes x, y, z run along src's y, z, x, the first and the last against them
        CHECK(paste_plan(3, 3, so, 4, 5, 6, d, SVO_PASTE_KEEP_EMPTY, &plan, cyc, f101) == PASTE_OK && !plan.whole && plan.rec.keep_empty == 1);
        CHECK(plan.rec.hi[0] == 25 && plan.rec.hi[1] == 36 && plan.rec.hi[2] == 44);
        CHECK(plan.rec.sign[0] == -1 && plan.rec.sign[1] == 1 && plan.rec.sign[2] == -1);
        CHECK(plan.rec.shift[0] == 5 + 5 - 1 + 20 && plan.rec.shift[1] == 7 - 30 && plan.rec.shift[2] == 3 + 4 - 1 + 40);
        const int32_t q0[3] = {20, 30, 40}, q1[3] = {24, 35, 43};
        uint32_t s0[3] = {0u, 0u, 0u}, s1[3] = {0u, 0u, 0u};
        paste_source(plan.rec, q0, s0);
        paste_source(plan.rec, q1, s1);
        CHECK(s0[0] == 6 && s0[1] == 9 && s0[2] == 7 && s1[0] == 3 && s1[1] == 5 && s1[2] == 12);
        // the whole extent under REPLACE restarts whatever the orientation; NULL src_origin is still the whole of src
        CHECK(paste_plan(3, 3, nullptr, -5, 0, 7, o, SVO_PASTE_REPLACE, &plan, cyc, f101) == PASTE_OK && plan.whole);
        CHECK(plan.rec.shift[0] == 63 && plan.rec.shift[1] == 0 && plan.rec.shift[2] == 63);
        CHECK(paste_plan(3, 2, nullptr, 0, 0, 0, o, SVO_PASTE_REPLACE, &plan, cyc, f101) == PASTE_OK && !plan.whole && plan.rec.hi[1] == 16);
        // the table: kPasteMixed passes, ids go through it
        PasteTurn R = plan.rec;
        R.id_map = map;
        CHECK(paste_mapped(R, kPasteMixed) == kPasteMixed && paste_mapped(R, 4u) == 2u && paste_mapped(R, 3u) == 0u && paste_mapped(R, 0u) == 0u);
        R.id_map = nullptr;
        CHECK(paste_mapped(R, kPasteMixed) == kPasteMixed && paste_mapped(R, 4u) == 4u);
    }
    free(map);

    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("paste oriented plan sanitize ok: %lld OUT, %lld IN, %lld CUT cells, %lld IN by the map, %lld OUT by the map\n", (long long)seen[0],
           (long long)seen[1], (long long)seen[2], (long long)in_by_map, (long long)out_by_map);
    return 0;
}
