// paste_rule_plan_sanitize.cpp — the host half of svo_tree_patch_tree_rule_gpu under AddressSanitizer + UBSan:
// svo_paste_cell.h's rule_relation, rule_takes and rule_voxel over a PasteRule against brute force over the voxels, for every
// aligned cell of every level of a 64^3 destination and all 12 rules: the identity and two non-trivial orientations of an
// off-grid box with three different dimensions out of a 16^3 and a 64^3 source, with and without a map that merges two ids
// and drops one, with every id in view and with one out of it, directed boxes over uniform regions, src == dst — the rows
// of the cell table that must say OUT on directed cells, svo_plan.cpp's paste_superseded for the record (the garbage walk)
// against a walk of the exported image written here, and paste_rule_check's statuses.  The trees are built by the host
// builder from svo_world puts; their arrays are copied into heap arrays of their exact sizes, so that a read past them is
// reported, and so is the id map.  The model is dense and written from the content rule.
// Built and run by tests/test_paste_rule_plan_host.py.
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

static uint32_t rng_state = 8765u;
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
    for (int z = 0; z < h.E; z++)
        for (int y = 0; y < h.E; y++)
            for (int x = 0; x < h.E; x++) {
                const uint32_t m = fill(x, y, z);
                if (!m) continue;
                const svo_block b{0u, (uint64_t)(1000 + m), 0.0f};
                CHECK(svo_put_block(w, x, y, z, &b, levels + 1) == SVO_OK);
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
// nothing (its record is copied and keeps its subtree)
static void superseded(const Node* nodes, int levels, const PasteRule& R, const PasteTree& S, uint32_t ni, int x, int y, int z, int depth,
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
        const uint32_t rel = rule_relation(R, S, cx, cy, cz, cs, k, &id);
        if (rel == PASTE_IN) subtree(nodes, c, nn, nm);
        else if (rel == PASTE_CUT) superseded(nodes, levels, R, S, c, cx, cy, cz, depth + 1, nn, nm);
    }
}

struct Case {
    int so[3], n[3], d[3];
};

static const uint32_t kRules[12] = {0u, 1u, 4u, 5u, 8u, 9u, 32u, 33u, 36u, 37u, 40u, 41u};
static int64_t seen[3], in_nonzero, in_zero, out_in_box, changed_voxels[64];

static PasteRule make_rule(const HostTree& D, const HostTree& S, const Case& c, int o, uint32_t rule, const uint32_t* bits, const uint16_t* map) {
    static const uint8_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const uint8_t* axis = perms[o >> 3];
    const uint8_t flip[3] = {(uint8_t)(o & 1), (uint8_t)((o >> 1) & 1), (uint8_t)((o >> 2) & 1)};
    PastePlan plan;
    CHECK(paste_rule_check(0u, rule) == RULE_OK);
    CHECK(paste_plan(D.t->levels, S.t->levels, c.so, c.n[0], c.n[1], c.n[2], c.d, 0u, &plan, axis, flip) == PASTE_OK);
    PasteRule R;
    static_cast<PasteTurn&>(R) = plan.rec;
    R.in_view = bits;
    R.id_map = map;
    R.rule = rule;
    R.dst = D.view();
    return R;
}

// every aligned cell of every level of dst, and every voxel, for one rule paste
static void check_rule(const HostTree& D, const HostTree& S, const Case& c, int o, uint32_t rule, const uint32_t* bits, const uint16_t* map) {
    static const uint8_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const uint8_t* axis = perms[o >> 3];
    const uint8_t flip[3] = {(uint8_t)(o & 1), (uint8_t)((o >> 1) & 1), (uint8_t)((o >> 2) & 1)};
    const PasteRule R = make_rule(D, S, c, o, rule, bits, map);
    const int E = D.E;
    const uint32_t A = rule & 3u, B = (rule >> 2) & 3u, C = (rule >> 4) & 3u;
    // the model, voxel by voxel, from the table of include/svo_rt.h
    std::vector<uint16_t> model(D.dense);
    for (int z = R.lo[2]; z < R.hi[2]; z++)
        for (int y = R.lo[1]; y < R.hi[1]; y++)
            for (int x = R.lo[0]; x < R.hi[0]; x++) {
                const int dd[3] = {x - c.d[0], y - c.d[1], z - c.d[2]};
                int s[3] = {-1, -1, -1};
                for (int a = 0; a < 3; a++) s[axis[a]] = c.so[axis[a]] + (flip[a] ? c.n[axis[a]] - 1 - dd[a] : dd[a]);
                uint16_t id = S.at(s[0], s[1], s[2]);
                if (map) id = map[id];
                const uint16_t rs = (!bits || ((bits[id >> 5] >> (id & 31u)) & 1u)) ? id : 0;
                const size_t i = ((size_t)z * E + y) * E + x;
                const uint16_t d = D.dense[i];
                uint16_t r = d;
                if (id != 0 && d == 0) r = A == 1u ? rs : 0;
                else if (id != 0 && d != 0) r = B == 0u ? d : (B == 1u ? rs : 0);
                else if (id == 0 && d != 0) r = C == 0u ? d : 0;
                model[i] = r;
                changed_voxels[rule] += r != d;
            }
    const PasteTree sv = S.view();
    int k = 1;
    for (int cs = 4; cs <= E; cs *= 4, k++)
        for (int z = 0; z < E; z += cs)
            for (int y = 0; y < E; y += cs)
                for (int x = 0; x < E; x += cs) {
                    if (cs == E) continue;  // (the root's own cell is never asked: k <= levels - 1)
                    uint32_t id = 77u;
                    const uint32_t rel = rule_relation(R, sv, x, y, z, cs, k, &id);
                    seen[rel]++;
                    if (rel == PASTE_CUT) continue;
                    bool agree = true, unchanged = true;
                    for (int c2 = z; c2 < z + cs; c2++)
                        for (int b = y; b < y + cs; b++)
                            for (int a = x; a < x + cs; a++) {
                                const size_t i = ((size_t)c2 * E + b) * E + a;
                                agree = agree && model[i] == id;
                                unchanged = unchanged && model[i] == D.dense[i];
                            }
                    bool meets = true, inside = true;
                    for (int a = 0; a < 3; a++) {
                        const int org = a == 0 ? x : (a == 1 ? y : z);
                        meets = meets && org + cs > R.lo[a] && org < R.hi[a];
                        inside = inside && org >= R.lo[a] && org + cs <= R.hi[a];
                    }
                    if (rel == PASTE_IN) {
                        CHECK(agree && inside);
                        (id ? in_nonzero : in_zero)++;
                    } else {
                        CHECK(unchanged);
                        out_in_box += meets;
                    }
                }
    for (int z = 0; z < E; z++)
        for (int y = 0; y < E; y++)
            for (int x = 0; x < E; x++) {
                const size_t i = ((size_t)z * E + y) * E + x;
                CHECK(rule_voxel(R, sv, x, y, z) == model[i]);
                uint32_t id = 77u;
                const bool takes = rule_takes(R, sv, x, y, z, &id);
                if (takes) CHECK(id == model[i]);
                else CHECK(model[i] == D.dense[i]);  // what the rule does not decide stays
                if (model[i] != D.dense[i]) CHECK(takes);
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
}

// one directed 16^3 cell of dst under every rule: the answer the table gives
static void directed_cell(const HostTree& D, const HostTree& S, const int32_t so[3], const int32_t d[3], int src_state, int dst_state) {
    // states: 0 empty, 1 uniform id != 0, 2 mixed
    for (uint32_t rule : kRules) {
        const Case c = {{so[0], so[1], so[2]}, {16, 16, 16}, {d[0], d[1], d[2]}};
        const PasteRule R = make_rule(D, S, c, 0, rule, nullptr, nullptr);
        const uint32_t A = rule & 3u, B = (rule >> 2) & 3u, C = (rule >> 4) & 3u;
        uint32_t id = 77u;
        const uint32_t rel = rule_relation(R, S.view(), d[0], d[1], d[2], 16, 2, &id);
        uint32_t want = PASTE_CUT;
        if (src_state == 0) want = (C == 0u || dst_state == 0) ? PASTE_OUT : PASTE_IN;
        else if (src_state == 1) {
            if (dst_state == 0) want = A == 0u ? PASTE_OUT : PASTE_IN;
            else if (dst_state == 1) want = B == 0u ? PASTE_OUT : PASTE_IN;
            else want = (A == 0u && B == 0u) ? PASTE_OUT : ((A == 1u && B == 1u) || (A == 0u && B == 2u)) ? PASTE_IN : PASTE_CUT;
        } else {
            if (dst_state == 0 && A == 0u) want = PASTE_OUT;
            else if (dst_state == 1 && B == 0u && C == 0u) want = PASTE_OUT;
        }
        CHECK(rel == want);
        // an OUT cell of dst costs the anchor's child block and nothing below it
        if (want == PASTE_OUT) {
            PatchAnchor a = patch_anchor(D.nodes, 3, R.lo, R.hi);
            a.whole = false;
            uint64_t gn = 0, gm = 0;
            paste_superseded(D.nodes, 3, a, R, S.view(), &gn, &gm);
            CHECK(a.node == 0 && gn == (uint64_t)__builtin_popcountll(D.nodes[0].mask) && gm == 0);
        }
    }
}

int main() {
    // dst: random content, a 16^3 of material 3 at (16, 32, 0), an empty 16^3 at (48, 48, 48), a full brick
    HostTree D, S64, S16;
    build(D, 3, [&](int x, int y, int z) -> uint32_t {
        if (x < 4 && y == 0 && z == 0) return (uint32_t)(x + 1);
        if (x >= 16 && x < 32 && y >= 32 && y < 48 && z >= 0 && z < 16) return 3u;
        if (x >= 48 && y >= 48 && z >= 48) return 0u;
        if (x >= 8 && x < 12 && y >= 4 && y < 8 && z >= 40 && z < 44) return 2u;
        const uint32_t r = rnd();
        return (r & 7u) < 2u ? 1u + ((r >> 3) & 3u) : 0u;
    });
    // src: 16^3 of materials 1, 2, 3 and 4 side by side along x at y = z = 16, an empty 32 x 16 x 16 at (32, 16, 32), a
    // 4^3 of material 1, a sparse octant, random elsewhere
    build(S64, 3, [&](int x, int y, int z) -> uint32_t {
        if (x < 4 && y == 0 && z == 0) return (uint32_t)(x + 1);
        if (y >= 16 && y < 32 && z >= 16 && z < 32) return 1u + (uint32_t)(x >> 4);
        if (x >= 32 && y >= 16 && y < 32 && z >= 32 && z < 48) return 0u;
        if (x >= 20 && x < 24 && y >= 40 && y < 44 && z >= 20 && z < 24) return 1u;
        const uint32_t r = rnd();
        if (x >= 32 && y >= 32 && z >= 32) return (r & 255u) == 0u ? 2u : 0u;
        return (r & 3u) == 0u ? 1u + ((r >> 3) & 3u) : 0u;
    });
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

    const Case box16 = {{3, 2, 1}, {9, 10, 11}, {30, 31, 29}};
    const Case box64 = {{10, 9, 8}, {13, 22, 27}, {11, 11, 11}};
    const int turns[3] = {0, 5 * 8 + 4, 3 * 8 + 3};  // identity; axis (2, 1, 0), flip (0, 0, 1); axis (1, 2, 0), flip (1, 1, 0)
    // with and without the map, with and without view bits: the four combinations under every orientation, the two sources
    // taking them in turn, so that each source meets all four under every rule
    for (uint32_t rule : kRules)
        for (int oi = 0; oi < 3; oi++)
            for (int combo = 0; combo < 4; combo++) {
                const uint32_t* bits = (combo & 1) ? &no2 : nullptr;
                const uint16_t* m = (combo & 2) ? map : nullptr;
                if ((oi + combo + (combo >> 1)) & 1) check_rule(D, S64, box64, turns[oi], rule, bits, m);
                else check_rule(D, S16, box16, turns[oi], rule, bits, m);
            }
    // directed boxes, the identity and a quarter turn about y
    const Case directed[] = {
        {{0, 16, 16}, {64, 16, 16}, {0, 24, 26}},    // the four K_SOLID 16^3 in a row, off the grid across them
        {{16, 16, 16}, {16, 16, 16}, {48, 32, 16}},  // one of them onto an aligned cell
        {{32, 16, 32}, {32, 16, 16}, {5, 41, 3}},    // src's empty region
        {{21, 22, 20}, {1, 1, 1}, {38, 5, 19}},      // one voxel
        {{20, 40, 20}, {4, 4, 4}, {17, 30, 41}},     // one src brick off dst's grid
        {{0, 0, 0}, {64, 64, 64}, {0, 0, 0}},        // the extent
    };
    for (const Case& c : directed)
        for (int o : {0, 44}) {
            Case cc = c;
            if (o == 44)
                for (int a = 0; a < 3; a += 2) cc.d[a] = c.d[a] < 64 - c.n[2 - a] ? c.d[a] : 64 - c.n[2 - a];
            for (uint32_t rule : kRules) check_rule(D, S64, cc, o, rule, nullptr, (rule & 4u) ? map : nullptr);
        }
    // src == dst: onto an overlapping box, turned
    const Case self[] = {{{20, 22, 18}, {20, 20, 20}, {27, 17, 25}}, {{10, 9, 8}, {13, 22, 27}, {11, 11, 11}}};
    for (const Case& c : self)
        for (uint32_t rule : kRules) check_rule(D, D, c, (rule & 1u) ? 44 : 0, rule, (rule & 8u) ? &no2 : nullptr, (rule & 32u) ? map : nullptr);
    CHECK(seen[PASTE_OUT] > 0 && seen[PASTE_IN] > 0 && seen[PASTE_CUT] > 0);
    CHECK(in_nonzero > 0 && in_zero > 0 && out_in_box > 0);
    CHECK(changed_voxels[0] == 0);
    for (uint32_t rule : kRules)
        if (rule) CHECK(changed_voxels[rule] > 0);

    {  // the rows that must say OUT, and the others, on directed 16^3 cells.  src: K_SOLID (16, 16, 16), empty (32, 16, 32),
       // mixed (0, 0, 0); dst: empty (48, 48, 48), K_SOLID (16, 32, 0), mixed (32, 0, 32)
        const int32_t s_solid[3] = {16, 16, 16}, s_empty[3] = {32, 16, 32}, s_mixed[3] = {0, 0, 0};
        const int32_t d_empty[3] = {48, 48, 48}, d_solid[3] = {16, 32, 0}, d_mixed[3] = {32, 0, 32};
        CHECK(src_cell(S64.view(), 1, 16, 16, 16) == 2u && src_cell(S64.view(), 1, 32, 16, 32) == 0u && src_cell(S64.view(), 1, 0, 0, 0) == kPasteMixed);
        CHECK(src_cell(D.view(), 1, 48, 48, 48) == 0u && src_cell(D.view(), 1, 16, 32, 0) == 3u && src_cell(D.view(), 1, 32, 0, 32) == kPasteMixed);
        const int32_t* ss[3] = {s_empty, s_solid, s_mixed};
        const int32_t* ds[3] = {d_empty, d_solid, d_mixed};
        for (int si = 0; si < 3; si++)
            for (int di = 0; di < 3; di++) directed_cell(D, S64, ss[si], ds[di], si, di);
    }

    {  // the rule check: flags first, then the bits above 5, then A, B, C
        CHECK(paste_rule_check(0u, 0u) == RULE_OK);
        for (uint32_t rule : kRules) CHECK(paste_rule_check(0u, rule) == RULE_OK && paste_rule_check(1u, rule) == RULE_FLAGS);
        int ok = 0;
        for (uint32_t rule = 0; rule < 64u; rule++) ok += paste_rule_check(0u, rule) == RULE_OK;
        CHECK(ok == 12);
        CHECK(paste_rule_check(2u, 0x40u) == RULE_FLAGS);
        CHECK(paste_rule_check(0u, 0x40u) == RULE_BITS && paste_rule_check(0u, 0x80000000u) == RULE_BITS && paste_rule_check(0u, 0x42u) == RULE_BITS);
        CHECK(paste_rule_check(0u, 2u) == RULE_SRC_ONLY && paste_rule_check(0u, 3u) == RULE_SRC_ONLY && paste_rule_check(0u, 3u | 3u << 2) == RULE_SRC_ONLY);
        CHECK(paste_rule_check(0u, 3u << 2) == RULE_BOTH && paste_rule_check(0u, 1u | 3u << 2 | 1u << 4) == RULE_BOTH);
        CHECK(paste_rule_check(0u, 1u << 4) == RULE_DST_ONLY && paste_rule_check(0u, 3u << 4) == RULE_DST_ONLY);
        // paste_plan is as it was: an unknown flag bit is still PASTE_FLAGS
        PastePlan plan;
        const int32_t o[3] = {0, 0, 0};
        CHECK(paste_plan(3, 3, o, 4, 4, 4, o, 2, &plan) == PASTE_FLAGS && paste_plan(3, 3, o, 4, 4, 4, o, 0x80000001u, &plan) == PASTE_FLAGS);
    }
    free(map);

    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("paste rule plan sanitize ok: %lld OUT, %lld IN, %lld CUT cells\n", (long long)seen[0], (long long)seen[1], (long long)seen[2]);
    return 0;
}
