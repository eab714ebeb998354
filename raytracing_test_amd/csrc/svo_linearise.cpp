// svo_linearise.cpp — editable world -> the breadth-first linearised tree the gfx950 kernel walks (canonical form:
// svo_world.h, svo_common.h).  One emitter serves both routes: svo_build_view linearises the root into a fresh tree,
// svo_tree_update re-linearises the edited child of a patched tree.  (svo_terrain.cpp is an independent builder of the
// same form; tests check they agree node for node.)
#include <deque>
#include <unordered_map>

#include "svo_world.h"

using namespace svo;

namespace {
constexpr uint32_t C_UNKNOWN = 0xFFFFFFFEu;  // memo: not classified yet (no material id: ids stay below 0xFFFF)

struct Emitter {
    svo_tree* t;
    const svo_world* w;
    bool from_root;  // a full build: every world node is visited (dense memo), and the tree's statistics are counted
    std::vector<uint8_t> solid;  // palette id -> stored by the tree's view
    // classes of the world nodes visited: by world node id for a full build; an update visits one path and the
    // edited subtree, and allocates nothing proportional to the world
    std::vector<uint32_t> dense;
    std::unordered_map<uint32_t, uint32_t> sparse;

    Emitter(svo_tree* t_, const svo_world* w_, bool from_root_) : t(t_), w(w_), from_root(from_root_), solid(w_->pal.m.size()) {
        for (size_t i = 0; i < solid.size(); i++) solid[i] = material_in_view(w->pal.m[i], t->view);
        if (from_root) dense.assign(w->nodes.size(), C_UNKNOWN);
    }

    uint32_t leaf_class(uint16_t mat) const { return solid[mat] ? (uint32_t)mat : C_EMPTY; }

    uint32_t classify(uint32_t n) {
        uint32_t& memo = from_root ? dense[n] : sparse.emplace(n, C_UNKNOWN).first->second;  // (stays valid over inserts)
        if (memo != C_UNKNOWN) return memo;
        const auto& e = w->nodes[n];
        if (e.leaf) return memo = leaf_class(e.mat);
        uint32_t kc[64];
        const uint32_t* k = w->kids(n);
        for (int i = 0; i < 64; i++) kc[i] = k[i] ? classify(k[i]) : C_EMPTY;
        return memo = fold_classes(kc);
    }

    // record of world node e at depth d; its descendants are appended to t->nodes breadth-first
    Node emit(uint32_t e, int d) {
        const int L = t->levels;
        struct Item {
            uint32_t e;
            int d;
            int64_t idx;  // where its record goes (-1: returned)
        };
        std::deque<Item> q;
        q.push_back({e, d, -1});
        Node root_rec{0, 0, K_INTERIOR};
        while (!q.empty()) {
            const Item it = q.front();
            q.pop_front();
            if (from_root) t->nodes_per_level[it.d]++;
            const uint32_t c = classify(it.e);
            Node rec{0, 0, K_INTERIOR};  // (EMPTY: only the root of an empty world is emitted so)
            if (c == C_MIXED) {
                const uint32_t* k = w->kids(it.e);
                if (it.d == L - 1) {
                    uint32_t vox[64];
                    for (int v = 0; v < 64; v++) vox[v] = k[v] ? classify(k[v]) : C_EMPTY;
                    const uint32_t ref = (uint32_t)t->mats.size();
                    BrickOut b = make_brick(vox, &t->mats);
                    rec = Node{b.mask, (b.info & K_UNIFORM) ? 0u : ref, b.info};
                    if (from_root) t->n_bricks++;
                } else {
                    uint64_t mask = 0;
                    for (int sl = 0; sl < 64; sl++)
                        if (k[sl] && classify(k[sl]) != C_EMPTY) mask |= 1ull << sl;
                    const uint64_t base = t->nodes.size();
                    t->nodes.resize(base + __builtin_popcountll(mask), Node{0, 0, 0});
                    int64_t j = (int64_t)base;
                    for (int sl = 0; sl < 64; sl++)
                        if ((mask >> sl) & 1ull) q.push_back({k[sl], it.d + 1, j++});
                    rec = Node{mask, (uint32_t)base, K_INTERIOR};
                }
            } else if (c != C_EMPTY) {
                rec = Node{~0ull, 0, K_SOLID | (c << 16)};
            }
            if (it.idx < 0) root_rec = rec;
            else t->nodes[(size_t)it.idx] = rec;
        }
        return root_rec;
    }

    // the world region of depth `d` holding (x, y, z): its node, or a uniform class when a leaf above covers it /
    // nothing is stored there
    struct Region {
        bool has_node;
        uint32_t node;
        uint32_t cls;
    };
    Region region(uint32_t x, uint32_t y, uint32_t z, int d) const {
        uint32_t n = 0;
        for (int depth = 0;; depth++) {
            const auto& e = w->nodes[n];
            if (e.leaf) return {false, 0, leaf_class(e.mat)};
            if (depth == d) return {true, n, 0};
            const uint32_t c = w->kids(n)[child_slot(x, y, z, (uint32_t)(2 * (w->levels - 1 - depth)))];
            if (!c) return {false, 0, C_EMPTY};
            n = c;
        }
    }
};
}  // namespace

extern "C" int svo_build(const svo_world* w, svo_tree** out) { return svo_build_view(w, SVO_VIEW_SOLID, out); }

extern "C" int svo_build_view(const svo_world* w, int32_t view, svo_tree** out) {
    if (!w || !out) SVO_FAIL(SVO_EINVAL, "svo_build: NULL argument");
    if (view != SVO_VIEW_SOLID && view != SVO_VIEW_ALL) SVO_FAIL(SVO_EINVAL, "svo_build_view: unknown view");
    svo_tree* t = new (std::nothrow) svo_tree();
    if (!t) SVO_FAIL(SVO_ENOMEM, "svo_build: out of memory");
    t->levels = w->levels;
    t->view = view;
    t->palette = w->pal.m;
    t->nodes.push_back(Node{0, 0, K_INTERIOR});  // the root's place: its descendants follow
    const Node root = Emitter(t, w, true).emit(0, 0);
    t->nodes[0] = root;
    if (t->nodes.size() > 0xFFFFFFFFull || t->mats.size() > 0xFFFFFFFFull) {
        delete t;
        SVO_FAIL(SVO_ERANGE, "svo_build: tree exceeds 2^32 nodes");
    }
    *out = t;
    return SVO_OK;
}

// ================================================================================================
// Incremental edits (putBlock / deleteBlock + updateSsboData,
// voxel_allocator.hpp:38-78).  After world edits, the linearised tree is patched instead of
// rebuilt: for each edited region, the deepest interior node A above it whose subtree still holds
// the old content is found; the edited child of A is re-linearised from the world (its subtree
// appended breadth-first), and A's child block is rewritten at the end of the array with the new
// child record (siblings are copied: their own subtrees stay where they are).  Only A's record is
// changed in place.  Results are the tree's *content*, not its canonical layout: regions that
// become uniform are not re-collapsed (traversal is unaffected); when superseded blocks exceed
// half the array, the tree is rebuilt from the world.  svo_tree_sync uploads the appended tail
// and the rewritten records.
// ================================================================================================
extern "C" int svo_tree_update(svo_tree* t, const svo_world* w, const int32_t* xyz, int64_t n, int32_t level) {
    if (!t || !w || (!xyz && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_tree_update: NULL argument");
    if (t->levels != w->levels) SVO_FAIL(SVO_EINVAL, "svo_tree_update: tree and world differ in levels");
    if (level < 1 || level > w->levels + 1) SVO_FAIL(SVO_EINVAL, "svo_tree_update: level out of range");
    if (t->volume_patched)
        SVO_FAIL(SVO_ESTATE, "svo_tree_update: the tree was patched by svo_tree_patch_volume_gpu or svo_tree_patch_points_gpu and no longer follows a world");
    if (t->no_world) SVO_FAIL(SVO_ESTATE, "svo_tree_update: the tree was built by svo_build_points_gpu and follows no world");
    const int L = t->levels;
    const int de = level - 1;  // depth of the edited region (putBlock's `level--`)
    if (w->pal.m.size() != t->palette.size()) {
        t->palette = w->pal.m;  // the world's palette only grows: ids stay valid
        t->palette_dirty = true;
    }
    t->top_valid = false;
    Emitter em(t, w, false);
    const uint32_t mk = wrap_mask(L);
    bool rebuild = de == 0 || node_kind(t->nodes[0].info) != K_INTERIOR;
    for (int64_t i = 0; i < n && !rebuild; i++) {
        const uint32_t x = (uint32_t)xyz[3 * i] & mk, y = (uint32_t)xyz[3 * i + 1] & mk, z = (uint32_t)xyz[3 * i + 2] & mk;
        // A: the deepest interior node above the edited region whose child on the path is interior
        uint32_t a = 0;
        int da = 0;
        while (da < de - 1) {
            const Node& A = t->nodes[a];
            const uint32_t sl = child_slot(x, y, z, (uint32_t)(2 * (L - 1 - da)));
            if (!((A.mask >> sl) & 1ull)) break;
            const uint32_t ci = packed_index(A, sl);
            if (node_kind(t->nodes[ci].info) != K_INTERIOR) break;
            a = ci;
            da++;
        }
        // the child of A on the path, re-linearised from the world
        const uint32_t s = child_slot(x, y, z, (uint32_t)(2 * (L - 1 - da)));
        {  // its columns: the only ones whose ceilings can change (svo_tree_sync)
            const int64_t cs = (int64_t)1 << (2 * (L - 1 - da)), cx = (int64_t)(x & ~(uint32_t)(cs - 1)), cz = (int64_t)(z & ~(uint32_t)(cs - 1));
            t->ceil_dirty.push_back({cx, cz, cx + cs, cz + cs});
        }
        const Emitter::Region r = em.region(x, y, z, da + 1);
        Node rec{0, 0, K_INTERIOR};
        bool empty;
        if (r.has_node) {
            empty = em.classify(r.node) == C_EMPTY;
            if (!empty) rec = em.emit(r.node, da + 1);
        } else {
            empty = r.cls == C_EMPTY;
            if (!empty) rec = Node{~0ull, 0, K_SOLID | (r.cls << 16)};
        }
        // A's child block, rewritten at the end of the array
        const Node A = t->nodes[a];
        const uint64_t m_old = A.mask, m_new = empty ? (m_old & ~(1ull << s)) : (m_old | (1ull << s));
        const uint64_t base = t->nodes.size();
        t->nodes.resize(base + __builtin_popcountll(m_new));
        uint64_t j = base;
        for (uint32_t sl = 0; sl < 64; sl++) {
            if (!((m_new >> sl) & 1ull)) continue;
            t->nodes[j++] = sl == s ? rec : t->nodes[packed_index(A, sl)];
        }
        t->garbage_nodes += (uint64_t)__builtin_popcountll(m_old);
        t->nodes[a] = Node{m_new, (uint32_t)base, K_INTERIOR};
        if (a < t->synced_nodes) t->dirty_nodes.push_back(a);
        em.sparse.clear();  // the next edit may change classes on its own path
        if (t->nodes.size() > 0xFFFFFFFFull) rebuild = true;
    }
    if (rebuild || t->garbage_nodes * 2 > t->nodes.size()) {
        svo_tree* f = nullptr;
        int rc = svo_build_view(w, t->view, &f);
        if (rc) return rc;
        t->nodes.swap(f->nodes);
        t->mats.swap(f->mats);
        t->palette.swap(f->palette);
        for (int i = 0; i < 8; i++) t->nodes_per_level[i] = f->nodes_per_level[i];
        t->n_bricks = f->n_bricks;
        t->garbage_nodes = t->garbage_mats = 0;
        t->dirty_nodes.clear();
        t->full_upload = t->palette_dirty = true;
        delete f;
    }
    return SVO_OK;
}
