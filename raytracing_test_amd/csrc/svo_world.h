// svo_world.h — what the host files that read or write the editable world share (svo_world.cpp: the edits;
// svo_linearise.cpp: world -> tree; svo_terrain.cpp: the builder that needs no world): the world itself and the pieces
// of the canonical form that every builder must state alike.  Host only: it pulls in <map> and the edit tree, so no HIP
// translation unit and not svo_internal.h may include it.
#pragma once

#include <string.h>

#include <functional>
#include <map>
#include <tuple>
#include <vector>

#include "svo_internal.h"
#include "svo_noise.h"

namespace svo {

// fn(begin, end) over [0, n) in chunks on up to `nthreads` threads (<= 0: the machine's, at most 16): svo_world.cpp
void parallel_for(int64_t n, int nthreads, const std::function<void(int64_t, int64_t)>& fn);

// genWorld's three noises (world_gen.cpp:15-22: seeds 42, 64, 100) and the column top they give
struct TerrainNoise {
    Simplex2 n42, n64, n100;
    TerrainNoise() {
        simplex2_seed(n42, 42);
        simplex2_seed(n64, 64);
        simplex2_seed(n100, 100);
    }
    int32_t height(int32_t x, int32_t z) const { return terrain_height(n42.perm, n64.perm, n100.perm, x, z); }
};

// ================================================================================================
// Palette
// ================================================================================================
struct Palette {
    std::vector<Material> m;
    std::map<std::tuple<uint32_t, uint64_t, uint32_t>, uint16_t> index;
    Palette() { m.push_back(Material{0, ~0ull, 0.0f}); }
    int intern(const Material& x) {
        uint32_t mb;
        memcpy(&mb, &x.meta, 4);
        auto key = std::make_tuple(x.flags, x.color, mb);
        auto it = index.find(key);
        if (it != index.end()) return it->second;
        if (m.size() >= 0xFFFFu) return -1;
        uint16_t id = (uint16_t)m.size();
        m.push_back(x);
        index[key] = id;
        return id;
    }
};

}  // namespace svo

// ================================================================================================
// Editable world: a 64-ary pointer tree with the reference's semantics (tetrahexa_tree.cpp), minus
// its root-array aliasing.  Node 0 is the root; a child id of 0 means "absent" (bitmap bit clear).
// Leaves may sit at any depth (putBlock level < levels+1 stores a uniform region).
// ================================================================================================
struct svo_world {
    int32_t levels;
    svo::Palette pal;
    struct ENode {
        uint32_t kids;  // branch: index of its 64-slot child block
        uint16_t mat;   // leaf: palette id
        uint8_t leaf;
    };
    std::vector<ENode> nodes;
    std::vector<uint32_t> kid_blocks;  // 64 ids per block
    std::vector<uint32_t> free_nodes, free_blocks;
    uint64_t live_nodes = 0;

    uint32_t new_block() {
        uint32_t b;
        if (!free_blocks.empty()) {
            b = free_blocks.back();
            free_blocks.pop_back();
        } else {
            b = (uint32_t)(kid_blocks.size() / 64);
            kid_blocks.resize(kid_blocks.size() + 64);
        }
        std::fill(kid_blocks.begin() + (size_t)b * 64, kid_blocks.begin() + (size_t)b * 64 + 64, 0u);
        return b;
    }
    uint32_t new_node(uint8_t leaf, uint16_t mat) {
        uint32_t n;
        if (!free_nodes.empty()) {
            n = free_nodes.back();
            free_nodes.pop_back();
        } else {
            n = (uint32_t)nodes.size();
            nodes.push_back(ENode{0, 0, 0});
        }
        nodes[n].leaf = leaf;
        nodes[n].mat = mat;
        nodes[n].kids = leaf ? 0 : new_block();
        live_nodes++;
        return n;
    }
    uint32_t* kids(uint32_t n) { return &kid_blocks[(size_t)nodes[n].kids * 64]; }
    const uint32_t* kids(uint32_t n) const { return &kid_blocks[(size_t)nodes[n].kids * 64]; }
    // deleteChildren (tetrahexa_tree.cpp:159-173)
    void drop_children(uint32_t n) {
        if (nodes[n].leaf) return;
        uint32_t b = nodes[n].kids;
        for (int i = 0; i < 64; i++) {
            uint32_t c = kid_blocks[(size_t)b * 64 + i];
            if (c) {
                drop_children(c);
                free_nodes.push_back(c);
                live_nodes--;
            }
        }
        free_blocks.push_back(b);
    }
    void make_leaf(uint32_t n, uint16_t mat) {
        drop_children(n);
        nodes[n].leaf = 1;
        nodes[n].mat = mat;
        nodes[n].kids = 0;
    }
    // split a leaf into 64 copies of itself (tetrahexa_tree.cpp:221-247)
    void split(uint32_t n) {
        uint16_t m = nodes[n].mat;
        uint32_t b = new_block();
        for (int i = 0; i < 64; i++) {
            uint32_t c = new_node(1, m);
            kid_blocks[(size_t)b * 64 + i] = c;
        }
        nodes[n].leaf = 0;
        nodes[n].kids = b;
    }
};

namespace svo {

// ================================================================================================
// Canonical linearisation.  Region classes in the solid view (non-solid blocks count as empty):
//   EMPTY, SOLID(material), MIXED.  A MIXED region at depth levels-1 becomes a BRICK, deeper up an
//   INTERIOR node whose non-EMPTY children follow in breadth-first order.
// ================================================================================================
constexpr uint32_t C_EMPTY = 0u;
constexpr uint32_t C_MIXED = 0xFFFFFFFFu;  // otherwise SOLID with material = class

struct BrickOut {
    uint64_t mask;
    uint32_t info;
};

// fold 64 voxel classes (EMPTY or SOLID ids) into brick mask + material run
inline BrickOut make_brick(const uint32_t* vox, std::vector<uint16_t>* mats_out) {
    uint64_t mask = 0;
    uint32_t first = C_EMPTY;
    bool uniform = true;
    for (int v = 0; v < 64; v++) {
        if (vox[v] == C_EMPTY) continue;
        mask |= 1ull << v;
        if (first == C_EMPTY) first = vox[v];
        else if (vox[v] != first) uniform = false;
    }
    if (uniform) return BrickOut{mask, K_BRICK | K_UNIFORM | (first << 16)};
    if (mats_out)
        for (int v = 0; v < 64; v++)
            if (vox[v] != C_EMPTY) mats_out->push_back((uint16_t)vox[v]);
    return BrickOut{mask, K_BRICK};
}

inline uint32_t fold_classes(const uint32_t* c) {
    uint32_t f = c[0];
    if (f == C_MIXED) return C_MIXED;
    for (int i = 1; i < 64; i++)
        if (c[i] != f) return C_MIXED;
    return f;  // all EMPTY or all SOLID(m)
}

}  // namespace svo
