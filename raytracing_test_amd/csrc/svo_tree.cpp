// svo_tree.cpp — reading a linearised tree on the host: its statistics, palette and stored blocks, the node a voxel
// resolves to, the raw arrays, its highest stored row, and the column ceilings the casts march under.
#include <string.h>

#include <algorithm>
#include <system_error>
#include <thread>

#include "svo_internal.h"

using namespace svo;

// ================================================================================================
// Tree queries
// ================================================================================================
extern "C" int svo_tree_get_info(const svo_tree* t, svo_tree_info* o) {
    if (!t || !o) SVO_FAIL(SVO_EINVAL, "svo_tree_get_info: NULL argument");
    memset(o, 0, sizeof(*o));
    o->levels = t->levels;
    o->n_materials = (uint32_t)t->palette.size();
    o->n_nodes = t->nodes.size();
    o->n_mat_bytes = t->mats.size() * sizeof(uint16_t);
    o->n_bricks = t->n_bricks;
    for (int i = 0; i < 8; i++) o->nodes_per_level[i] = t->nodes_per_level[i];
    o->device_bytes = t->device_bytes;
    o->device = t->device;
    o->view = t->view;
    return SVO_OK;
}

extern "C" int svo_tree_palette(const svo_tree* t, uint32_t id, svo_block* out) {
    if (!t || !out) SVO_FAIL(SVO_EINVAL, "svo_tree_palette: NULL argument");
    if (id >= t->palette.size()) SVO_FAIL(SVO_ERANGE, "svo_tree_palette: id out of range");
    *out = to_block(t->palette[id]);
    return SVO_OK;
}

extern "C" int svo_tree_get_block(const svo_tree* t, int32_t x, int32_t y, int32_t z, svo_block* out, uint32_t* mid) {
    if (!t || !out) SVO_FAIL(SVO_EINVAL, "svo_tree_get_block: NULL argument");
    const uint32_t mk = wrap_mask(t->levels);
    const uint32_t wx = (uint32_t)x & mk, wy = (uint32_t)y & mk, wz = (uint32_t)z & mk;
    uint32_t ni = 0, mat = 0;
    for (int d = 0; d < t->levels; d++) {
        const Node& n = t->nodes[ni];
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) {
            mat = node_material(n.info);
            break;
        }
        if (kind == K_BRICK) {
            const uint32_t v = child_slot(wx, wy, wz, 0);
            if ((n.mask >> v) & 1ull)
                mat = (n.info & K_UNIFORM) ? node_material(n.info) : t->mats[packed_index(n, v)];
            break;
        }
        const uint32_t sl = child_slot(wx, wy, wz, (uint32_t)(2 * (t->levels - 1 - d)));
        if (!((n.mask >> sl) & 1ull)) break;
        ni = packed_index(n, sl);
    }
    *out = to_block(t->palette[mat]);
    if (mid) *mid = mat;
    return SVO_OK;
}

extern "C" int svo_tree_get_blocks(const svo_tree* t, const int32_t* xyz, int64_t n, uint32_t* ids) {
    if (!t || ((!xyz || !ids) && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_tree_get_blocks: NULL argument");
    for (int64_t i = 0; i < n; i++) {
        svo_block b;
        int rc = svo_tree_get_block(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &b, &ids[i]);
        if (rc) return rc;
    }
    return SVO_OK;
}

extern "C" int svo_tree_node_indices(const svo_tree* t, const int32_t* xyz, int64_t n, uint64_t* idx) {
    if (!t || ((!xyz || !idx) && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_tree_node_indices: NULL argument");
    const uint32_t mk = wrap_mask(t->levels);
    for (int64_t i = 0; i < n; i++) {
        const uint32_t wx = (uint32_t)xyz[3 * i] & mk, wy = (uint32_t)xyz[3 * i + 1] & mk, wz = (uint32_t)xyz[3 * i + 2] & mk;
        uint32_t ni = 0;
        for (int d = 0; d < t->levels; d++) {
            const Node& nd = t->nodes[ni];
            if (node_kind(nd.info) != K_INTERIOR) break;
            const uint32_t sl = child_slot(wx, wy, wz, (uint32_t)(2 * (t->levels - 1 - d)));
            if (!((nd.mask >> sl) & 1ull)) break;
            ni = packed_index(nd, sl);
        }
        idx[i] = ni;
    }
    return SVO_OK;
}

extern "C" int svo_tree_export(const svo_tree* t, void* nodes, uint64_t nb, void* mats, uint64_t mb) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_export: NULL tree");
    if (nodes) {
        if (nb < t->nodes.size() * sizeof(Node)) SVO_FAIL(SVO_ERANGE, "svo_tree_export: node buffer too small");
        memcpy(nodes, t->nodes.data(), t->nodes.size() * sizeof(Node));
    }
    if (mats) {
        if (mb < t->mats.size() * sizeof(uint16_t)) SVO_FAIL(SVO_ERANGE, "svo_tree_export: material buffer too small");
        memcpy(mats, t->mats.data(), t->mats.size() * sizeof(uint16_t));
    }
    return SVO_OK;
}

// Highest y of any stored voxel (wrapped coordinates), by a descent that visits child slots from the
// top y-row down and prunes regions that cannot beat the best found so far; cached on the tree.
namespace {
int32_t top_y_of(const svo_tree* t, uint32_t ni, int32_t y0, int depth, int32_t best) {
    const Node& n = t->nodes[ni];
    const int32_t size = 1 << (2 * (t->levels - depth));
    if (y0 + size - 1 <= best) return best;
    const uint32_t kind = node_kind(n.info);
    if (kind == K_SOLID) return y0 + size - 1;
    if (kind == K_BRICK) {
        for (int ly = 3; ly >= 0; ly--)
            if (n.mask & (0x000F000F000F000Full << (4 * ly))) return std::max(best, y0 + ly);
        return best;
    }
    const int32_t cs = size >> 2;
    for (int sy = 3; sy >= 0; sy--) {
        if (y0 + (sy + 1) * cs - 1 <= best) break;
        for (int sz = 0; sz < 4; sz++)
            for (int sx = 0; sx < 4; sx++) {
                const uint32_t sl = (uint32_t)((sz << 4) | (sy << 2) | sx);
                if (!((n.mask >> sl) & 1ull)) continue;
                const uint32_t ci = packed_index(n, sl);
                best = top_y_of(t, ci, y0 + sy * cs, depth + 1, best);
            }
    }
    return best;
}
}  // namespace

int32_t svo::tree_top_y(const svo_tree* t) {
    std::lock_guard<std::mutex> lock(t->top_mu);
    if (!t->top_valid) {
        t->top_y = t->nodes.empty() ? -1 : top_y_of(t, 0, 0, 0, -1);
        t->top_valid = true;
    }
    return t->top_y;
}

// Column ceilings: one walk over the tree fills the finest level (blocks of 4^kCeilK0 columns) with
// the highest stored row over each block, then coarser levels take maxima of 4 x 4 blocks.
namespace {
struct CeilWalk {
    const svo_tree* t;
    int32_t bsh;   // log2 of the finest block's width
    int64_t rows;  // finest blocks per row
    int16_t* top;
    void put(int64_t bx, int64_t bz, int32_t y) {
        int16_t& c = top[bz * rows + bx];
        if (y > c) c = (int16_t)y;
    }
    // region of node ni: [x0, x0 + size) x [y0, ..) x [z0, ..)
    void walk(uint32_t ni, int32_t x0, int32_t y0, int32_t z0, int depth) {
        const Node& n = t->nodes[ni];
        const int32_t size = 1 << (2 * (t->levels - depth));
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) {
            const int64_t nb = std::max<int64_t>(1, (int64_t)size >> bsh);
            for (int64_t bz = 0; bz < nb; bz++)
                for (int64_t bx = 0; bx < nb; bx++) put(((int64_t)x0 >> bsh) + bx, ((int64_t)z0 >> bsh) + bz, y0 + size - 1);
            return;
        }
        if (kind == K_BRICK) {
            for (int ly = 3; ly >= 0; ly--)
                if (n.mask & (0x000F000F000F000Full << (4 * ly))) {
                    put((int64_t)x0 >> bsh, (int64_t)z0 >> bsh, y0 + ly);
                    break;
                }
            return;
        }
        const int32_t cs = size >> 2;
        uint64_t m = n.mask;
        uint32_t ci = n.ref;
        while (m) {
            const uint32_t sl = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            walk(ci++, x0 + (int32_t)(sl & 3u) * cs, y0 + (int32_t)((sl >> 2) & 3u) * cs, z0 + (int32_t)(sl >> 4) * cs, depth + 1);
        }
    }
};
}  // namespace

namespace {
// the highest stored row over every block of 2^bsh columns (`rows` blocks per row of `top`, preset to -1), by one walk
void walk_all(const svo_tree* t, int32_t bsh, int64_t rows, int16_t* top) {
    CeilWalk cw{t, bsh, rows, top};
    const Node& root = t->nodes[0];
    if (node_kind(root.info) != K_INTERIOR) {
        cw.walk(0, 0, 0, 0, 0);
        return;
    }
    // the root's children by column (x, z slot): each thread walks the four children over one
    // quarter x quarter of the columns, so the blocks it writes are its own
    const int32_t cs = 1 << (2 * (t->levels - 1));
    auto quadrant = [&, cs](uint32_t xz) {
        CeilWalk w = cw;
        for (uint32_t y = 0; y < 4; y++) {
            const uint32_t sl = ((xz >> 2) << 4) | (y << 2) | (xz & 3u);
            if (!((root.mask >> sl) & 1ull)) continue;
            const uint32_t ci = packed_index(root, sl);
            w.walk(ci, (int32_t)(xz & 3u) * cs, (int32_t)y * cs, (int32_t)(xz >> 2) * cs, 1);
        }
    };
    std::vector<std::thread> th;
    uint32_t started = 0;
    try {
        for (; started < 16; started++) th.emplace_back(quadrant, started);
    } catch (const std::system_error&) {
        // (no more threads: the quadrants not started are walked here)
    }
    for (uint32_t xz = started; xz < 16; xz++) quadrant(xz);
    for (auto& x : th) x.join();
}
}  // namespace

// level 0 of `out` over the level-0 blocks [bx0, bx1) x [bz0, bz1) as the 4 x 4 maxima of the fine table
static void level0_from_fine(const svo_tree* t, const std::vector<int16_t>& fine, int16_t* top, int64_t bx0, int64_t bz0, int64_t bx1, int64_t bz1) {
    const int64_t rows = (int64_t)1 << (2 * (t->levels - kCeilK0)), per = (int64_t)1 << (2 * kCeilK0 - kCeilFineSh), frows = rows * per;
    for (int64_t bz = bz0; bz < bz1; bz++)
        for (int64_t bx = bx0; bx < bx1; bx++) {
            int16_t v = -1;
            for (int64_t dz = 0; dz < per; dz++)
                for (int64_t dx = 0; dx < per; dx++) v = std::max(v, fine[(size_t)((bz * per + dz) * frows + bx * per + dx)]);
            top[bz * rows + bx] = v;
        }
}

int32_t svo::tree_ceilings(const svo_tree* t, std::vector<int16_t>& out, int64_t off[kCeilMax], std::vector<int16_t>* fine) {
    out.clear();
    if (fine) fine->clear();
    const int32_t nlev = std::min<int32_t>(kCeilMax, t->levels - kCeilK0);
    if (nlev <= 0 || t->nodes.empty()) return 0;
    int64_t total = 0;
    for (int32_t j = 0; j < nlev; j++) {
        const int64_t rows = (int64_t)1 << (2 * (t->levels - kCeilK0 - j));
        off[j] = total;
        total += rows * rows;
    }
    out.assign((size_t)total, (int16_t)-1);
    const int64_t rows0 = (int64_t)1 << (2 * (t->levels - kCeilK0));
    if (fine) {  // one walk fills the fine table; level 0 is its 4 x 4 maxima
        tree_ceilings_fine(t, *fine);
        level0_from_fine(t, *fine, out.data(), 0, 0, rows0, rows0);
    } else {
        walk_all(t, 2 * kCeilK0, rows0, out.data());
    }
    ceilings_coarsen(t, out, off, nlev, 0, 0, (int64_t)1 << (2 * t->levels), (int64_t)1 << (2 * t->levels));
    return nlev;
}

void svo::tree_ceilings_fine(const svo_tree* t, std::vector<int16_t>& out) {
    out.clear();
    if (t->levels - kCeilK0 <= 0 || t->nodes.empty()) return;
    const int64_t rows = (int64_t)1 << (2 * t->levels - kCeilFineSh);
    out.assign((size_t)(rows * rows), (int16_t)-1);
    walk_all(t, kCeilFineSh, rows, out.data());
}

// levels 1 .. nlev-1 as 4 x 4 maxima of the finer level, over the blocks that hold columns [x0, x1) x [z0, z1)
void svo::ceilings_coarsen(const svo_tree* t, std::vector<int16_t>& out, const int64_t off[kCeilMax], int32_t nlev, int64_t x0, int64_t z0,
                           int64_t x1, int64_t z1) {
    for (int32_t j = 1; j < nlev; j++) {
        const int32_t bsh = 2 * (kCeilK0 + j);
        const int64_t rows = (int64_t)1 << (2 * (t->levels - kCeilK0 - j)), fine = rows * 4;
        const int16_t* f = out.data() + off[j - 1];
        int16_t* c = out.data() + off[j];
        for (int64_t bz = z0 >> bsh; bz < std::min(rows, ((z1 - 1) >> bsh) + 1); bz++)
            for (int64_t bx = x0 >> bsh; bx < std::min(rows, ((x1 - 1) >> bsh) + 1); bx++) {
                int16_t v = -1;
                for (int64_t dz = 0; dz < 4; dz++)
                    for (int64_t dx = 0; dx < 4; dx++) v = std::max(v, f[(bz * 4 + dz) * fine + bx * 4 + dx]);
                c[bz * rows + bx] = v;
            }
    }
}

// The finest level over the columns [x0, x1) x [z0, z1) (aligned to the finest blocks) recomputed from the tree: the
// blocks are cleared, then a walk that enters only the nodes whose columns meet the rectangle raises them again.
namespace {
struct CeilRectWalk {
    CeilWalk cw;
    int64_t x0, z0, x1, z1;
    void walk(uint32_t ni, int64_t nx, int32_t ny, int64_t nz, int depth) {
        const svo_tree* t = cw.t;
        const Node& n = t->nodes[ni];
        const int64_t size = (int64_t)1 << (2 * (t->levels - depth));
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) {
            const int32_t bsh = cw.bsh;
            const int64_t ax = std::max(nx, x0), bx = std::min(nx + size, x1), az = std::max(nz, z0), bz = std::min(nz + size, z1);
            for (int64_t z = az >> bsh; z <= (bz - 1) >> bsh; z++)
                for (int64_t x = ax >> bsh; x <= (bx - 1) >> bsh; x++) cw.put(x, z, ny + (int32_t)size - 1);
            return;
        }
        if (kind == K_BRICK) {
            cw.walk(ni, (int32_t)nx, ny, (int32_t)nz, depth);
            return;
        }
        const int64_t cs = size >> 2;
        uint64_t m = n.mask;
        uint32_t ci = n.ref;
        while (m) {
            const uint32_t sl = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const int64_t cx = nx + (int64_t)(sl & 3u) * cs, cz = nz + (int64_t)(sl >> 4) * cs;
            const uint32_t c = ci++;
            if (cx >= x1 || cx + cs <= x0 || cz >= z1 || cz + cs <= z0) continue;
            walk(c, cx, ny + (int32_t)((sl >> 2) & 3u) * (int32_t)cs, cz, depth + 1);
        }
    }
};
}  // namespace

// (the table `top` of blocks of 2^bsh columns, `rows` per row, over a rectangle aligned to level-0 blocks)
static void rect_rewalk(const svo_tree* t, int32_t bsh, int64_t rows, int16_t* top, int64_t x0, int64_t z0, int64_t x1, int64_t z1) {
    for (int64_t bz = z0 >> bsh; bz < z1 >> bsh; bz++)
        for (int64_t bx = x0 >> bsh; bx < x1 >> bsh; bx++) top[bz * rows + bx] = -1;
    CeilRectWalk w{CeilWalk{t, bsh, rows, top}, x0, z0, x1, z1};
    w.walk(0, 0, 0, 0, 0);
}

// a column rectangle widened to whole level-0 blocks
static void widen_rect(int64_t& x0, int64_t& z0, int64_t& x1, int64_t& z1) {
    const int32_t bsh = 2 * kCeilK0;
    x0 = (x0 >> bsh) << bsh;
    z0 = (z0 >> bsh) << bsh;
    x1 = (((x1 - 1) >> bsh) + 1) << bsh;
    z1 = (((z1 - 1) >> bsh) + 1) << bsh;
}

void svo::ceilings_update_rect(const svo_tree* t, std::vector<int16_t>& out, const int64_t off[kCeilMax], int32_t nlev, int64_t x0,
                               int64_t z0, int64_t x1, int64_t z1, std::vector<int16_t>* fine) {
    if (nlev <= 0 || t->nodes.empty()) return;
    widen_rect(x0, z0, x1, z1);
    const int32_t bsh = 2 * kCeilK0;
    if (fine && !fine->empty()) {  // one restricted walk, into the fine table; level 0 follows from it
        rect_rewalk(t, kCeilFineSh, (int64_t)1 << (2 * t->levels - kCeilFineSh), fine->data(), x0, z0, x1, z1);
        level0_from_fine(t, *fine, out.data() + off[0], x0 >> bsh, z0 >> bsh, x1 >> bsh, z1 >> bsh);
    } else {
        rect_rewalk(t, bsh, (int64_t)1 << (2 * (t->levels - kCeilK0)), out.data() + off[0], x0, z0, x1, z1);
    }
    ceilings_coarsen(t, out, off, nlev, x0, z0, x1, z1);
}

extern "C" int svo_tree_ceilings_fine(const svo_tree* t, int16_t* out, int64_t cap, int32_t* shift, int64_t* n) {
    if (!t || !shift || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_ceilings_fine: NULL argument");
    std::vector<int16_t> c;
    tree_ceilings_fine(t, c);
    *shift = kCeilFineSh;
    *n = (int64_t)c.size();
    if (out) {
        if (cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_ceilings_fine: buffer too small");
        if (!c.empty()) memcpy(out, c.data(), c.size() * sizeof(int16_t));
    }
    return SVO_OK;
}

extern "C" int svo_tree_ceilings(const svo_tree* t, int16_t* out, int64_t cap, int32_t* levels, int64_t* n) {
    if (!t || !levels || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_ceilings: NULL argument");
    std::vector<int16_t> c;
    int64_t off[kCeilMax] = {0, 0, 0, 0};
    *levels = tree_ceilings(t, c, off);
    *n = (int64_t)c.size();
    if (out) {
        if (cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_ceilings: buffer too small");
        if (!c.empty()) memcpy(out, c.data(), c.size() * sizeof(int16_t));
    }
    return SVO_OK;
}
