// svo_terrain.cpp — the terrain / heightfield builder: genWorld's columns -> the canonical tree (svo_world.h,
// svo_common.h) without a per-voxel edit tree, for depth-12 / depth-14 terrain that the reference's one-leaf-per-voxel
// layout cannot hold.  Heights are generated in parallel; a min/max pyramid over aligned 4^k column footprints
// classifies every region in O(1) (see classify_region); the tree is emitted depth by depth with a count pass + prefix
// sum + write pass, all multi-threaded.  Independent of svo_linearise.cpp on purpose: tests check that the two builders
// agree node for node.
#include <algorithm>
#include <atomic>

#include "svo_world.h"

using namespace svo;

namespace {
struct Pyramid {
    int32_t W, L;           // columns
    std::vector<int32_t> dimx, dimz;
    std::vector<std::vector<int16_t>> hmin, hmax;  // level k: ceil(W/4^k) x ceil(L/4^k), [cx*dz + cz]
};

struct TerrainCtx {
    int32_t levels, E, W, L;
    const int16_t* h;  // [x*L + z]
    Pyramid pyr;
    uint32_t id_of[5];  // terrain material -> palette id (0 for non-stored)
    int32_t view;       // SVO_VIEW_SOLID / SVO_VIEW_ALL
};

inline uint32_t solid_class(const TerrainCtx& T, int32_t h, int32_t y) {
    return T.id_of[terrain_material(h, y)];
}

// class of the aligned region [x0,x0+s) x [y0,y0+s) x [z0,z0+s), s = 4^k >= 4 (svo_noise.h
// terrain_region_class over the pyramid's min / max tops of its footprint)
uint32_t classify_region(const TerrainCtx& T, int32_t x0, int32_t y0, int32_t z0, int32_t s, int k) {
    const int32_t y1 = y0 + s - 1;
    if (x0 >= T.W || z0 >= T.L) return C_EMPTY;  // no columns here
    const bool partial = (x0 + s > T.W) || (z0 + s > T.L);
    const int32_t cx = x0 >> (2 * k), cz = z0 >> (2 * k);
    const size_t ci = (size_t)cx * T.pyr.dimz[k] + cz;
    const int32_t hmin = T.pyr.hmin[k][ci], hmax = T.pyr.hmax[k][ci];
    if (terrain_region_empty(T.view, hmax, y0, y1)) return C_EMPTY;
    if (partial) return C_MIXED;
    return terrain_region_class(T.id_of, T.view, hmin, hmax, y0, y1, C_EMPTY, C_MIXED);
}

void brick_voxels(const TerrainCtx& T, int32_t x0, int32_t y0, int32_t z0, uint32_t vox[64]) {
    for (int lz = 0; lz < 4; lz++)
        for (int lx = 0; lx < 4; lx++) {
            const int32_t x = x0 + lx, z = z0 + lz;
            const bool have = x < T.W && z < T.L;
            const int32_t h = have ? T.h[(size_t)x * T.L + z] : 0;
            for (int ly = 0; ly < 4; ly++) vox[(lz << 4) | (ly << 2) | lx] = have ? solid_class(T, h, y0 + ly) : C_EMPTY;
        }
}

struct Region {
    int32_t x0, y0, z0;
};
}  // namespace

static int build_from_heights(int32_t levels, int32_t width, int32_t length, int32_t nthreads, int32_t view, std::vector<int16_t>& hg,
                              svo_tree** out);

// genWorld's column tops (world_gen.cpp:22), parallel over x: put(x * length + z, top) for every column
template <class Put>
static void terrain_heights(int32_t width, int32_t length, int32_t nthreads, Put put) {
    const TerrainNoise tn;
    parallel_for(width, nthreads, [&](int64_t b, int64_t e) {
        for (int64_t x = b; x < e; x++)
            for (int32_t z = 0; z < length; z++) put((size_t)x * length + z, tn.height((int32_t)x, z));
    });
}

extern "C" int svo_build_terrain(int32_t levels, int32_t width, int32_t length, int32_t nthreads, svo_tree** out) {
    return svo_build_terrain_view(levels, width, length, nthreads, SVO_VIEW_SOLID, out);
}

extern "C" int svo_build_terrain_view(int32_t levels, int32_t width, int32_t length, int32_t nthreads, int32_t view, svo_tree** out) {
    if (!out) SVO_FAIL(SVO_EINVAL, "svo_build_terrain: out is NULL");
    if (view != SVO_VIEW_SOLID && view != SVO_VIEW_ALL) SVO_FAIL(SVO_EINVAL, "svo_build_terrain_view: unknown view");
    if (levels < 2 || levels > 7) SVO_FAIL(SVO_EINVAL, "svo_build_terrain: levels must be in [2, 7]");
    const int32_t E = 1 << (2 * levels);
    if (width < 1 || length < 1 || width > E || length > E) SVO_FAIL(SVO_EINVAL, "svo_build_terrain: columns must fit the extent");
    std::vector<int16_t> hg((size_t)width * length);
    std::atomic<int> bad(0);
    terrain_heights(width, length, nthreads, [&](size_t i, int32_t h) {
        if (h < 0 || h > 32767) bad = 1;
        hg[i] = (int16_t)h;
    });
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_build_terrain: a column top falls outside [0, 32767]");
    return build_from_heights(levels, width, length, nthreads, view, hg, out);
}

extern "C" int svo_build_heightfield(int32_t levels, int32_t width, int32_t length, const int32_t* heights, int32_t nthreads,
                                     svo_tree** out) {
    if (!out || !heights) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield: NULL argument");
    if (levels < 2 || levels > 7) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield: levels must be in [2, 7]");
    const int32_t E = 1 << (2 * levels);
    if (width < 1 || length < 1 || width > E || length > E) SVO_FAIL(SVO_EINVAL, "svo_build_heightfield: columns must fit the extent");
    std::vector<int16_t> hg((size_t)width * length);
    for (size_t i = 0; i < hg.size(); i++) {
        if (heights[i] < 0 || heights[i] > 32767) SVO_FAIL(SVO_ERANGE, "svo_build_heightfield: heights must be in [0, extent-2]");
        hg[i] = (int16_t)heights[i];
    }
    return build_from_heights(levels, width, length, nthreads, SVO_VIEW_SOLID, hg, out);
}

static int build_from_heights(int32_t levels, int32_t width, int32_t length, int32_t nthreads, int32_t view, std::vector<int16_t>& hg,
                              svo_tree** out) {
    const int32_t E = 1 << (2 * levels);
    for (size_t i = 0; i < hg.size(); i++)
        if (hg[i] + 1 >= E || 21 >= E)
            SVO_FAIL(SVO_ERANGE, "svo_build_terrain: a column top falls outside [0, extent-2] (wrap not supported here; use svo_gen_world)");
    TerrainCtx T;
    T.levels = levels;
    T.E = E;
    T.W = width;
    T.L = length;
    T.h = hg.data();
    T.view = view;
    // ---- min/max pyramid over aligned 4^k footprints
    T.pyr.W = width;
    T.pyr.L = length;
    T.pyr.dimx.push_back(width);
    T.pyr.dimz.push_back(length);
    T.pyr.hmin.push_back(hg);
    T.pyr.hmax.push_back(hg);
    for (int k = 1; k <= levels; k++) {
        const int32_t px = T.pyr.dimx[k - 1], pz = T.pyr.dimz[k - 1];
        const int32_t dx = (px + 3) / 4, dz = (pz + 3) / 4;
        std::vector<int16_t> mn((size_t)dx * dz), mx((size_t)dx * dz);
        const auto& pmn = T.pyr.hmin[k - 1];
        const auto& pmx = T.pyr.hmax[k - 1];
        parallel_for(dx, nthreads, [&](int64_t b, int64_t e) {
            for (int64_t cx = b; cx < e; cx++)
                for (int32_t cz = 0; cz < dz; cz++) {
                    int16_t a = 32767, c = -32768;
                    for (int i = 0; i < 4; i++)
                        for (int j = 0; j < 4; j++) {
                            const int64_t sx = cx * 4 + i, sz = (int64_t)cz * 4 + j;
                            if (sx >= px || sz >= pz) continue;
                            a = std::min(a, pmn[(size_t)sx * pz + sz]);
                            c = std::max(c, pmx[(size_t)sx * pz + sz]);
                        }
                    mn[(size_t)cx * dz + cz] = a;
                    mx[(size_t)cx * dz + cz] = c;
                }
        });
        T.pyr.dimx.push_back(dx);
        T.pyr.dimz.push_back(dz);
        T.pyr.hmin.push_back(std::move(mn));
        T.pyr.hmax.push_back(std::move(mx));
    }
    svo_tree* t = new (std::nothrow) svo_tree();
    if (!t) SVO_FAIL(SVO_ENOMEM, "svo_build_terrain: out of memory");
    t->levels = levels;
    t->view = view;
    // palette: the blocks genWorld stores (stored flags = 1 | Block.flags)
    t->palette.push_back(Material{0, ~0ull, 0.0f});
    t->palette.push_back(Material{1u, rgb_to_u64(0, 150, 10), 0.0f});  // 1 grass
    t->palette.push_back(Material{1u, rgb_to_u64(45, 18, 0), 0.0f});   // 2 dirt
    t->palette.push_back(Material{1u, rgb_to_u64(33, 33, 33), 0.0f});  // 3 stone
    t->palette.push_back(Material{1u | 0x14u, rgb_to_u64(0, 150, 10), 0.0f});  // 4 water (LIQUID)
    T.id_of[TM_AIR] = C_EMPTY;
    T.id_of[TM_WATER] = view ? 4u : C_EMPTY;
    T.id_of[TM_GRASS] = 1;
    T.id_of[TM_DIRT] = 2;
    T.id_of[TM_STONE] = 3;

    // root
    const uint32_t rc = classify_region(T, 0, 0, 0, E, levels);
    if (rc == C_EMPTY) {
        t->nodes.push_back(Node{0, 0, K_INTERIOR});
        t->nodes_per_level[0] = 1;
        *out = t;
        return SVO_OK;
    }
    if (rc != C_MIXED) {
        t->nodes.push_back(Node{~0ull, 0, K_SOLID | (rc << 16)});
        t->nodes_per_level[0] = 1;
        *out = t;
        return SVO_OK;
    }
    std::vector<Region> cur{{0, 0, 0}};
    std::vector<uint64_t> cur_node{0};  // node index of each MIXED region
    t->nodes.push_back(Node{0, 0, K_INTERIOR});
    t->nodes_per_level[0] = 1;
    uint64_t level_end = 1;  // nodes emitted so far = start of the next depth
    for (int d = 0; d < levels && !cur.empty(); d++) {
        const int32_t s = 1 << (2 * (levels - d));  // region size at depth d
        const int32_t cs = s >> 2;
        const int64_t nr = (int64_t)cur.size();
        if (d == levels - 1) {
            // bricks: two passes for the material run offsets
            std::vector<uint32_t> nmat(nr);
            std::vector<BrickOut> bo(nr);
            parallel_for(nr, nthreads, [&](int64_t b, int64_t e) {
                uint32_t vox[64];
                for (int64_t i = b; i < e; i++) {
                    brick_voxels(T, cur[i].x0, cur[i].y0, cur[i].z0, vox);
                    bo[i] = make_brick(vox, nullptr);
                    nmat[i] = (bo[i].info & K_UNIFORM) ? 0u : (uint32_t)__builtin_popcountll(bo[i].mask);
                }
            });
            std::vector<uint64_t> moff(nr + 1, 0);
            for (int64_t i = 0; i < nr; i++) moff[i + 1] = moff[i] + nmat[i];
            t->mats.resize(moff[nr]);
            parallel_for(nr, nthreads, [&](int64_t b, int64_t e) {
                uint32_t vox[64];
                for (int64_t i = b; i < e; i++) {
                    uint32_t ref = 0;
                    if (nmat[i]) {
                        brick_voxels(T, cur[i].x0, cur[i].y0, cur[i].z0, vox);
                        uint64_t o = moff[i];
                        for (int v = 0; v < 64; v++)
                            if (vox[v] != C_EMPTY) t->mats[o++] = (uint16_t)vox[v];
                        ref = (uint32_t)moff[i];
                    }
                    t->nodes[cur_node[i]] = Node{bo[i].mask, ref, bo[i].info};
                }
            });
            t->n_bricks = (uint64_t)nr;
            break;
        }
        // pass 1: per region, count non-empty and mixed children
        std::vector<uint32_t> nkid(nr), nmix(nr);
        parallel_for(nr, nthreads, [&](int64_t b, int64_t e) {
            for (int64_t i = b; i < e; i++) {
                uint32_t a = 0, m = 0;
                for (int sl = 0; sl < 64; sl++) {
                    uint32_t c = classify_region(T, cur[i].x0 + (sl & 3) * cs, cur[i].y0 + ((sl >> 2) & 3) * cs,
                                                 cur[i].z0 + ((sl >> 4) & 3) * cs, cs, levels - d - 1);
                    a += c != C_EMPTY;
                    m += c == C_MIXED;
                }
                nkid[i] = a;
                nmix[i] = m;
            }
        });
        std::vector<uint64_t> koff(nr + 1, 0), moff(nr + 1, 0);
        for (int64_t i = 0; i < nr; i++) {
            koff[i + 1] = koff[i] + nkid[i];
            moff[i + 1] = moff[i] + nmix[i];
        }
        const uint64_t base = level_end;
        t->nodes.resize(base + koff[nr]);
        t->nodes_per_level[d + 1] = koff[nr];
        std::vector<Region> next(moff[nr]);
        std::vector<uint64_t> next_node(moff[nr]);
        // pass 2: write this depth's INTERIOR nodes and the next depth's SOLID children
        parallel_for(nr, nthreads, [&](int64_t b, int64_t e) {
            for (int64_t i = b; i < e; i++) {
                uint64_t mask = 0, kpos = base + koff[i], mpos = moff[i];
                for (int sl = 0; sl < 64; sl++) {
                    const int32_t x = cur[i].x0 + (sl & 3) * cs, y = cur[i].y0 + ((sl >> 2) & 3) * cs,
                                  z = cur[i].z0 + ((sl >> 4) & 3) * cs;
                    uint32_t c = classify_region(T, x, y, z, cs, levels - d - 1);
                    if (c == C_EMPTY) continue;
                    mask |= 1ull << sl;
                    if (c == C_MIXED) {
                        next[mpos] = Region{x, y, z};
                        next_node[mpos] = kpos;
                        mpos++;
                    } else {
                        t->nodes[kpos] = Node{~0ull, 0, K_SOLID | (c << 16)};
                    }
                    kpos++;
                }
                t->nodes[cur_node[i]] = Node{mask, (uint32_t)(base + koff[i]), K_INTERIOR};
            }
        });
        level_end = base + koff[nr];
        cur.swap(next);
        cur_node.swap(next_node);
    }
    if (t->nodes.size() > 0xFFFFFFFFull) {
        delete t;
        SVO_FAIL(SVO_ERANGE, "svo_build_terrain: tree exceeds 2^32 nodes");
    }
    *out = t;
    return SVO_OK;
}

extern "C" int svo_terrain_heights(int32_t width, int32_t length, int32_t nthreads, int32_t* out) {
    if (width < 0 || length < 0 || (!out && (int64_t)width * length > 0)) SVO_FAIL(SVO_EINVAL, "svo_terrain_heights: bad argument");
    terrain_heights(width, length, nthreads, [&](size_t i, int32_t h) { out[i] = h; });
    return SVO_OK;
}
