// svo_world.cpp — the editable 64-ary voxel world of libsvo_rt's host side (the reference's putBlock / getBlock /
// deleteBlock / genWorld API), with the library's thread-local error state and parallel_for.  svo_linearise.cpp turns a
// world into the breadth-first tree the gfx950 kernel walks.  Reference paths are relative to the
// reedthorngag/raytracing_test snapshot.
#include <algorithm>
#include <atomic>
#include <thread>

#include "svo_world.h"

using namespace svo;

static thread_local std::string g_err;
void svo::set_error(const std::string& msg) { g_err = msg; }

extern "C" const char* svo_last_error(void) { return g_err.c_str(); }
extern "C" int svo_version(void) { return SVO_RT_VERSION; }

void svo::parallel_for(int64_t n, int nthreads, const std::function<void(int64_t, int64_t)>& fn) {
    // default: the machine's threads, at most 16 (a GPU box exposes many more cores than its share)
    if (nthreads <= 0) nthreads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    nthreads = (int)std::min<int64_t>(nthreads, std::max<int64_t>(1, n / 64));
    if (nthreads <= 1 || n < 2) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    std::atomic<int64_t> next(0);
    const int64_t chunk = std::max<int64_t>(1, n / (nthreads * 8));
    for (int i = 0; i < nthreads; i++)
        th.emplace_back([&] {
            for (;;) {
                int64_t b = next.fetch_add(chunk);
                if (b >= n) break;
                fn(b, std::min(n, b + chunk));
            }
        });
    for (auto& t : th) t.join();
}

extern "C" int svo_world_create(int32_t levels, svo_world** out) {
    if (!out) SVO_FAIL(SVO_EINVAL, "svo_world_create: out is NULL");
    if (levels < 1 || levels > 7) SVO_FAIL(SVO_EINVAL, "svo_world_create: levels must be in [1, 7]");
    svo_world* w = new (std::nothrow) svo_world();
    if (!w) SVO_FAIL(SVO_ENOMEM, "svo_world_create: out of memory");
    w->levels = levels;
    w->new_node(0, 0);  // root: an empty branch (tetrahexa_tree.cpp:15-18)
    *out = w;
    return SVO_OK;
}

extern "C" void svo_world_destroy(svo_world* w) { delete w; }

extern "C" int svo_world_node_count(const svo_world* w, uint64_t* n) {
    if (!w || !n) SVO_FAIL(SVO_EINVAL, "svo_world_node_count: NULL argument");
    *n = w->live_nodes;
    return SVO_OK;
}

static int put_block_id(svo_world* w, int32_t x, int32_t y, int32_t z, uint16_t mat, int32_t level) {
    const int target = level - 1;  // putBlock: `level--` (tetrahexa_tree.cpp:178)
    const uint32_t mk = wrap_mask(w->levels);
    const uint32_t wx = (uint32_t)x & mk, wy = (uint32_t)y & mk, wz = (uint32_t)z & mk;
    uint32_t n = 0;
    for (int depth = 0;; depth++) {
        if (depth == target) {
            w->make_leaf(n, mat);
            return SVO_OK;
        }
        if (w->nodes[n].leaf) w->split(n);
        const uint32_t slot = child_slot(wx, wy, wz, (uint32_t)(2 * (w->levels - 1 - depth)));
        uint32_t c = w->kids(n)[slot];
        if (!c) {
            if (depth + 1 == target) {
                c = w->new_node(1, mat);
                w->kids(n)[slot] = c;
                return SVO_OK;
            }
            c = w->new_node(0, 0);
            w->kids(n)[slot] = c;
        }
        n = c;
    }
}

extern "C" int svo_put_block(svo_world* w, int32_t x, int32_t y, int32_t z, const svo_block* b, int32_t level) {
    if (!w || !b) SVO_FAIL(SVO_EINVAL, "svo_put_block: NULL argument");
    if (level < 1 || level > w->levels + 1) SVO_FAIL(SVO_EINVAL, "svo_put_block: level out of range");
    int id = w->pal.intern(Material{1u | b->flags, b->color, b->metadata});
    if (id < 0) SVO_FAIL(SVO_ERANGE, "svo_put_block: more than 65534 distinct blocks");
    return put_block_id(w, x, y, z, (uint16_t)id, level);
}

extern "C" int svo_get_block(const svo_world* w, int32_t x, int32_t y, int32_t z, svo_block* out) {
    if (!w || !out) SVO_FAIL(SVO_EINVAL, "svo_get_block: NULL argument");
    const uint32_t mk = wrap_mask(w->levels);
    const uint32_t wx = (uint32_t)x & mk, wy = (uint32_t)y & mk, wz = (uint32_t)z & mk;
    uint32_t n = 0;
    for (int depth = 0; depth <= w->levels; depth++) {
        if (w->nodes[n].leaf) {
            *out = to_block(w->pal.m[w->nodes[n].mat]);
            return SVO_OK;
        }
        if (depth == w->levels) break;
        uint32_t c = w->kids(n)[child_slot(wx, wy, wz, (uint32_t)(2 * (w->levels - 1 - depth)))];
        if (!c) {
            *out = svo_block{0, ~0ull, 0.0f};
            return SVO_OK;
        }
        n = c;
    }
    SVO_FAIL(SVO_ESTATE, "svo_get_block: branch at voxel depth (corrupt world)");
}

extern "C" int svo_delete_block(svo_world* w, int32_t x, int32_t y, int32_t z, int32_t level, svo_block* removed) {
    if (!w) SVO_FAIL(SVO_EINVAL, "svo_delete_block: NULL world");
    if (level < 1 || level > w->levels + 1) SVO_FAIL(SVO_EINVAL, "svo_delete_block: level out of range");
    const int target = level - 1;
    const uint32_t mk = wrap_mask(w->levels);
    const uint32_t wx = (uint32_t)x & mk, wy = (uint32_t)y & mk, wz = (uint32_t)z & mk;
    svo_block found{0, ~0ull, 0.0f};
    if (target == 0) {
        if (w->nodes[0].leaf) found = to_block(w->pal.m[w->nodes[0].mat]);
        w->drop_children(0);
        w->nodes[0].leaf = 0;
        w->nodes[0].kids = w->new_block();
        if (removed) *removed = found;
        return SVO_OK;
    }
    uint32_t n = 0;
    for (int depth = 0;; depth++) {
        if (w->nodes[n].leaf) w->split(n);
        const uint32_t slot = child_slot(wx, wy, wz, (uint32_t)(2 * (w->levels - 1 - depth)));
        uint32_t c = w->kids(n)[slot];
        if (!c) break;  // already empty
        if (depth + 1 == target) {
            if (w->nodes[c].leaf) found = to_block(w->pal.m[w->nodes[c].mat]);
            w->drop_children(c);
            w->free_nodes.push_back(c);
            w->live_nodes--;
            w->kids(n)[slot] = 0;
            break;
        }
        n = c;
    }
    if (removed) *removed = found;
    return SVO_OK;
}

// initTetraHexaTree's debug blocks (tetrahexa_tree.cpp:20-27)
extern "C" int svo_init_tetra_hexa_tree(svo_world* w) {
    if (!w) SVO_FAIL(SVO_EINVAL, "svo_init_tetra_hexa_tree: NULL world");
    struct P {
        int x, y, z;
        uint32_t f;
        int level;
    } puts[8] = {{1000, 1000, 1000, 1, 5}, {10, 100, 10, 2, 6}, {100, 10, 100, 3, 6}, {20, 10, 200, 4, 5},
                 {1, 10, 10, 5, 6},        {2, 10, 10, 6, 6},    {3, 10, 10, 7, 6},    {4, 10, 10, 8, 6}};
    // the reference's levels are for maxDepth 6; rescale so "6" stays one voxel
    for (auto& p : puts) {
        svo_block b{p.f, 0ull, 0.0f};
        int lv = p.level + (w->levels - 5);
        if (lv < 1) lv = 1;
        int rc = svo_put_block(w, p.x, p.y, p.z, &b, lv);
        if (rc) return rc;
    }
    return SVO_OK;
}

// genWorld's column puts (world_gen.cpp:24-39) for one column with top y
static void gen_column(svo_world* w, int32_t x, int32_t z, int32_t y);

// genWorld (world_gen.cpp:13-42) over width x length columns
extern "C" int svo_gen_world(svo_world* w, int32_t width, int32_t length) {
    if (!w || width < 0 || length < 0) SVO_FAIL(SVO_EINVAL, "svo_gen_world: bad argument");
    const TerrainNoise tn;
    for (int32_t x = 0; x < width; x++)
        for (int32_t z = 0; z < length; z++) gen_column(w, x, z, tn.height(x, z));
    return SVO_OK;
}

// the same puts from caller-given column tops heights[x*length + z]
extern "C" int svo_gen_heightfield(svo_world* w, int32_t width, int32_t length, const int32_t* heights) {
    if (!w || width < 0 || length < 0 || (!heights && (int64_t)width * length > 0)) SVO_FAIL(SVO_EINVAL, "svo_gen_heightfield: bad argument");
    for (int32_t x = 0; x < width; x++)
        for (int32_t z = 0; z < length; z++) gen_column(w, x, z, heights[(size_t)x * length + z]);
    return SVO_OK;
}

static void gen_column(svo_world* w, int32_t x, int32_t z, int32_t y) {
    const uint64_t green = rgb_to_u64(0, 150, 10), brown = rgb_to_u64(45, 18, 0), grey = rgb_to_u64(33, 33, 33);
    const int32_t voxel = w->levels + 1;
    auto id = [&](uint32_t f, uint64_t c) { return (uint16_t)w->pal.intern(Material{1u | f, c, 0.0f}); };
    if (y < 20) {
        const uint16_t water = id(0x4u | 0x10u, green);
        for (int32_t i = 20; i > y; i--) put_block_id(w, x, i, z, water, voxel);
        put_block_id(w, x, y, z, id(0, brown), voxel);
    } else {
        put_block_id(w, x, y, z, id(0, green), voxel);
    }
    y--;
    for (int i = 3; y > 0 && i; i--, y--) put_block_id(w, x, y, z, id(0, brown), voxel);
    for (; y > 0; y--) put_block_id(w, x, y, z, id(0, grey), voxel);
}

extern "C" int svo_get_blocks(const svo_world* w, const int32_t* xyz, int64_t n, svo_block* out) {
    if (!w || ((!xyz || !out) && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_get_blocks: NULL argument");
    for (int64_t i = 0; i < n; i++) {
        int rc = svo_get_block(w, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &out[i]);
        if (rc) return rc;
    }
    return SVO_OK;
}

extern "C" int svo_put_blocks(svo_world* w, const int32_t* xyz, const svo_block* b, int64_t n, int32_t level) {
    if (!w || ((!xyz || !b) && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_put_blocks: NULL argument");
    for (int64_t i = 0; i < n; i++) {
        int rc = svo_put_block(w, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &b[i], level);
        if (rc) return rc;
    }
    return SVO_OK;
}
