// Host code of libsvo_rt under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md §5 "race detection /
// sanitizers": on host code only — GPU sanitizers are not available on the pool).  Built and run by
// tests/test_sanitizers.py from every host file of raytracing_test_amd/csrc (build.py HOST_SRCS): world edits, every
// builder in both views, incremental updates (patch, growth, rebuild), lookups, export and the checkpoint round trip
// (svo_world.cpp, svo_linearise.cpp, svo_terrain.cpp, svo_tree.cpp, svo_tree_file.cpp); and from svo_plan.cpp, the
// launch planning: the frame octant, the segment test, the ceiling tables kept up to date over edits, the AO plan
// image, the sync bookkeeping, the frame schedule's decisions and the choice of the cast kernel's instance.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/svo_rt.h"
#include "../../raytracing_test_amd/csrc/svo_cast_instances.h"
#include "../../raytracing_test_amd/csrc/svo_plan.h"

// the device half of the library (the .hip files; svo_tree_destroy: svo_device.hip) is not built here: a tree is only ever host-side
extern "C" void svo_tree_destroy(svo_tree* t) { delete t; }

#define CHECK(x)                                                              \
    do {                                                                      \
        int rc_ = (x);                                                        \
        if (rc_) {                                                            \
            fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, svo_last_error()); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

#define EXPECT(x)                                                   \
    do {                                                            \
        if (!(x)) {                                                 \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #x); \
            exit(1);                                                \
        }                                                           \
    } while (0)

// the tables ceil_tables_update kept over the edits' rectangles against the tables rebuilt from the tree; the pair table's
// relation to the ceilings (tests/test_gpu_edits.py _pairs_of checks the same on the device's copy)
static void check_ceilings(svo_tree* t, int32_t n) {
    if (t->full_upload) {  // (a rebuilt tree is uploaded whole: svo_upload builds its tables)
        t->full_upload = false;
    } else {
        for (const auto& r : t->ceil_dirty) {
            int64_t zr[svo::kCeilMax][2], qr[2];
            svo::ceil_tables_update(t, n, r, zr, qr);
        }
    }
    t->ceil_dirty.clear();
    const std::vector<int16_t> c = t->ceil_host;
    const std::vector<uint32_t> p = t->ceilp_host;
    const std::vector<uint64_t> q = t->ceilq_host;
    EXPECT(svo::ceil_tables_build(t) == n);
    EXPECT(c == t->ceil_host && p == t->ceilp_host && q == t->ceilq_host);
    for (int32_t j = 0; j < n; j++) {
        const int64_t rows = (int64_t)1 << (2 * (t->levels - svo::kCeilK0 - j));
        const int32_t up = j + svo::kCeilPairStep < n ? j + svo::kCeilPairStep : n - 1, sh = 2 * (up - j);
        for (int64_t z = 0; z < rows; z++)
            for (int64_t x = 0; x < rows; x++) {
                const uint32_t v = p[t->ceil_off[j] + z * rows + x];
                EXPECT((int16_t)(v & 0xFFFFu) == c[t->ceil_off[j] + z * rows + x]);
                EXPECT((int16_t)(v >> 16) == c[t->ceil_off[up] + (z >> sh) * (rows >> sh) + (x >> sh)]);
            }
    }
}

static void check_frame_setup() {
    const float along_x[3] = {1.0f, 0.0f, 0.0f};
    svo::RayGen rg;
    for (int oct = 0; oct < 8; oct++) {
        const float v[3] = {oct & 1 ? -1.0f : 1.0f, oct & 2 ? -1.0f : 1.0f, oct & 4 ? -1.0f : 1.0f};
        float dir[3];
        CHECK(svo_normalize(v, dir));
        svo::raygen_init(rg, dir, 0.6f, 0.4f, 64, 36);
        EXPECT(svo::frame_dirs(rg, 64, 36, 0) == 1 + oct);  // (code = 1, plus 1 << a for each negative axis)
        EXPECT(svo::frame_dirs(rg, 64, 36, SVO_CAST_NO_OCTANT) == 0);
    }
    svo::raygen_init(rg, along_x, 0.6f, 0.4f, 64, 36);  // (a view along +x straddles y and z)
    EXPECT(svo::frame_dirs(rg, 64, 36, 0) == 0);
    const float a[3] = {4.0f, 90.0f, 4.0f}, b[3] = {4.5f, 90.0f, 4.5f}, c[3] = {4.25f, 90.0f, 4.0f};
    EXPECT(!svo::need_seg(0, false, 300, a, 1) && !svo::need_seg(0, false, 300, b, 1));
    EXPECT(svo::need_seg(0, false, 300, c, 1));
    EXPECT(svo::need_seg(0, false, 1 << 28, a, 1));
    EXPECT(svo::need_seg(0, true, 300, a, 1));
    EXPECT(svo::need_seg(SVO_CAST_SEGMENTS, false, 300, a, 1));
    double frac[3];
    int32_t cell[3];
    svo::frame_axes(1 + 2, c, frac, cell);  // (y steps down: its exact position is one below)
    EXPECT(cell[0] == 4 && cell[1] == 90 && cell[2] == 4 && frac[0] == 0.25 && frac[1] == -1.0 && frac[2] == 0.0);
}

// the image's layout (ao_count_plan, svo_shade.h): per (face, cell of the brick) a header {offset / 4, bricks}, then per
// brick 8 words {key, 0, voxel mask, sample mask, 0, 0} and a 64-bit sample mask per voxel of the mask, padded to 4 words
static void check_ao_plan(int32_t n, int32_t steps, bool planned) {
    std::vector<float> tab(3 * (size_t)n);
    svo::hemisphere_table(n, tab.data());
    const std::vector<uint32_t> img = svo::ao_plan_image(n, steps, tab.data());
    EXPECT(img.empty() == !planned);
    if (!planned) return;
    const uint64_t all = n == 64 ? ~0ull : (1ull << n) - 1;
    for (size_t g = 0; g < 6 * 64; g++) {
        EXPECT(2 * g + 1 < img.size());
        size_t at = (size_t)img[2 * g] * 4;
        uint64_t seen = 0;
        for (uint32_t b = 0; b < img[2 * g + 1]; b++) {
            EXPECT(at + 8 <= img.size());
            const uint64_t vm = img[at + 2] | ((uint64_t)img[at + 3] << 32), um = img[at + 4] | ((uint64_t)img[at + 5] << 32);
            const size_t words = 2 * (size_t)__builtin_popcountll(vm);
            EXPECT(at + 8 + words <= img.size());
            uint64_t of_voxels = 0;
            for (size_t k = 0; k < words; k += 2) of_voxels |= img[at + 8 + k] | ((uint64_t)img[at + 9 + k] << 32);
            EXPECT(of_voxels == um);
            seen |= um;
            at += (8 + words + 3) / 4 * 4;
        }
        // (the bricks of a cell end where the next cell's begin: every brick carried popcount(vm) masks)
        EXPECT(at == (g + 1 < 6 * 64 ? (size_t)img[2 * g + 2] * 4 : img.size()));
        EXPECT(seen == all);
    }
}

static void check_sync_state(svo_tree* t) {
    std::vector<uint32_t> dirty = {5, 3, 4, 9, 9, 10, 20};
    const auto runs = svo::dirty_runs(dirty);
    EXPECT(runs.size() == 3 && runs[0].first == 3 && runs[0].second == 5 && runs[1].first == 9 && runs[1].second == 10 &&
           runs[2].first == 20 && runs[2].second == 20);
    t->synced_nodes = t->nodes.size();  // (as after svo_upload)
    t->synced_mats = t->mats.size();
    t->dirty_nodes.clear();
    t->ceil_dirty.clear();
    t->palette_dirty = t->full_upload = false;
    EXPECT(!svo::tree_unsynced(t));
    t->nodes.push_back(svo::Node{0, 0, 0});
    EXPECT(svo::tree_unsynced(t));
    t->nodes.pop_back();
    t->mats.push_back(1);
    EXPECT(svo::tree_unsynced(t));
    t->mats.pop_back();
    t->dirty_nodes.push_back(0);
    EXPECT(svo::tree_unsynced(t));
    t->dirty_nodes.clear();
    t->palette_dirty = true;
    EXPECT(svo::tree_unsynced(t));
    t->palette_dirty = false;
    t->full_upload = true;
    EXPECT(svo::tree_unsynced(t));
    t->full_upload = false;
    t->ceil_dirty.push_back({0, 0, 16, 16});
    EXPECT(svo::tree_unsynced(t));
    t->ceil_dirty.clear();
    EXPECT(!svo::tree_unsynced(t));
}

// one frame on schedule s; a frame sorted after primes it (sched_order, svo_cast.hip, once the sort is queued)
static svo::SchedPlan sched_frame(svo_tree::Sched& s, const int64_t sig[7], const float cam[6]) {
    const svo::SchedPlan p = svo::sched_decide(s, 8192, sig, cam);
    EXPECT(p.write_cost == p.sort && s.blocks == 8192);
    if (p.sort) s.primed = true;
    return p;
}

static void check_schedule() {
    svo_tree::Sched s{};
    int64_t sig[7] = {1920, 1080, 1, 0, 1, 2, 0};
    float cam[6] = {4.0f, 90.0f, 4.0f, 0.0f, 0.0f, 1.0f};
    svo::SchedPlan p = sched_frame(s, sig, cam);  // (a new record has no last frame to be near to)
    EXPECT(!p.use_order && !p.sort && !s.primed);
    const auto settle = [&]() {  // a still camera: one frame primes, the next use its order, every kSchedEvery-th sorts again
        p = sched_frame(s, sig, cam);
        EXPECT(!p.use_order && p.write_cost && p.sort);
        for (int f = 1; f < svo::kSchedEvery; f++) {
            p = sched_frame(s, sig, cam);
            EXPECT(p.use_order && !p.write_cost && !p.sort);
        }
        p = sched_frame(s, sig, cam);
        EXPECT(p.use_order && p.write_cost && p.sort);
    };
    settle();
    cam[3] = sinf(0.0175f);  // a turn of 1 degree (kSchedTurnCos: half a degree)
    cam[5] = cosf(0.0175f);
    p = sched_frame(s, sig, cam);
    EXPECT(!p.use_order && !p.sort && !s.primed);
    settle();
    cam[0] += 1.5f * svo::kSchedMove;
    p = sched_frame(s, sig, cam);
    EXPECT(!p.use_order && !p.sort && !s.primed);
    settle();
    sig[0] = 1280;  // another frame geometry: the stored order is of other blocks
    p = sched_frame(s, sig, cam);
    EXPECT(!p.use_order && p.sort);
}

// Which k_cast instance a launch runs (svo::cast_instance) against the rule written out as rows, over every request; the
// results are exactly the instances that exist (svo_cast_instances.h: the lists the kernels are instantiated from).
// A row: the request fields it holds for (ANY: every value; dirs: ANY, 0 or NZ, any octant), then the instance (REQ: the
// request's field of that name).  Every request must fall under exactly one row.
enum { ANY = -1, REQ = -1, NZ = 1 };
struct InstanceRule {
    int stats, timeline, ao, shade, records, wide, dirs;  // (seg: ANY in every row)
    int STATS, STAMPS, AO, SHADE, WIDE, SEG, DIRS, NOREC;
};
static const InstanceRule kInstanceRules[] = {
    // stats timeline ao shade records wide dirs    STATS STAMPS AO SHADE WIDE SEG DIRS NOREC
    // primary and AO casts, the pick ray: counters bring the stamps; an AO launch has no timeline of its own
    {1, ANY, ANY, 0, ANY, ANY, ANY, /**/ 1, 1, REQ, 0, REQ, REQ, 0, 0},
    {0, 1, 0, 0, ANY, ANY, ANY, /**/ 0, 1, 0, 0, REQ, REQ, 0, 0},
    {0, ANY, 1, 0, ANY, 0, ANY, /**/ 0, 0, 1, 0, 0, REQ, REQ, 0},  // (the octant: narrow nodes only)
    {0, ANY, 1, 0, ANY, 1, ANY, /**/ 0, 0, 1, 0, 1, REQ, 0, 0},
    {0, 0, 0, 0, ANY, 0, ANY, /**/ 0, 0, 0, 0, 0, REQ, REQ, 0},
    {0, 0, 0, 0, ANY, 1, ANY, /**/ 0, 0, 0, 0, 1, REQ, 0, 0},
    // shading: diagnostics
    {1, ANY, ANY, 1, ANY, ANY, ANY, /**/ 1, 1, 0, 1, REQ, 1, 0, 0},
    {0, 1, ANY, 1, ANY, ANY, ANY, /**/ 0, 1, 0, 1, REQ, 1, 0, 0},
    // shading on the camera's octant: with hit records, without
    {0, 0, ANY, 1, 1, 0, NZ, /**/ 0, 0, 0, 1, 0, 1, REQ, 0},
    {0, 0, ANY, 1, 0, 0, NZ, /**/ 0, 0, 0, 1, 0, REQ, REQ, 1},
    // shading otherwise: wide nodes, or no common octant
    {0, 0, ANY, 1, ANY, 1, ANY, /**/ 0, 0, 0, 1, 1, 1, 0, 0},
    {0, 0, ANY, 1, ANY, 0, 0, /**/ 0, 0, 0, 1, 0, 1, 0, 0},
};

static bool same_instance(const svo::CastInstance& a, const svo::CastInstance& b) {
    return a.stats == b.stats && a.stamps == b.stamps && a.ao == b.ao && a.shade == b.shade && a.wide == b.wide && a.seg == b.seg &&
           a.dirs == b.dirs && a.norec == b.norec;
}

static void check_cast_instances() {
#define LISTED(...) {__VA_ARGS__},
    const std::vector<svo::CastInstance> listed = {SVO_CAST_ALL(LISTED)};
#undef LISTED
    std::vector<int> picked(listed.size(), 0);
    for (size_t i = 0; i < listed.size(); i++)
        for (size_t j = 0; j < i; j++) EXPECT(!same_instance(listed[i], listed[j]));
    const auto holds = [](int rule, int v) { return rule == ANY || rule == v; };
    const auto pick = [](int rule, int req) { return rule == REQ ? req : rule; };
    for (int bits = 0; bits < 128; bits++)
        for (int dirs = 0; dirs <= 8; dirs++) {
            const svo::CastRequest q = {(bits & 1) != 0,  (bits & 2) != 0,  (bits & 4) != 0,  (bits & 8) != 0,
                                        (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0, dirs};
            const svo::CastInstance k = svo::cast_instance(q);
            int rules = 0;
            for (const InstanceRule& r : kInstanceRules) {
                if (!(holds(r.stats, q.stats) && holds(r.timeline, q.timeline) && holds(r.ao, q.ao) && holds(r.shade, q.shade) &&
                      holds(r.records, q.records) && holds(r.wide, q.wide) && holds(r.dirs, dirs != 0)))
                    continue;
                rules++;
                const svo::CastInstance want = {r.STATS != 0, r.STAMPS != 0, pick(r.AO, q.ao) != 0, r.SHADE != 0, pick(r.WIDE, q.wide) != 0,
                                                pick(r.SEG, q.seg) != 0, pick(r.DIRS, dirs), r.NOREC != 0};
                EXPECT(same_instance(k, want));
            }
            EXPECT(rules == 1);
            size_t at = 0;
            while (at < listed.size() && !same_instance(listed[at], k)) at++;
            EXPECT(at < listed.size());
            picked[at]++;
        }
    for (size_t i = 0; i < listed.size(); i++) EXPECT(picked[i] > 0);
    // an octant code outside 1..8 counts as 8
    svo::CastRequest q = {};
    q.dirs = 9;
    EXPECT(svo::cast_instance(q).dirs == 8);
    q.dirs = -1;
    EXPECT(svo::cast_instance(q).dirs == 8);
}

static void probe(const svo_tree* t, int n, unsigned seed) {
    std::vector<int32_t> xyz(3 * n);
    for (int i = 0; i < 3 * n; i++) xyz[i] = (int32_t)((seed = seed * 1103515245u + 12345u) >> 8) % 2048 - 512;
    std::vector<uint32_t> ids(n);
    std::vector<uint64_t> idx(n);
    CHECK(svo_tree_get_blocks(t, xyz.data(), n, ids.data()));
    CHECK(svo_tree_node_indices(t, xyz.data(), n, idx.data()));
}

int main(int argc, char** argv) {
    const char* ckpt = argc > 1 ? argv[1] : "/tmp/sanitize_tree.svo";
    svo_world* w = nullptr;
    CHECK(svo_world_create(5, &w));
    CHECK(svo_init_tetra_hexa_tree(w));
    CHECK(svo_gen_world(w, 200, 200));
    for (int view = 0; view < 2; view++) {
        svo_tree* t = nullptr;
        CHECK(svo_build_view(w, view, &t));
        probe(t, 20000, 7 + view);
        const int32_t ceil_levels = svo::ceil_tables_build(t);
        EXPECT(ceil_levels == 3);
        // edits: voxels, 4^3 blocks, deletes, far away (wrap), then enough to force a rebuild
        unsigned s = 99;
        for (int round = 0; round < 6; round++) {
            std::vector<int32_t> xyz;
            for (int i = 0; i < 40; i++) {
                s = s * 1664525u + 1013904223u;
                xyz.push_back((int32_t)(s >> 8) % 260 - 20);
                xyz.push_back((int32_t)(s >> 16) % 80);
                xyz.push_back((int32_t)(s >> 4) % 260 - 20);
            }
            const int level = round % 3 == 2 ? 5 : 6;
            for (size_t i = 0; i < xyz.size() / 3; i++) {
                if (round % 2) {
                    svo_block removed;
                    CHECK(svo_delete_block(w, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], level, &removed));
                } else {
                    const svo_block b{(uint32_t)(i % 3 == 0 ? 0x14 : 0x2), 12345u + i, 0.0f};
                    CHECK(svo_put_block(w, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &b, level));
                }
            }
            CHECK(svo_tree_update(t, w, xyz.data(), (int64_t)(xyz.size() / 3), level));
            probe(t, 5000, s);
            check_ceilings(t, ceil_levels);
        }
        check_sync_state(t);
        svo_tree_info info;
        CHECK(svo_tree_get_info(t, &info));
        std::vector<uint8_t> nodes(info.n_nodes * 16), mats(info.n_mat_bytes + 2);
        CHECK(svo_tree_export(t, nodes.data(), nodes.size(), mats.data(), mats.size()));
        CHECK(svo_tree_save(t, ckpt));
        svo_tree* u = nullptr;
        CHECK(svo_tree_load(ckpt, &u));
        probe(u, 5000, 3);
        svo_tree_destroy(u);
        svo_tree_destroy(t);
    }
    svo_world_destroy(w);
    // the column builders, both views, ragged widths, and the heightfield builder
    for (int view = 0; view < 2; view++) {
        svo_tree* t = nullptr;
        CHECK(svo_build_terrain_view(5, 300, 170, 4, view, &t));
        probe(t, 20000, 11);
        svo_tree_destroy(t);
    }
    std::vector<int32_t> h(97 * 33);
    for (size_t i = 0; i < h.size(); i++) h[i] = (int32_t)(((uint32_t)(i * 2654435761u) >> 7) % 60u);
    svo_tree* t = nullptr;
    CHECK(svo_build_heightfield(4, 97, 33, h.data(), 3, &t));
    probe(t, 5000, 5);
    svo_tree_destroy(t);
    check_frame_setup();
    check_ao_plan(16, 8, true);
    check_ao_plan(20, 4, true);
    check_ao_plan(16, 128, false);
    check_ao_plan(65, 4, false);
    check_schedule();
    check_cast_instances();
    // error paths return codes (no exits, no leaks)
    svo_world* bad = nullptr;
    if (svo_world_create(9, &bad) == 0) return 1;
    if (svo_tree_load("/nonexistent/file.svo", &t) != SVO_EIO) return 1;
    float out[3];
    const float v[3] = {1.0f, -0.45f, 1.0f};
    CHECK(svo_normalize(v, out));
    printf("host sanitize ok\n");
    return 0;
}
