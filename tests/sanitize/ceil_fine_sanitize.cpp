// The fine column ceilings' host code under AddressSanitizer + UndefinedBehaviorSanitizer: the table built from small trees
// (svo_tree.cpp tree_ceilings_fine, through svo_plan.cpp ceil_tables_build) against a column scan by the tree's own voxel
// lookup, its update over the rectangles of edits (ceil_tables_update / ceil_tables_update_all) against the rebuild, and
// the bookkeeping svo_device.hip takes from svo_plan.cpp: the elements of the table a span of level-0 rows covers
// (ceil_fine_span) and which launches march on it (ceil_fine_for).  The level switch of the march itself is device code
// (svo_ceil_march.h) and keeps no host state.  Built and run by tests/test_ceil_fine_sanitize.py from every host file.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/svo_rt.h"
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

// [z][x] per 4 x 4 columns the highest row svo_tree_get_blocks finds a voxel in
static std::vector<int16_t> scan(const svo_tree* t) {
    const int32_t e = 1 << (2 * t->levels), rows = e >> svo::kCeilFineSh;
    std::vector<int16_t> top((size_t)rows * rows, (int16_t)-1);
    std::vector<int32_t> p((size_t)3 * e * e);
    std::vector<uint32_t> ids((size_t)e * e);
    for (int32_t y = 0; y < e; y++) {
        for (int32_t z = 0; z < e; z++)
            for (int32_t x = 0; x < e; x++) {
                int32_t* q = &p[3 * ((size_t)z * e + x)];
                q[0] = x;
                q[1] = y;
                q[2] = z;
            }
        CHECK(svo_tree_get_blocks(t, p.data(), (int64_t)e * e, ids.data()));
        for (int32_t z = 0; z < e; z++)
            for (int32_t x = 0; x < e; x++)
                if (ids[(size_t)z * e + x]) top[(size_t)(z >> svo::kCeilFineSh) * rows + (x >> svo::kCeilFineSh)] = (int16_t)y;
    }
    return top;
}

// the kept table is the scan's, and the C entry point hands out the same
static void check_table(svo_tree* t) {
    const std::vector<int16_t> want = scan(t);
    EXPECT(t->ceil_fine_host == want);
    // level 0 is kept from the fine table: the same as the walk that fills it directly
    std::vector<int16_t> direct;
    int64_t off[svo::kCeilMax] = {0, 0, 0, 0};
    (void)svo::tree_ceilings(t, direct, off);
    EXPECT(direct == t->ceil_host);
    int32_t sh = 0;
    int64_t n = 0;
    CHECK(svo_tree_ceilings_fine(t, nullptr, 0, &sh, &n));
    EXPECT(sh == svo::kCeilFineSh && n == (int64_t)want.size());
    std::vector<int16_t> got((size_t)n);
    CHECK(svo_tree_ceilings_fine(t, got.data(), n, &sh, &n));
    EXPECT(got == want);
    EXPECT(svo_tree_ceilings_fine(t, got.data(), n - 1, &sh, &n) == SVO_ERANGE);
}

static void put(svo_world* w, svo_tree* t, int32_t x, int32_t y, int32_t z, uint64_t colour, int32_t level) {
    const svo_block b = {1u, colour, 0.0f};
    const int32_t p[3] = {x, y, z};
    CHECK(svo_put_block(w, x, y, z, &b, level));
    if (t) CHECK(svo_tree_update(t, w, p, 1, level));
}

static void del(svo_world* w, svo_tree* t, int32_t x, int32_t y, int32_t z, int32_t level) {
    const int32_t p[3] = {x, y, z};
    svo_block gone;
    CHECK(svo_delete_block(w, x, y, z, level, &gone));
    CHECK(svo_tree_update(t, w, p, 1, level));
}

// the tables brought up to date over the tree's dirty rectangles, one call per rectangle or all at once
static void settle(svo_tree* t, int32_t n, bool at_once) {
    if (t->full_upload) {  // (a rebuilt tree is uploaded whole: svo_upload builds its tables)
        t->full_upload = false;
        EXPECT(svo::ceil_tables_build(t) == n);
    } else if (at_once) {
        svo::CeilRows rows;
        svo::ceil_tables_update_all(t, n, t->ceil_dirty, &rows);
        const int64_t total = (int64_t)t->ceil_fine_host.size();
        for (const auto& z : rows.level[0]) {  // what sync_ceilings would copy lies inside the table
            const svo::CeilFineSpan f = svo::ceil_fine_span(t, z);
            EXPECT(f.first >= 0 && f.count >= 0 && f.first + f.count <= total);
        }
    } else {
        for (const auto& r : t->ceil_dirty) {
            int64_t zr[svo::kCeilMax][2], qr[2];
            svo::ceil_tables_update(t, n, r, zr, qr);
        }
    }
    t->ceil_dirty.clear();
    check_table(t);
}

static void run(int32_t levels) {
    svo_world* w = nullptr;
    svo_tree* t = nullptr;
    CHECK(svo_world_create(levels, &w));
    const int32_t e = 1 << (2 * levels), vox = levels + 1;
    // a slope of single voxels, a 16^3 SOLID region above the brick level, a voxel in the last column
    for (int32_t i = 0; i < e; i += 3) put(w, nullptr, i, (i * 7) % e, (i * 5) % e, 100 + i, vox);
    put(w, nullptr, 16, 32, 16, 7, levels - 1);
    put(w, nullptr, e - 1, e - 1, e - 1, 8, vox);
    CHECK(svo_build(w, &t));
    const int32_t n = svo::ceil_tables_build(t);
    EXPECT(n == std::min<int32_t>(svo::kCeilMax, levels - svo::kCeilK0) && n > 0);
    EXPECT((int64_t)t->ceil_fine_host.size() == (int64_t)(e >> svo::kCeilFineSh) * (e >> svo::kCeilFineSh));
    check_table(t);
    // the whole table is one span of every level-0 row, none is empty, rows past the end are clipped
    const int64_t rows0 = e >> (2 * svo::kCeilK0);
    svo::CeilFineSpan f = svo::ceil_fine_span(t, {0, rows0});
    EXPECT(f.first == 0 && f.count == (int64_t)t->ceil_fine_host.size());
    f = svo::ceil_fine_span(t, {1, 1});
    EXPECT(f.count == 0);
    f = svo::ceil_fine_span(t, {rows0 - 1, rows0 + 5});
    EXPECT(f.first + f.count == (int64_t)t->ceil_fine_host.size() && f.count == 4 * (int64_t)(e >> svo::kCeilFineSh));
    // edits: a column raised and one lowered inside one 4-column block, the SOLID region cut into, the last column cleared
    put(w, t, 5, e - 2, 6, 9, vox);
    del(w, t, 6, (6 * 7) % e, (6 * 5) % e, vox);
    settle(t, n, false);
    del(w, t, 20, 47, 20, vox);
    del(w, t, e - 1, e - 1, e - 1, vox);
    put(w, t, e - 1, 3, 0, 10, vox);
    settle(t, n, true);
    for (int32_t i = 0; i < e; i += 3)  // (many rectangles at once)
        if (i != 6) del(w, t, i, (i * 7) % e, (i * 5) % e, vox);
    settle(t, n, true);
    svo_tree_destroy(t);
    svo_world_destroy(w);
}

int main() {
    run(3);
    run(4);
    // a tree too shallow for ceilings has no fine table, and its updates are no-ops
    svo_world* w = nullptr;
    svo_tree* t = nullptr;
    CHECK(svo_world_create(2, &w));
    put(w, nullptr, 3, 4, 5, 1, 3);
    CHECK(svo_build(w, &t));
    EXPECT(svo::ceil_tables_build(t) == 0 && t->ceil_fine_host.empty());
    svo::ceilings_update_rect(t, t->ceil_host, t->ceil_off, 0, 0, 0, 16, 16, &t->ceil_fine_host);
    EXPECT(t->ceil_fine_host.empty() && t->ceil_host.empty());
    int32_t sh = 0;
    int64_t n = -1;
    CHECK(svo_tree_ceilings_fine(t, nullptr, 0, &sh, &n));
    EXPECT(n == 0);
    svo_tree_destroy(t);
    svo_world_destroy(w);
    // an empty world
    CHECK(svo_world_create(3, &w));
    CHECK(svo_build(w, &t));
    (void)svo::ceil_tables_build(t);
    for (int16_t v : t->ceil_fine_host) EXPECT(v == -1);
    svo_tree_destroy(t);
    svo_world_destroy(w);
    EXPECT(svo::ceil_fine_for(2, 0) && svo::ceil_fine_for(1, 0) && !svo::ceil_fine_for(0, 0) && !svo::ceil_fine_for(2, 1));
    printf("ceil fine sanitize ok\n");
    return 0;
}
