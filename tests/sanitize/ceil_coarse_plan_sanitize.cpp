// The host half of the march's coarse levels under AddressSanitizer + UndefinedBehaviorSanitizer: which levels of the
// ceiling table a launch's march walks before its first (svo_plan.cpp march_levels), over every tree depth the ABI admits
// (1 .. 7 levels), every table size (0 .. kCeilMax levels) and every first level, against the rule restated here; and the
// offset arithmetic set_ceilings takes from svo_plan.cpp (march_params) over small trees of 2 .. 5 levels: every level handed
// to the kernel lies inside the tree's table with all its rows, is 4 times as wide as the next, and the last 4 times as
// wide as the launch's first.  The table is printed, one line per case, for tests/test_ceil_coarse_host.py to hold against
// its own restatement.  The march itself is device code (svo_ceil_march.h) and keeps no host state.
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

// the rule, restated: the levels above `first` that the table has, at most kMarchCoarseMax of them, each with at least
// 2 x 2 blocks in a tree of `levels` levels; coarsest first
static std::vector<int32_t> want_levels(int32_t ceil_levels, int32_t first, int32_t levels) {
    std::vector<int32_t> v;
    if (ceil_levels <= first) return v;
    for (int32_t l = first + 1; l < std::min<int32_t>(ceil_levels, svo::kCeilMax) && l <= first + svo::kMarchCoarseMax; l++) {
        const int32_t lg_rows = 2 * (levels - svo::kCeilK0 - l);  // log2 of the blocks per row
        if (lg_rows >= 1) v.insert(v.begin(), l);
    }
    return v;
}

static void plan_table() {
    for (int32_t levels = 1; levels <= 7; levels++)
        for (int32_t ceil_levels = 0; ceil_levels <= svo::kCeilMax; ceil_levels++)
            for (int32_t first = 0; first < svo::kCeilMax; first++) {
                const svo::MarchLevels m = svo::march_levels(ceil_levels, first, levels);
                const std::vector<int32_t> want = want_levels(ceil_levels, first, levels);
                EXPECT(m.n == (int32_t)want.size() && m.n >= 0 && m.n <= svo::kMarchCoarseMax);
                for (int32_t j = 0; j < m.n; j++) EXPECT(m.level[j] == want[j]);
                printf("plan %d %d %d :", levels, ceil_levels, first);
                for (int32_t j = 0; j < m.n; j++) printf(" %d", m.level[j]);
                printf("\n");
            }
    EXPECT(svo::march_levels(3, -1, 5).n == 0);
}

static void params(int32_t levels) {
    svo_world* w = nullptr;
    svo_tree* t = nullptr;
    CHECK(svo_world_create(levels, &w));
    const int32_t e = 1 << (2 * levels);
    const svo_block b = {1u, 7u, 0.0f};
    for (int32_t i = 0; i < e; i += std::max(3, e / 40)) CHECK(svo_put_block(w, i, (i * 7) % e, (i * 5) % e, &b, levels + 1));
    CHECK(svo_build(w, &t));
    const int32_t n = svo::ceil_tables_build(t);
    t->ceil_levels = n;  // (svo_upload sets it with the tables: a host tree carries the count here)
    EXPECT(n == std::max(0, std::min<int32_t>(svo::kCeilMax, levels - svo::kCeilK0)));
    for (int32_t first = 0; first < svo::kCeilMax; first++)
        for (int32_t launch = 0; launch <= 2; launch++) {
            const svo::MarchParams p = svo::march_params(t, launch, first);
            const svo::MarchLevels m = svo::march_levels(n, first, levels);
            EXPECT(p.n == (launch > 0 ? m.n : 0));
            uint32_t next_sh = 2u * (uint32_t)(svo::kCeilK0 + first);
            for (int32_t j = p.n - 1; j >= 0; j--) {  // finest to coarsest: each 4 times as wide
                EXPECT(p.sh[j] == next_sh + 2u);
                next_sh = p.sh[j];
                const int64_t rows = (int64_t)e >> p.sh[j];
                EXPECT(rows >= 2);
                EXPECT(p.off[j] == t->ceil_off[m.level[j]] && p.off[j] >= 0 && p.off[j] + rows * rows <= (int64_t)t->ceil_host.size());
                // the level's own table: every block's ceiling is the maximum of its four by four children one level down
                const int64_t lower = m.level[j] - 1 >= 0 ? t->ceil_off[m.level[j] - 1] : -1;
                for (int64_t z = 0; z < rows && lower >= 0; z++)
                    for (int64_t x = 0; x < rows; x++) {
                        int16_t mx = -1;
                        for (int64_t k = 0; k < 16; k++) mx = std::max(mx, t->ceil_host[(size_t)(lower + (4 * z + k / 4) * 4 * rows + 4 * x + k % 4)]);
                        EXPECT(t->ceil_host[(size_t)(p.off[j] + z * rows + x)] == mx);
                    }
            }
            printf("params %d %d %d :", levels, first, launch);
            for (int32_t j = 0; j < p.n; j++) printf(" %u@%lld", p.sh[j], (long long)p.off[j]);
            printf("\n");
        }
    svo_tree_destroy(t);
    svo_world_destroy(w);
}

int main() {
    plan_table();
    for (int32_t levels = 2; levels <= 5; levels++) params(levels);
    printf("ceil coarse plan sanitize ok\n");
    return 0;
}
