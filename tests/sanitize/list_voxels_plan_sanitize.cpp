// list_voxels_plan_sanitize.cpp — the host half of svo_tree_list_voxels_gpu under AddressSanitizer + UBSan: svo_plan.cpp's
// list_box (the box check and clip) and svo_list_unrank.h's closed-form count and digit-by-digit unranking, which the
// kernels share, against a brute-force enumeration of the box's voxels sorted by key — over boxes that touch each face of
// the extent, single voxels in its corners and boxes that straddle region boundaries of every level, at levels 1 and 7.
// Built and run by tests/test_list_voxels_plan_host.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../raytracing_test_amd/csrc/svo_plan.h"

using namespace svo;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            fails++;                                                \
        }                                                           \
    } while (0)

// svo_points_source.h voxel_key, restated: 6 bits per level, z<<4 | y<<2 | x, the top level first
static uint64_t key(uint32_t x, uint32_t y, uint32_t z, int32_t levels) {
    uint64_t k = 0;
    for (int d = 0; d < levels; d++) {
        const uint32_t sh = (uint32_t)(2 * (levels - 1 - d));
        k = (k << 6) | (uint64_t)((((z >> sh) & 3u) << 4) | (((y >> sh) & 3u) << 2) | ((x >> sh) & 3u));
    }
    return k;
}

struct Vox {
    uint64_t k;
    int32_t x, y, z;
};

// the region of edge s at (rx, ry, rz) against the box at origin o of (nx, ny, nz) voxels: count and every rank
static void check(int32_t levels, int32_t rx, int32_t ry, int32_t rz, int32_t s, const int32_t o[3], int32_t nx, int32_t ny, int32_t nz) {
    ListBox B;
    CHECK(list_box(levels, o, nx, ny, nz, &B) == LIST_BOX_OK);
    CHECK(B.lo[0] == o[0] && B.lo[1] == o[1] && B.lo[2] == o[2] && B.hi[0] == o[0] + nx && B.hi[1] == o[1] + ny && B.hi[2] == o[2] + nz);
    std::vector<Vox> want;
    for (int32_t z = std::max(rz, B.lo[2]); z < std::min(rz + s, B.hi[2]); z++)
        for (int32_t y = std::max(ry, B.lo[1]); y < std::min(ry + s, B.hi[1]); y++)
            for (int32_t x = std::max(rx, B.lo[0]); x < std::min(rx + s, B.hi[0]); x++)
                want.push_back(Vox{key((uint32_t)x, (uint32_t)y, (uint32_t)z, levels), x, y, z});
    std::sort(want.begin(), want.end(), [](const Vox& a, const Vox& b) { return a.k < b.k; });
    const uint64_t n = list_clip_volume(rx, ry, rz, s, B);
    CHECK(n == want.size());
    if (n != want.size()) return;
    Vox* exact = (Vox*)malloc(sizeof(Vox) * (n ? n : 1));  // (its exact size: a read past the count is reported)
    std::copy(want.begin(), want.end(), exact);
    int bad = 0;
    for (uint64_t q = 0; q < n; q++) {
        int32_t p[3] = {rx, ry, rz};
        list_unrank(p, s, B, q);
        bad += !(p[0] == exact[q].x && p[1] == exact[q].y && p[2] == exact[q].z);
    }
    free(exact);
    CHECK(bad == 0);
}

int main() {
    ListBox B;
    for (int32_t levels : {1, 7}) {
        const int32_t E = 1 << (2 * levels);
        CHECK(list_box(levels, nullptr, 0, 0, 0, &B) == LIST_BOX_OK && B.lo[0] == 0 && B.lo[1] == 0 && B.lo[2] == 0);
        CHECK(B.hi[0] == E && B.hi[1] == E && B.hi[2] == E);
        CHECK(list_box(levels, nullptr, -3, 0, 7, &B) == LIST_BOX_OK);  // (the dimensions are ignored)
        const int32_t z0[3] = {0, 0, 0}, neg[3] = {0, -1, 0}, last[3] = {E - 1, E - 1, E - 1}, past[3] = {0, 0, E};
        const int32_t huge[3] = {0x7FFFFFFF, 0, 0};
        CHECK(list_box(levels, z0, E, E, E, &B) == LIST_BOX_OK && B.hi[0] == E && B.hi[2] == E);
        CHECK(list_box(levels, z0, 0, 1, 1, &B) == LIST_BOX_DIM);
        CHECK(list_box(levels, z0, 1, -1, 1, &B) == LIST_BOX_DIM);
        CHECK(list_box(levels, z0, 1, 1, 0, &B) == LIST_BOX_DIM);
        CHECK(list_box(levels, neg, 1, 1, 1, &B) == LIST_BOX_EXTENT);
        CHECK(list_box(levels, z0, E + 1, 1, 1, &B) == LIST_BOX_EXTENT);
        CHECK(list_box(levels, last, 1, 1, 1, &B) == LIST_BOX_OK && B.lo[1] == E - 1 && B.hi[1] == E);
        CHECK(list_box(levels, last, 1, 2, 1, &B) == LIST_BOX_EXTENT);
        CHECK(list_box(levels, past, 1, 1, 1, &B) == LIST_BOX_EXTENT);
        CHECK(list_box(levels, huge, 0x7FFFFFFF, 1, 1, &B) == LIST_BOX_EXTENT);  // (no wrap of the 32-bit sum)
    }

    {  // level 1: the extent is one brick-sized region
        const int32_t whole[3] = {0, 0, 0};
        check(1, 0, 0, 0, 4, whole, 4, 4, 4);
        for (int a = 0; a < 3; a++)
            for (int32_t side : {0, 3}) {  // the six faces, as slabs one voxel thick
                int32_t o[3] = {0, 0, 0}, n[3] = {4, 4, 4};
                o[a] = side;
                n[a] = 1;
                check(1, 0, 0, 0, 4, o, n[0], n[1], n[2]);
            }
        for (int32_t x : {0, 3})
            for (int32_t y : {0, 3})
                for (int32_t z : {0, 3}) {
                    const int32_t o[3] = {x, y, z};
                    check(1, 0, 0, 0, 4, o, 1, 1, 1);
                }
        const int32_t off[3] = {1, 2, 1};
        check(1, 0, 0, 0, 4, off, 3, 1, 2);
    }
    {  // level 7: the whole extent as one K_SOLID region, boxes off every grid
        const int32_t E = 16384;
        for (int a = 0; a < 3; a++)
            for (int side = 0; side < 2; side++) {  // touching each face, straddling region boundaries on the other axes
                int32_t o[3] = {4093, 8190, 12287}, n[3] = {7, 5, 6};
                o[a] = side ? E - n[a] : 0;
                check(7, 0, 0, 0, E, o, n[0], n[1], n[2]);
            }
        for (int32_t x : {0, E - 1})
            for (int32_t y : {0, E - 1})
                for (int32_t z : {0, E - 1}) {
                    const int32_t o[3] = {x, y, z};
                    check(7, 0, 0, 0, E, o, 1, 1, 1);
                }
        const int32_t mid[3] = {4093, 8190, 12287};   // boundaries of 4096, 2 and 1 meet 4096 * k here
        check(7, 0, 0, 0, E, mid, 10, 9, 11);
        check(7, 4096, 8192, 12288, 4096, mid, 10, 9, 11);   // a region one level down that the box only cuts
        check(7, 4092, 8188, 12284, 4, mid, 10, 9, 11);      // a brick-sized region on the box's corner
        check(7, 0, 0, 0, 4096, mid, 10, 9, 11);             // a region the box misses: nothing to unrank
        const int32_t slab[3] = {0, 16383, 0};
        check(7, 0, 0, 0, E, slab, 40, 1, 40);
        const int32_t line[3] = {16300, 5, 16383};
        check(7, 0, 0, 0, E, line, 84, 1, 1);
    }
    if (fails) return 1;
    printf("list voxels plan sanitize ok\n");
    return 0;
}
