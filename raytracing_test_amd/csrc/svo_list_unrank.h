// svo_list_unrank.h — the box arithmetic of svo_tree_list_voxels_gpu (svo_list_voxels.hip), shared by its kernels and the
// host: no HIP, so it also builds with g++ and runs on a CPU (tests/sanitize/list_voxels_plan_sanitize.cpp).  A box is
// [lo, hi) per axis inside the extent; a region is an aligned cube of edge s = 4^k at p.  The voxels of a region inside the
// box, in key order (6 bits per level, the top level first, slot z<<4 | y<<2 | x), are numbered 0 .. count - 1; list_unrank
// finds the q-th without visiting the others: per level the 64 sub-cells' clipped counts are separable (lz * ly * lx), so
// the digit of each axis is found by at most three comparisons against a running product.
#pragma once

#include <stdint.h>

#include "svo_common.h"

namespace svo {

struct ListBox {
    int32_t lo[3], hi[3];  // x, y, z
};

// voxels of [a, a + c) inside [lo, hi)
SVO_HD int32_t list_clip_len(int32_t a, int32_t c, int32_t lo, int32_t hi) {
    const int32_t b = a + c < hi ? a + c : hi, f = a > lo ? a : lo;
    return b > f ? b - f : 0;
}

// voxels of the region of edge s at (x, y, z) inside the box: the product of its three clipped edge lengths
SVO_HD uint64_t list_clip_volume(int32_t x, int32_t y, int32_t z, int32_t s, const ListBox& B) {
    return (uint64_t)list_clip_len(x, s, B.lo[0], B.hi[0]) * (uint64_t)list_clip_len(y, s, B.lo[1], B.hi[1]) *
           (uint64_t)list_clip_len(z, s, B.lo[2], B.hi[2]);
}

// which of the four cells of edge c along one axis, from p on, holds entry q, every voxel of the axis standing for `per`
// entries; q is reduced to the entry within that cell's slab, *len: the cell's clipped length
SVO_HD int32_t list_pick_cell(int32_t p, int32_t c, int32_t lo, int32_t hi, uint64_t per, uint64_t& q, uint64_t* len) {
    for (int32_t i = 0; i < 3; i++) {
        const uint64_t l = (uint64_t)list_clip_len(p + i * c, c, lo, hi);
        if (q < l * per) {
            *len = l;
            return i;
        }
        q -= l * per;
    }
    *len = (uint64_t)list_clip_len(p + 3 * c, c, lo, hi);
    return 3;
}

// the q-th voxel, in key order, of the region of edge s at p[] inside the box (q < list_clip_volume): p[] becomes it
SVO_HD void list_unrank(int32_t p[3], int32_t s, const ListBox& B, uint64_t q) {
    uint64_t lx = (uint64_t)list_clip_len(p[0], s, B.lo[0], B.hi[0]), ly = (uint64_t)list_clip_len(p[1], s, B.lo[1], B.hi[1]), lz = 0;
    for (int32_t c = s >> 2; c >= 1; c >>= 2) {  // a digit per level: z, then y, then x, as the key's slot
        const uint64_t LX = lx, LY = ly;
        const int32_t sz = list_pick_cell(p[2], c, B.lo[2], B.hi[2], LY * LX, q, &lz);
        const int32_t sy = list_pick_cell(p[1], c, B.lo[1], B.hi[1], lz * LX, q, &ly);
        const int32_t sx = list_pick_cell(p[0], c, B.lo[0], B.hi[0], lz * ly, q, &lx);
        p[0] += sx * c;
        p[1] += sy * c;
        p[2] += sz * c;
    }
}

}  // namespace svo
