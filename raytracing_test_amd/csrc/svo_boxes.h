// svo_boxes.h — forward boxes from a parent's 64-bit child mask: runs of free cells (run_fwd), the box of empty sibling
// slots ahead of the ray (box_exits), and a child's occupancy and rank (slot_top, popc_add).  No memory traffic.
// Used by svo_lookup.h (the descent) and by trace() in svo_trace.h (the box an empty cell grows into).
#pragma once

#include "svo_cast_params.h"

// A run of free cells through a 4-cell line (occupancy bits 0-3; higher bits are ignored) from the
// ray's cell c (free itself) in its step direction: t = cells in the run (>= 1), m = their slots.
// A sentinel bit stands for the end of the line: one ctz (up) or one clz (down) finds the run.
// ((1 << w) - 1) << o in one v_bfm_b32 (clang emits a shift, a not and a shift)
__device__ __forceinline__ uint32_t bfm(uint32_t w, uint32_t o) {
    uint32_t r;
    asm("v_bfm_b32 %0, %1, %2" : "=v"(r) : "v"(w), "v"(o));
    return r;
}
__device__ __forceinline__ void run_up(uint32_t occ, uint32_t c, uint32_t& t, uint32_t& m) {
    t = (uint32_t)__builtin_ctz((occ | 16u) >> c);
    m = bfm(t, c);
}
__device__ __forceinline__ void run_down(uint32_t occ, uint32_t c, uint32_t& t, uint32_t& m) {
    // slots below c at bits 1..c, the sentinel at bit 0: the highest set bit is the run's first slot
    const uint32_t lo = 31u - (uint32_t)__builtin_clz(__builtin_amdgcn_ubfe((occ << 1) | 1u, 0u, c + 1u));
    t = c + 1u - lo;
    m = bfm(t, lo);
}
__device__ __forceinline__ void run_fwd(uint32_t occ, uint32_t c, bool pos, uint32_t ud, uint32_t& t, uint32_t& m) {
    if (ud == 1u) {
        run_up(occ, c, t, m);
    } else if (ud == 2u) {
        run_down(occ, c, t, m);
    } else {
        uint32_t t0, m0, t1, m1;
        run_up(occ, c, t0, m0);
        run_down(occ, c, t1, m1);
        t = pos ? t0 : t1;
        m = pos ? m0 : m1;
    }
}

// per 16-bit half of v: 1 if it is nonzero — one packed min (clang scalarises the vector form)
__device__ __forceinline__ uint32_t nonzero16(uint32_t v) {
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(v), "s"(0x00010001u));
    return r;
}

// Grow the ray's empty child slot into a forward box of empty sibling slots (greedy: the run along x
// from the mask row, then whole rows along z; one cell in y), all from the parent's 64-bit child
// mask in registers, without loops.  Returns per-axis steps to leave it, less one (the index of the
// step that leaves).
__device__ __forceinline__ void box_exits(const uint32_t w[3], const int32_t s[3], uint32_t sh, uint64_t pmask, const uint32_t ud[3],
                                          int32_t e[3]) {
    const uint32_t cx = __builtin_amdgcn_ubfe(w[0], sh, 2u), cy = __builtin_amdgcn_ubfe(w[1], sh, 2u), cz = __builtin_amdgcn_ubfe(w[2], sh, 2u);
    const bool px = s[0] > 0, py = s[1] > 0, pz = s[2] > 0;
    const uint32_t lo = (uint32_t)pmask, hi = (uint32_t)(pmask >> 32);
    uint32_t tx, xm, tz, zm;
    // x run through the row (cy, cz)
    run_fwd((uint32_t)(pmask >> (16u * cz + 4u * cy)), cx, px, ud[0], tx, xm);
    // rows (cy, z) over the x run: bit z (bits 0, 16 -> 0, 1 of the low half, 2, 3 of the high) =
    // the row holds a solid slot
    const uint32_t xs = xm << (4u * cy);
    const uint32_t xl = xs | (xs << 16);
    const uint32_t zc = nonzero16(lo & xl) | (nonzero16(hi & xl) << 2);
    run_fwd(zc | (zc >> 15), cz, pz, ud[2], tz, zm);
    (void)zm;
    // (growing the box along y as well — whole planes over the x run x z run — cost more per crossing
    // than it saved in crossings: without it C3 2.7 %, C5 3.7 %, C2 0.5-2.7 % faster; x runs alone
    // were 16 % slower at C3 / C5)
    const uint32_t ty = 1u;
    // steps to leave: t cells of 2^sh voxels, less the part of the current cell behind the ray;
    // less one: x + ~y = x - y - 1
    const uint32_t m = (1u << sh) - 1u;
    e[0] = (int32_t)((tx << sh) + ~((px ? w[0] : ~w[0]) & m));
    e[1] = (int32_t)((ty << sh) + ~((py ? w[1] : ~w[1]) & m));
    e[2] = (int32_t)((tz << sh) + ~((pz ? w[2] : ~w[2]) & m));
}

// The child mask shifted so that slot sl's bit lands on bit 63 (m << (63 - sl)): its sign is the
// occupancy, and one more shift leaves exactly the lower slots' bits, whose popcount is the
// child's rank among its siblings.
__device__ __forceinline__ uint64_t slot_top(uint64_t m, uint32_t sl) { return m << (sl ^ 63u); }
// popcount(x) + acc through the accumulating v_bcnt_u32_b32 (clang adds acc separately)
__device__ __forceinline__ uint32_t popc_add(uint64_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"((uint32_t)x), "v"(acc));
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"((uint32_t)(x >> 32)), "v"(r));
    return r;
}
