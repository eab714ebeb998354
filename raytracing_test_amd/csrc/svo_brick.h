// svo_brick.h — the voxel steps through one 4^3 brick on its mask in registers (brick_walk).  Used by trace() in
// svo_trace.h, for bricks and for the empty regions of rays outside the closed forms' domain.
#pragma once

#include "svo_exact.h"
#include "svo_stats.h"

// Voxel steps through a brick on its register mask (see trace): returns the voxel index reached;
// `left` = per-axis steps left in the brick (bytes 0-2, a zero byte = left the brick), `solid` =
// stopped on a solid voxel.  The crossing value of every step is kept (recovering it after the
// walk as T - a, exact for fast rays, measured no faster).
// TRACK: keep the crossing value of every step (R.tlast); without it trace recovers the last one
// once, at the end of the ray (exact sums: T - a).  (A wave-uniform runtime flag in this loop
// measured 1.6 % slower than tracking always.)
// (Skipping the per-step budget test for waves with budget for a whole walk, at most 10 steps,
// measured equal.)
template <bool STATS, bool TRACK>
__device__ __forceinline__ uint32_t brick_walk(Ray& R, uint64_t bmask, const uint32_t w[3], uint32_t left0, uint32_t& left, bool& solid,
                                               Stats& st) {
    // 127 - voxel index (byte 0: the 64-bit shift reads its low 6 bits, 63 - v, which moves the
    // voxel's bit to bit 63 — one shift and a sign test; the +-1/4/16 moves of a walk stay within
    // 48..143, so byte 0 never borrows) and steps left (bytes 1-3, biased: 0x80 + left - 1, so a
    // byte leaves the brick by clearing its top bit, without a borrow) in one register.  The step
    // keeps its delta instead of the axis: the axis follows from the last delta after the walk.
    uint32_t pk = (left0 << 8) | (127u - child_slot(w[0], w[1], w[2], 0u));
    const uint32_t d0 = (uint32_t)(-R.s[0]) - 0x100u, d1 = (uint32_t)(-R.s[1] * 4) - 0x10000u, d2 = (uint32_t)(-R.s[2] * 16) - 0x1000000u;
    uint32_t dl = 0u;
    bool go;
    do {  // one exit: the compiler keeps the state in place (no per-exit copies)
        solid = (int64_t)(bmask << (pk & 63u)) < 0;
        go = !solid && R.steps > 0;
        if (go) {
            // one DDA step (ray_caster.cpp:70-80) without position updates
            const bool cx = (R.T[0] < R.T[1]) && (R.T[0] < R.T[2]);
            const bool cy = !cx && (R.T[1] < R.T[2]);
            if (TRACK) R.tlast = cx ? R.T[0] : (cy ? R.T[1] : R.T[2]);
            R.T[0] = cx ? R.T[0] + R.a(0) : R.T[0];
            R.T[1] = cy ? R.T[1] + R.a(1) : R.T[1];
            R.T[2] = (cx || cy) ? R.T[2] : R.T[2] + R.a(2);  // (a mask or, not a fourth f64 compare)
            R.steps--;
            dl = cx ? d0 : (cy ? d1 : d2);
            pk += dl;
            if (STATS) {
                st.brick_steps++;
                st.wv_brick += wave_lead();
            }
            go = (pk & 0x80808000u) == 0x80808000u;  // every steps-left byte above its bias: inside
        }
    } while (go);
    if (dl != 0u) R.axis = dl == d0 ? 0u : (dl == d1 ? 1u : 2u);
    left = pk >> 8;
    return 63u - (pk & 63u);
}
