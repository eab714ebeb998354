// svo_ceil_march.h — the column-ceiling march before the loop: the descent of a linear ray through the air above the
// terrain, block by block on exact event values, ended by one crossing (ceil_march).  Used by trace() in svo_trace.h,
// which hands its exits to skip_box (svo_skip.h).
#pragma once

#include "svo_exact.h"
#include "svo_skip.h"
#include "svo_stats.h"

// the fine phase's bound, in 4-column blocks: the whole wave walks as far as its longest lane, so a ray gliding over a plain
// must hand over to the loop's boxes (C3, interleaved on one box: 8 blocks 0.1368 ms, 24 0.1308, 64 0.1344)
constexpr int32_t kMarchFineMax = 24;
// ... and the budget it wants left beyond the first phase's end: its blocks span up to 8 x / z steps each.  A march whose end
// lies beyond the budget moves nothing (skip_box refuses it), so a ray with less left keeps the first phase's end
constexpr int32_t kMarchFineSpan = 8 * kMarchFineMax;
// A coarse level (256- or 64-column blocks) is walked only by launches whose budget spans at least this many of its blocks:
// a level passes no more blocks than the budget has x / z steps for, each pass saves at most three trips of the next
// level, and entering a level costs a loop's set-up, the trip that fails and a descent whatever it passes — about what
// two passes save.  C2 (budget 300) ran 3.5 % slower with both levels on whatever its budget, its range wholly above the
// parent's; AO rays are shorter still.  At 8 blocks a budget below 512 steps marches as it did (16-column
// blocks first), one below 2048 from 64 columns
constexpr int32_t kMarchCoarseSpan = 8;

// Column-ceiling march (round 5).  A descending ray above the ceiling of its 16-column block crosses, cell by cell,
// only empty voxels until its row reaches that ceiling or it leaves the block; castRayFromCam's DDA (ray_caster.cpp:71-80)
// takes its x / z / y steps at the crossing values T_k + j * a_k, so every event that matters here is one fma of an
// integer index: the x (z) event entering the next block, j = the cells left in the block on that axis, and the y event
// entering the ceiling row c, j = y - 1 - c.  The march walks the blocks the ray's column path crosses (their order
// follows from the x / z boundary events alone) comparing exact event values, one ceiling load per block (the
// next block's load issued before this one is judged), until the ceiling event comes first or the ray enters a block
// at or below its ceiling; every voxel entered before that event is then empty, and one closed-form crossing
// (skip_box) moves the ray to the state right after it — the cell that event enters is the loop's next untested
// voxel.  This replaces the chain of per-block ceiling moves of a ray's descent (C3: ~6 of its ~11 loop iterations,
// each a full iteration with its own exact crossing) by one crossing and a few integer / fma steps per block.
// Linear rays only (every sum exact: `fast` in the non-segment instances), stepping down (R.s[1] < 0); a tie between
// the x and z boundary events (a block corner) or between a boundary and the ceiling event stops the march there.

// The march's state between blocks of one level: per axis the index (from the ray's state) and value of the event that
// leaves the current block (bx, bz); the event that entered it (Ein: -inf, axis -1 for the block the ray starts in); and,
// once a block fails, the first event whose voxel is not proven empty (stop_axis -1: the ray's own voxel)
struct March {
    int32_t jx, jz;
    double Ex, Ez;
    uint32_t bx, bz;
    double Ein;
    int32_t ein_axis, ein_j, stop_axis, stop_j;
    int32_t jy;  // the index of the y event entering the ceiling row of the block that failed (negative: the ray entered below it)
};

// An upper estimate of the DDA steps up to the march's end: no more x (z) events than the failed block's exit index, no
// more y events than down to its ceiling row (from below it: the rows down to 0).  Only what the march does with its
// budget rests on it, never a result.
__device__ __forceinline__ int32_t march_reach(const March& m, int32_t wy) { return m.jx + m.jz + 2 + (m.jy >= 0 ? m.jy : wy) + 1; }

// The blocks of one level, 2^lsh columns wide, `rows` of them per row of the table ceil(index) reads, until one fails or
// `bound` blocks are proven.  Returns the blocks passed.
template <class Ceil>
__device__ __forceinline__ int32_t march_level(const Ray& R, int32_t wy, uint32_t lsh, uint32_t rows, int32_t bound, const Ceil& ceil, March& m) {
    const uint32_t bm = (1u << lsh) - 1u, rm = rows - 1u;
    const uint32_t dx = R.s[0] > 0 ? 1u : rm, dz = R.s[2] > 0 ? 1u : rm;  // (one block on, wrapped)
    int32_t jx = m.jx, jz = m.jz, ein_axis = m.ein_axis, ein_j = m.ein_j, stop_axis = -1, stop_j = 0;
    double Ex = m.Ex, Ez = m.Ez, Ein = m.Ein;
    uint32_t bx = m.bx, bz = m.bz;
    int32_t cv = ceil(__umul24(bz, rows) + bx), jy = 0, it = 0;
    for (;; it++) {
        const bool xn = Ex < Ez;
        // the next block's ceiling, loaded before this block is judged (the blocks' order follows from x / z alone)
        const uint32_t nbx = xn ? (bx + dx) & rm : bx, nbz = xn ? bz : (bz + dz) & rm;
        const int32_t ncv = ceil(__umul24(nbz, rows) + nbx);
        jy = wy - 1 - cv;  // the y event entering the ceiling row
        const double tc = jy >= 0 ? on_grid(R.T[1], jy, R.a(1)) : -__builtin_inf();
        if (!(tc > Ein) || it == bound) {  // the voxel entering this block is at or below its ceiling: end before that event
            stop_axis = ein_axis;        // (and a bound on the march: its blocks so far are proven)
            stop_j = ein_j;
            break;
        }
        const double Eexit = xn ? Ex : Ez;
        // the next boundary lies beyond the budget: only the ceiling event can come first within it
        const bool far = (xn ? jx : jz) > R.steps;
        if (!(Eexit < tc) || Ex == Ez || far) {
            if (far || (!(Ez <= tc && Ez <= Ex) && tc <= Ex)) {  // the first unproven event, in the DDA's order at ties: z, y, x
                stop_axis = 1;
                stop_j = jy;
            } else if (Ez <= tc && Ez <= Ex) {
                stop_axis = 2;
                stop_j = jz;
            } else {
                stop_axis = 0;
                stop_j = jx;
            }
            break;
        }
        Ein = Eexit;  // on into the next block
        if (xn) {
            ein_axis = 0;
            ein_j = jx;
            jx += (int32_t)bm + 1;
            Ex = on_grid(R.T[0], jx, R.a(0));
        } else {
            ein_axis = 2;
            ein_j = jz;
            jz += (int32_t)bm + 1;
            Ez = on_grid(R.T[2], jz, R.a(2));
        }
        bx = nbx;
        bz = nbz;
        cv = ncv;
    }
    m = March{jx, jz, Ex, Ez, bx, bz, Ein, ein_axis, ein_j, stop_axis, stop_j, jy};
    return it;
}

// The descent between two levels, from the block that failed onto the blocks 2^csh columns wide, a quarter of its width: the
// march goes on from the event that entered the failed block, in the sub-block that event left the ray in.  That follows from
// the cells the ray has left in the block on each axis: on the axis it entered by, all of them; on the other, the exit index
// less the events of that axis that precede the entering event in the DDA's order (z before x at equal values: entered in z,
// the x events strictly below it; in x, the z events at or below it; the block the ray starts in: none), counted exactly
// (count_est and its settling compare, as skip_box counts them).  The entering event stays what it was.
__device__ __forceinline__ void march_descend(const Ray& R, uint32_t csh, March& m) {
    const bool ez = m.ein_axis == 2;
    double F;
    int32_t n = count_est(ez ? R.T[0] : R.T[2], ez ? R.a(0) : R.a(2), ez ? R.inv_a(0) : R.inv_a(2), m.Ein, (float)m.Ein, F);
    n += (ez ? F < m.Ein : F <= m.Ein) ? 1 : 0;
    const int32_t kx = m.ein_axis == 0 ? m.ein_j + 1 : (ez ? n : 0), kz = ez ? m.ein_j + 1 : (m.ein_axis == 0 ? n : 0);
    const uint32_t lx = ((uint32_t)(m.jx - kx) >> csh) & 3u, lz = ((uint32_t)(m.jz - kz) >> csh) & 3u;  // sub-blocks left after it
    m.jx -= (int32_t)(lx << csh);
    m.jz -= (int32_t)(lz << csh);
    m.Ex = on_grid(R.T[0], m.jx, R.a(0));
    m.Ez = on_grid(R.T[2], m.jz, R.a(2));
    m.bx = (m.bx << 2) + (R.s[0] > 0 ? 3u - lx : lx);
    m.bz = (m.bz << 2) + (R.s[2] > 0 ? 3u - lz : lz);
}

// The march: one loop per level, coarse to fine, never back.  It starts on the coarsest level the launch gives it
// (P.march_sh: 256- and 64-column blocks of P.ceil, where the tree has them and the budget spans kMarchCoarseSpan of them),
// goes on over the 16-column blocks of the launch's first ceiling level (ceilp: its pairs), then — fine descent — over
// 4-column blocks on the tree's fine ceilings (ceilf: svo_tree.d_ceilf, int16 row-major; null: none).  A coarse block's
// ceiling is the maximum over all its columns, far above most of them on terrain, so a level ends long before the ray
// meets anything: it enters a block at or below its ceiling, or that block's ceiling event comes before its exit.  The
// next level takes the march on from the event that entered that block (march_descend), judging its blocks the same way,
// through as many of the coarser blocks as it takes.  High above the terrain a 256-column block passes where sixteen
// 16-column blocks in a row did.
// The coarse levels only place the 16-column phase: every end they prove, the 16-column phase proves too, so the ends kept
// are that phase's and the last one's.  The last phase runs for at most kMarchFineMax blocks (what it has proven by then
// stands; the loop's ceiling boxes carry on), and only for rays with kMarchFineSpan steps of budget to spare beyond the
// 16-column phase's end.  One loop per level, not one over blocks of any size: a wave runs each until its last lane is
// done, and a loop that holds several levels issues every level's code for every block.  The coarse levels share one
// loop's code (their shift and table are scalars of the launch).
// The march's end: ex (skip_box's exits) of the first event whose voxel it could not prove empty.  Returns false when
// nothing beyond the current voxel is proven (its own row is at or below its block's ceiling).
template <bool STATS>
__device__ __forceinline__ bool ceil_march(const CastParams& P, const uint32_t* __restrict__ ceilp, const int16_t* __restrict__ ceilf,
                                           const Ray& R, uint32_t wm, int32_t ex[3], Stats& st) {
    const uint32_t lsh = P.ceil_sh[0];  // the launch's first level: blocks 2^lsh columns wide
    // the coarse levels this budget spans (the first lane's: a launch's rays share their budget, and the levels walked
    // change the trips only, never the end)
    const int32_t nc = P.march_n, ub = __builtin_amdgcn_readfirstlane(R.steps);
    int32_t l0 = 0;
    if (l0 < nc && (ub >> P.march_sh[0]) < kMarchCoarseSpan) l0 = 1;
    if (l0 == 1 && l0 < nc && (ub >> P.march_sh[1]) < kMarchCoarseSpan) l0 = 2;
    const uint32_t sh0 = l0 >= nc ? lsh : (l0 == 0 ? P.march_sh[0] : P.march_sh[1]), bm = (1u << sh0) - 1u;
    const int32_t wy = (int32_t)((uint32_t)R.r[1] & wm);
    const uint32_t wx = (uint32_t)R.r[0] & wm, wz = (uint32_t)R.r[2] & wm;
    // per axis the next block-boundary event: its index from the current state (the cells left in the block) and value
    March m;
    m.jx = (int32_t)(R.s[0] > 0 ? bm - (wx & bm) : (wx & bm));
    m.jz = (int32_t)(R.s[2] > 0 ? bm - (wz & bm) : (wz & bm));
    m.Ex = on_grid(R.T[0], m.jx, R.a(0));
    m.Ez = on_grid(R.T[2], m.jz, R.a(2));
    m.bx = wx >> sh0;
    m.bz = wz >> sh0;
    m.Ein = -__builtin_inf();
    m.ein_axis = -1;
    m.ein_j = 0;
#pragma nounroll
    for (int32_t l = l0; l < nc; l++) {  // (selects, not indices: the launch's parameters stay scalar)
        const uint32_t sh = l == 0 ? P.march_sh[0] : P.march_sh[1];
        const int16_t* __restrict__ const tab = P.ceil + (l == 0 ? P.march_off[0] : P.march_off[1]);
        const int32_t n = march_level(R, wy, sh, (wm + 1u) >> sh, 1024, [&](uint32_t i) { return (int32_t)tab[i]; }, m);
        if (STATS) {
            if (sh == lsh + 2u) st.march_64 += (uint32_t)n;
            else st.march_256 += (uint32_t)n;
        }
        march_descend(R, sh - 2u, m);
    }
    const int32_t n16 = march_level(R, wy, lsh, (wm + 1u) >> lsh, 1024, [&](uint32_t i) { return (int32_t)(int16_t)(ceilp[i] & 0xFFFFu); }, m);
    if (STATS) st.ceil_moves += (uint32_t)n16;
    const int32_t c_axis = m.stop_axis, c_j = m.stop_j;
    if (ceilf && R.steps - march_reach(m, wy) >= kMarchFineSpan) {  // (ceilf: uniform)
        march_descend(R, lsh - 2u, m);
        if (STATS) st.march_descents++;
        const int32_t n4 = march_level(R, wy, lsh - 2u, (wm + 1u) >> (lsh - 2u), kMarchFineMax, [&](uint32_t i) { return (int32_t)ceilf[i]; }, m);
        if (STATS) st.march_fine += (uint32_t)n4;
        if (march_reach(m, wy) > R.steps) {  // its end may lie beyond the budget: the 16-column phase's stands
            m.stop_axis = c_axis;
            m.stop_j = c_j;
        }
    }
    // (selects on values: a dynamically indexed register array would go through scratch)
    ex[0] = m.stop_axis == 0 ? m.stop_j : R.steps;
    ex[1] = m.stop_axis == 1 ? m.stop_j : R.steps;
    ex[2] = m.stop_axis == 2 ? m.stop_j : R.steps;
    return m.stop_axis >= 0;
}
