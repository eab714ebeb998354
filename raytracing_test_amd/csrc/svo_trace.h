// svo_trace.h — one ray: the trace<OPT> option word and trace() itself (the semantics are in svo_cast_kernel.h's header
// note).  The one header svo_shade.h includes.  The rest of a ray's device code is in the eight headers below, one concern
// each, included in the order of their definitions (the map of the traversal code):
#pragma once

#include <algorithm>

#include "svo_cast_params.h"

#include "svo_exact.h"       // the note on exact closed-form skipping, the tests for the rays it covers, Ray, dda_step
#include "svo_boxes.h"       // forward boxes of empty sibling slots, from the parent's child mask
#include "svo_skip.h"        // the closed-form crossing of an empty box (skip_box), its counts and exact segments
#include "svo_stats.h"       // the diagnostics counters and the slots of their buffer (S_*)
#include "svo_lookup.h"      // the parent in registers, the LDS path, node addressing, the region lookup
#include "svo_brick.h"       // the brick walk
#include "svo_ceil_march.h"  // the column-ceiling march before the loop
#include "svo_bounce.h"      // the shading pass's bounce state and refraction

__host__ __device__ constexpr int32_t dirs_sign(int DIRS, int k) { return DIRS == 0 ? 0 : (((DIRS - 1) >> k) & 1) ? -1 : 1; }

// trace()'s compile-time options: one word, trace<OPT>, or-ed from the names below.  Inside trace() each is a constant
// of the name without its prefix (STATS, REFLECT, ...).
enum : uint32_t {
    T_PLAIN = 0u,       // none of them (the AO rays)
    T_STATS = 1u << 0,  // diagnostics: the traversal counters (Stats), added to P.stats when the ray ends; *ray_work
    // the shading pass's reflections and refractions, applied where the ray meets such a block (*bounce); the steps'
    // signs may change on the way
    T_REFLECT = 1u << 1,
    // (shading rays whose end position is not output): a ray moving up above the highest stored voxel row `top`
    // (wrapped) whose budget cannot carry it past the extent in y leaves the loop as a miss at once — it can only enter
    // empty space — and skips its remaining steps (top < 0: off); so does a ray whose budget ends inside an empty box;
    // and with column ceilings, a ray above `top` crosses the whole half-space above it (every x and z) in one move.
    T_ESCAPE = 1u << 2,
    T_SEG = 1u << 3,  // segment-bounded crossings, for rays that may not be linear (need_seg; see `lin` below)
    // (AO) of the parent that par_out receives only the shift is exact (lookup: L_PSH) — a ray ending in a SOLID region
    // above the bricks leaves that region's mask and ref
    T_KEEPPAR = 1u << 4,
    // no crossing value is output (shading launches without hit records), so none is tracked per step.
    T_NO_T = 1u << 5,
    // The column ceilings the ray checks, at most one of:
    T_CEIL_NONE = 0u,
    T_CEIL_PAIRS = 1u << 6,   // the launch's two levels of the column ceilings (P.ceilp pairs)
    T_CEIL_QUADS = 1u << 7,   // every level, the coarsest block the ray is above (P.ceilq: a max-mipmap walk of the ceilings)
    T_CEIL_SHADOW = 1u << 8,  // as pairs, on those of the solid-view tree of a shading launch, P.sceilp — the shadow rays
    T_CEIL_ANY = T_CEIL_PAIRS | T_CEIL_QUADS | T_CEIL_SHADOW,
    // (the shading pass) the straight trace of a shading ray hands its first hit on to the bouncing one, at most one of:
    T_XS_NONE = 0u,
    T_XS_SAVE = 1u << 9,  // on a hit, store the DDA state the ray entered its block with in *xs (RayState)
    // start from *xs instead of the origin's first step (the flags fast / lin still from the origin and direction), with
    // no pre-top box and no march
    T_XS_RESUME = 1u << 10,
    T_XS_ANY = T_XS_SAVE | T_XS_RESUME,
    // t_dirs(1..8): every ray of the launch steps with the signs dirs_sign(DIRS, k) (frame_dirs proves it on the host):
    // the steps are compile-time constants and the sign branches of the crossings and brick walks fold away; 0:
    // per-wave sign flags (dir_flags)
    T_DIRS_SHIFT = 11u,
    T_DIRS_ANY = 15u << T_DIRS_SHIFT,
};
__host__ __device__ constexpr uint32_t t_dirs(int dirs) { return (uint32_t)dirs << T_DIRS_SHIFT; }
__host__ __device__ constexpr uint32_t t_if(bool on, uint32_t opt) { return on ? opt : 0u; }  // an option an instance's flag decides

// One ray with castRayFromCam semantics.  par_out: receives the parent of the region the ray ended in (it holds the
// final voxel; the LDS path holds its ancestors at depths 0 .. levels-1-sh/2).
template <uint32_t OPT, class Mem>
__device__ __forceinline__ Hit trace(const CastParams& P, const Mem& mem, const uint16_t* mats, const Path& path, const float o[3],
                                     const float d[3], int32_t budget, unsigned long long* ray_work = nullptr,
                                     Bounce* bounce = nullptr, Parent* par_out = nullptr, int32_t top = -1, int32_t pre_top = -1,
                                     const FrameAxes* fx = nullptr, RayState* xs = nullptr) {
    constexpr bool STATS = (OPT & T_STATS) != 0u, REFLECT = (OPT & T_REFLECT) != 0u, ESCAPE = (OPT & T_ESCAPE) != 0u;
    constexpr bool SEG = (OPT & T_SEG) != 0u, KEEPPAR = (OPT & T_KEEPPAR) != 0u, NO_T = (OPT & T_NO_T) != 0u;
    constexpr int DIRS = (int)((OPT & T_DIRS_ANY) >> T_DIRS_SHIFT);
    constexpr uint32_t CEIL = OPT & T_CEIL_ANY, XS = OPT & T_XS_ANY;
    static_assert((CEIL & (CEIL - 1u)) == 0u, "trace: the T_CEIL_ options exclude each other");
    static_assert((XS & (XS - 1u)) == 0u, "trace: T_XS_SAVE and T_XS_RESUME exclude each other");
    static_assert(DIRS <= 8 && (OPT >> (T_DIRS_SHIFT + 4u)) == 0u, "trace: DIRS is 0..8; no other option bits");
    Ray R;
    if (DIRS != 0 && fx) {
        // a frame ray of an octant instance: the origin's part of dda_axis is the frame's (fx)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float df = rcp_rn(d[k]);
            const double delta = (double)df;
            R.r[k] = fx->cell[k];
            R.T[k] = __builtin_fma(-fx->frac[k], delta, __builtin_fabs(delta));
            R.af[k] = __builtin_fabsf(df);
            R.s[k] = dirs_sign(DIRS, k);
            R.ia[k] = __builtin_amdgcn_rcpf(R.af[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const Dda1 ax = dda_axis(o[k], d[k]);
            R.r[k] = ax.cell;
            R.T[k] = ax.dpos;
            R.af[k] = (float)ax.adelta;  // exact: adelta is |f32 quotient|
            R.s[k] = ax.step;
            R.ia[k] = __builtin_amdgcn_rcpf((float)ax.adelta);
        }
    }
    R.steps = budget;
    R.axis = 3u;
    R.tlast = 0.0;
    // closed-form crossings (fast): budget < 2^20 also keeps the f32 count estimates within 3/8 of
    // the truth (count_est, seg_cap); linear rays need no segment bounds, and a wave of linear rays
    // takes the cheaper crossing.  Origins within 2^30 (an exact start cell: deltaPos starts in
    // [0, 2 absDelta]); beyond them castRayFromCam's int conversion is undefined, and those rays step
    // voxel by voxel (no closed form over a start cell the conversion clamped)
    // (bitwise ands: one straight-line computation, no branch per term)
    bool fast = ((unsigned)!(P.flags & SVO_CAST_ITERATIVE) & (unsigned)(budget < (1 << 20)) & (unsigned)axis_ok(R.T[0], R.a(0)) &
                 (unsigned)axis_ok(R.T[1], R.a(1)) & (unsigned)axis_ok(R.T[2], R.a(2)) & (unsigned)((DIRS != 0 && fx) || span_ok(R)) &  // (frame rays: unit directions)
                 (unsigned)(!SEG || (__builtin_fabsf(o[0]) < 0x1p30f && __builtin_fabsf(o[1]) < 0x1p30f &&
                                     __builtin_fabsf(o[2]) < 0x1p30f))) != 0u;  // (!SEG: need_seg bounds the origins)
    // SEG: the instance carries segment-bounded crossings (the host picks it when rays can be
    // non-linear: need_seg).  The other one runs exact-origin rays only; it re-tests them cheaply
    // (lin_origin) and steps any other ray voxel by voxel.
    bool lin = SEG ? fast && exact_axis(R.T[0], R.a(0), budget) && exact_axis(R.T[1], R.a(1), budget) && exact_axis(R.T[2], R.a(2), budget)
                   : (DIRS != 0 && fx) ? fast  // (need_seg: this instance's frame origins are exact)
                   : ((unsigned)fast & (unsigned)lin_origin(o[0]) & (unsigned)lin_origin(o[1]) & (unsigned)lin_origin(o[2])) != 0u;
    if (!SEG) fast = lin;
    const bool wseg = SEG && __ballot(fast && !lin) != 0ull;  // wave-uniform (REFLECT: taken per crossing)
    // octant segment instances cache their segment bounds (skip_box RB); none yet (cap -1)
    constexpr bool RB = SEG && DIRS != 0 && !REFLECT;
    if (RB) {
#pragma unroll
        for (int k = 0; k < 3; k++) R.rb[k] = R.r[k] - R.s[k];
    }
    // Instances without segments run rays from integral / half-integral origins only (need_seg):
    // every sum they take is exact, so they recover the output crossing value once at the end
    // (T - a on the last step's axis) instead of keeping it on every brick step
    // (NO_T: no crossing value is output — shading launches without hit records — so none is kept)
    constexpr bool TRACK = (REFLECT || SEG) && !NO_T;
    constexpr uint32_t LOOK = t_if(STATS, L_STATS) | t_if(!REFLECT, L_SPLIT) | t_if(KEEPPAR, L_PSH);  // the region lookups' options
    uint32_t ud[3];
    if (DIRS != 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            R.s[k] = dirs_sign(DIRS, k);  // (equal to dda_axis' step: frame_dirs)
            ud[k] = dirs_sign(DIRS, k) > 0 ? 1u : 2u;
        }
    } else {
        dir_flags(R.s, ud);
    }
    // the hit is mat != kNoHit (a flag of its own costs lane-mask upkeep every iteration)
    uint32_t mat = kNoHit;
    const uint32_t wm = P.wmask;
    Stats st = {};
    Parent par;
    // the root (node 0 of the tree this trace walks; uniform, one scalar load) is the first parent and stands in the
    // per-lane path at depth 0, so the first lookup starts at the root's child slot instead of loading the root (one
    // dependent load fewer per ray; every later restart at depth 0 reads the same node from the path: C3 -0.8 %, C4
    // -0.6 %, C5 -1.1 %, shaded -0.5 %, profiles/r06/ab_root_seed_*.txt).  A root that is not interior (a one-level
    // tree, a uniform world) keeps the virtual parent above it.
    const Node rn = mem.root();
    if (P.levels >= 2 && (rn.info & K_KIND_MASK) == K_INTERIOR) {  // (uniform)
        path.put(0, rn.mask, rn.ref);
        par.mask = rn.mask;
        par.ref = rn.ref;
        par.sh = 2u * (uint32_t)(P.levels - 1);
    } else {
        // a virtual parent above the root (its one child region, slot 0 of the wrapped coordinates, is
        // the whole world = node 0): the first lookup takes the same path as every later one
        par.mask = 1ull;
        par.ref = 0u;
        par.sh = 2u * (uint32_t)P.levels;
    }
    // T_XS_RESUME: resume a ray from the state its straight trace (T_XS_SAVE) stopped in — the cell it entered, untested;
    // the flags above (fast, lin: from the origin and direction) are the ones that trace had
    bool done = R.steps <= 0;
    if (XS == T_XS_RESUME) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            R.T[k] = xs->T[k];
            R.r[k] = xs->r[k];
        }
        R.steps = xs->steps;
        R.axis = xs->axis;
        done = false;
    } else if (!done) {
        dda_step(R);
    }
    // pre_top (>= 0: the tree's highest stored voxel row, tree_top_y): a ray starting above it is in
    // one empty region {y > pre_top} (every x, z; up to the wrap in y) and crosses it in one move,
    // exactly like a box (false: its budget ends up there, state unchanged, the loop walks it)
    if (XS != T_XS_RESUME && pre_top >= 0 && fast && !done) {
        uint32_t w[3];
        wrap3(R, wm, w);
        if ((int32_t)w[1] > pre_top) {
            const int32_t ex[3] = {R.steps, R.s[1] < 0 ? (int32_t)w[1] - pre_top - 1 : (int32_t)(wm - w[1]), R.steps};
            skip_box<TRACK, RB>(R, ex, wseg);
        }
    }
    // one back-edge: every path through the body ends at the loop latch
    bool escaped = false;
    uint32_t bref = 0u, binfo = 0u;
    uint64_t bmask = 0ull;
    // coordinate bits changed since the last voxel known to lie in the parent's region, by ceiling moves since
    // the last lookup and the step before them (the lookup's restart depth)
    uint32_t jump = 0u;
    const bool ceil_on = CEIL != T_CEIL_NONE && (CEIL == T_CEIL_SHADOW ? P.sceil_levels : P.ceil_levels) > 0;  // (uniform)
    const uint32_t* const ceilp = CEIL == T_CEIL_SHADOW ? P.sceilp : P.ceilp;
    uint32_t ckey = 0xFFFFFFFFu, cval = 0u;  // the lane's 16-column block (key) and its ceilings (c0 | c1 << 16)
    uint64_t cq = 0ull;                      // (T_CEIL_QUADS: the ceilings of the blocks of every level holding the lane's 16-column block)
    // the descent through the air above the terrain in one march (ceil_march): linear primary / AO rays stepping down
    // (the voxel it ends in is untested, even when the budget ends with it: the loop tests it)
    // (primary / AO casts, and the shading pass's rays before any bounce; exact-sum lanes only: `lin` in segment instances)
    constexpr bool MARCH = CEIL == T_CEIL_PAIRS || CEIL == T_CEIL_QUADS;
    if (XS != T_XS_RESUME && MARCH && ceil_on && !done && (SEG ? lin : fast) && R.s[1] < 0 && R.steps > 0) {
        int32_t ex[3];
        if (ceil_march<STATS>(P, ceilp, P.ceilf, R, wm, ex, st)) (void)skip_box<TRACK, RB>(R, ex, wseg);
    }
    while (!done) {
        // the voxel just entered is untested
        if (STATS) {
            st.wv_iters += wave_lead();
            st.iters++;
        }
        const int32_t steps_in = R.steps;  // (the progress guard below)
        uint32_t w[3];
        wrap3(R, wm, w);
        if (STATS && pre_top >= 0 && (int32_t)w[1] > pre_top) st.above_top++;
        if (ESCAPE && top >= 0 && R.s[1] > 0 && (int32_t)w[1] > top && (int64_t)w[1] + R.steps <= (int64_t)wm) {
            escaped = true;  // only empty voxels ahead: a miss
            break;
        }
        uint32_t sh = 0u;
        bool pend = false;  // the lookup found a brick: step through it below
        const uint32_t ax = R.axis;
        const uint32_t wa = ax == 0u ? w[0] : (ax == 1u ? w[1] : w[2]);
        const int32_t sa = ax == 0u ? R.s[0] : (ax == 1u ? R.s[1] : R.s[2]);
        const uint32_t moved = jump | (wa ^ ((wa - (uint32_t)sa) & wm));  // bits the last step(s) changed
        // Column ceilings: a ray above the highest stored row of the 256- (then 64-) column block it is in
        // has only empty voxels between it and that row, and above it up to the top of the world, over the
        // whole block: that box is crossed without a lookup (R_CEIL; the next lookup restarts from the
        // per-lane path at the depth the moves since the last lookup left intact)
        int32_t cex[3] = {0, 0, 0};
        bool cl = false, any_cl = false, gt = false;
        int32_t c0 = -1, c1 = 32767;  // the ceilings of the lane's blocks at the launch's two levels (set_ceilings)
        uint32_t lv = 0u;             // (T_CEIL_QUADS) how many levels' ceilings the ray is above: its box is a block of level lv - 1
        if (CEIL == T_CEIL_QUADS && ceil_on && fast && R.steps > 0) {
            const int32_t y = (int32_t)w[1];
            constexpr uint32_t lsh0 = 2u * kCeilK0;
            const uint32_t rows0 = (wm + 1u) >> lsh0;
            const uint32_t key = __umul24(w[2] >> lsh0, rows0) + (w[0] >> lsh0);
            if (key != ckey) {
                ckey = key;
                cq = P.ceilq[key];
            }
            // (the ceilings grow with the level: a block's holds its children's)
            lv = (uint32_t)(y > (int32_t)(int16_t)cq) + (uint32_t)(y > (int32_t)(int16_t)(cq >> 16)) +
                 (uint32_t)(y > (int32_t)(int16_t)(cq >> 32)) + (uint32_t)(y > (int32_t)(int16_t)(cq >> 48));
            cl = lv != 0u;
            if (ESCAPE) gt = top >= 0 && y > top;
        } else if (ceil_on && fast && R.steps > 0) {
            const int32_t y = (int32_t)w[1];
            const uint32_t lsh0 = P.ceil_sh[0], rows0 = (wm + 1u) >> lsh0;
            const uint32_t key = __umul24(w[2] >> lsh0, rows0) + (w[0] >> lsh0);  // (< 2^28: 2^14 x 2^14 blocks at most)
            // (the lane's block and its ceilings stay in registers until it moves to another block; both
            // ceilings come from one 32-bit load of svo_tree.d_ceilp: the block's ceiling and its parent block's)
            if (key != ckey) {
                ckey = key;
                cval = ceilp[key];
            }
            c0 = (int32_t)(int16_t)(cval & 0xFFFFu);
            c1 = (int32_t)cval >> 16;
            const bool p1 = y > c1;
            cl = p1 || y > c0;
            // above the tree's highest stored row (ESCAPE instances: top): every column is empty from there up to the
            // top of the world, so the box spans every x and z (a ray climbing out of the terrain band crosses it in one
            // move instead of one per 256-column block; its budget ends in it or it wraps in y)
            if (ESCAPE) gt = top >= 0 && y > top;
        }
        // (the box exits are taken only when a lane of the wave moves — wave-uniform; with the forward boxes gated
        // the same way, 1.1 % faster at C3 than per-lane selects: profiles/r03/ab_r03_x_*.log)
        any_cl = ceil_on && __ballot(cl) != 0ull;
        if (any_cl) {
            const int32_t y = (int32_t)w[1];
            const bool p1 = y > c1;
            uint32_t bmk = (1u << (p1 ? P.ceil_sh[1] : P.ceil_sh[0])) - 1u;  // block width - 1
            int32_t c = p1 ? c1 : c0;
            if (CEIL == T_CEIL_QUADS) {
                const uint32_t l = (lv - 1u) & 3u;  // (lanes with lv 0 take no box)
                bmk = (1u << (2u * (kCeilK0 + l))) - 1u;
                c = (int32_t)(int16_t)(cq >> (16u * l));
            }
            // steps to leave the box, less one: the block's faces in x / z, the ceiling (down) or the top
            // of the world (up) in y
            cex[0] = gt ? R.steps : (int32_t)(R.s[0] > 0 ? bmk - (w[0] & bmk) : (w[0] & bmk));
            cex[1] = R.s[1] < 0 ? y - (gt ? top : c) - 1 : (int32_t)(wm - w[1]);
            cex[2] = gt ? R.steps : (int32_t)(R.s[2] > 0 ? bmk - (w[2] & bmk) : (w[2] & bmk));
        }
        uint32_t kind = R_CEIL;
        if (!cl) {
            kind = lookup<LOOK>(P, mem, path, w, moved, par, sh, bmask, bref, binfo, st);
            jump = 0u;
        }
        // The lookup's outcome as lane predicates, taken once (an else-if chain here cost a lane-mask save, split and
        // rejoin per arm): a SOLID region or a brick; else the cell is empty, and the ray's budget is spent, or it
        // crosses the empty box in closed form (fast), or it steps through it voxel by voxel.  The budget is tested
        // before the crossing changes it.
        const bool k_solid = kind == R_SOLID, k_brick = kind == R_BRICK;
        const bool open = !k_solid && !k_brick && R.steps > 0;  // an empty cell with budget left
        const bool cross = open && fast;
        bool crossed = false;
        if (cross) {
            crossed = [&] {
                       int32_t ex[3];
                       if (REFLECT) dir_flags(R.s, ud);  // reflections and refractions flip steps
                       // (a wave whose every crossing is a ceiling move — the air above the terrain — skips the forward
                       // boxes: wave-uniform)
                       if (!any_cl || __ballot(!cl) != 0ull) {
                           box_exits(w, R.s, sh, par.mask, ud, ex);
                           if (any_cl) {
#pragma unroll
                               for (int k = 0; k < 3; k++) ex[k] = cl ? cex[k] : ex[k];
                           }
                       } else {
#pragma unroll
                           for (int k = 0; k < 3; k++) ex[k] = cex[k];
                       }
                       const bool moved_ok = skip_box<TRACK, RB>(R, ex, REFLECT ? SEG && __ballot(!lin) != 0ull : wseg);
                       if (ceil_on && cl && moved_ok) {
                           // (the voxel this move started from need not lie in the parent's region: the step
                           // that entered it — `moved` — counts too)
                           uint32_t wn[3];
                           wrap3(R, wm, wn);
                           jump = moved | (w[0] ^ wn[0]) | (w[1] ^ wn[1]) | (w[2] ^ wn[2]);
                           if (STATS) st.ceil_moves++;
                       }
                       return moved_ok;
                   }();
        }
        // a crossing that did not move: the budget ends inside this empty box (its steps are taken after the loop)
        const bool boxed = cross && !crossed;
        // not exact: voxel steps to the end of this (empty) 4^3 brick, then a lookup
        const bool walk = open && !fast;
        mat = k_solid ? binfo >> 16 : mat;
        done = (!k_brick && !open) || boxed;  // a SOLID region, a spent budget, or one that ends in this box
        pend = k_brick || walk;
        bmask = walk ? 0ull : bmask;
        // (ESCAPE: where a ray without a hit ends is not output — a miss whose budget ends in empty space skips them)
        if (ESCAPE && top >= 0) escaped = boxed;
        if (STATS) {
            if (k_brick) st.bricks++;
            if (boxed) st.skip_out++;
            if (crossed) {
                st.skips++;
                st.wv_skips += wave_lead();
                st.skip_by_sh[min(3u, (sh >> 1) - 1u)]++;
            }
        }
        if (pend) {
            // voxel steps inside the brick, solid mask in registers.  (Postponing bricks until
            // more lanes hold one, or bounding the steps per iteration, measured slower.)
            uint32_t w[3];
            wrap3(R, wm, w);
            // Voxel index v and per-axis steps left in the brick (one byte each) are stepped
            // instead of positions; positions follow from the step counts when the brick ends.
            // Steps left: 4 - c stepping up, c + 1 stepping down (c = the cell in the brick), i.e.
            // (c ^ 3) + 1 or c + 1 — all three bytes at once, biased by 0x7F (brick_walk).
            const uint32_t up3 = (R.s[0] > 0 ? 3u : 0u) | (R.s[1] > 0 ? 0x300u : 0u) | (R.s[2] > 0 ? 0x30000u : 0u);
            const uint32_t left0 = (((w[0] & 3u) | ((w[1] & 3u) << 8) | ((w[2] & 3u) << 16)) ^ up3) + 0x808080u;
            uint32_t left, v;
            bool solid;
            v = brick_walk<STATS, TRACK>(R, bmask, w, left0, left, solid, st);
            if (solid) {
                mat = brick_material(mats, bmask, bref, binfo, v);
                done = true;
            } else if (R.steps <= 0 && (left & 0x808080u) == 0x808080u) {
                done = true;  // budget ended inside the brick
            }
            const uint32_t dn = left0 - left;  // steps taken per axis, one byte each (no borrows)
            R.r[0] = step_by(R.r[0], (int32_t)(dn & 0xFFu), R.s[0], REFLECT ? 0u : ud[0]);
            R.r[1] = step_by(R.r[1], (int32_t)((dn >> 8) & 0xFFu), R.s[1], REFLECT ? 0u : ud[1]);
            R.r[2] = step_by(R.r[2], (int32_t)(dn >> 16), R.s[2], REFLECT ? 0u : ud[2]);
        }
        const uint32_t mfl = REFLECT && mat != kNoHit ? P.mat_flags[mat] : 0u;
        const uint32_t mflags = mfl & 7u;
        if (REFLECT && R.steps > 0 && mflags == 3u) {
            // a reflective block (flags & 7 == 3) with budget left: undo the last crossing on the
            // hit axis, mirror that axis (step and direction) and take the next DDA step from the
            // block, as low_res.frag:170-189 + :319-331 do
            const uint32_t ax = R.axis;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (ax == (uint32_t)k) {
                    R.T[k] -= R.a(k);
                    R.s[k] = -R.s[k];
                    bounce->d[k] = -bounce->d[k];
                }
            }
            bounce->n++;
            if (STATS) st.bends++;
#pragma unroll
            for (int k = 0; k < 3; k++) bounce->m[k] *= 0.94f;
            dda_step(R);
            done = false;
            mat = kNoHit;
        } else if (REFLECT && R.steps > 0 && mflags == 5u) {
            // a refractive block (glass, or liquid when the scene tree holds it) with budget left:
            // tint (liquid (0.94, 0.97, 1.0), else 0.95) and pass; the first one bends the ray
            // (refractRay, :211-240).  The shader's exact position is never advanced by its DDA: it
            // is the origin (minus 1 on axes with a negative initial step), +1 on the other axes with
            // a negative step, then min(new step, 0); deltaPos restarts from the current cell.
            const bool liquid = (mfl & 0x10u) != 0u;
            const float t0 = liquid ? 0.94f : 0.95f, t1 = liquid ? 0.97f : 0.95f, t2 = liquid ? 1.0f : 0.95f;
            if (STATS) {
                st.tints++;
                st.tint_iters++;
            }
            bounce->m[0] *= t0;
            bounce->m[1] *= t1;
            bounce->m[2] *= t2;
            uint32_t wr[3];
            wrap3(R, wm, wr);  // the refractive voxel (its region, when uniform, is passed below)
            if (!(bounce->n & kBent)) {
                bounce->n |= kBent;
                if (STATS) st.bends++;
                const uint32_t ax = R.axis;
                double ex[3];
                float nrm[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    ex[k] = (double)o[k];
                    if (d[k] < 0.0f) ex[k] -= 1.0;
                    if (ax != (uint32_t)k && R.s[k] < 0) ex[k] += 1.0;
                    if (ax == (uint32_t)k) nrm[k] = (float)R.s[k];
                }
                if (liquid) {
                    // the wave wobble (:225-229) at the shader's (float) exact position
                    const float arg = ((P.time + (float)ex[0] * 0.2f) - (float)ex[2] * 0.1f) * 10.0f;
                    nrm[0] += svo::sin_f32(arg) * 0.2f;
                    normalize3(nrm, nrm);
                }
                refract_dir(bounce->d, nrm);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float dk = bounce->d[k];
                    const int32_t s = dk < 0.0f ? -1 : 1;
                    const double delta = (double)svo::rcp_rn(dk);
                    const double ad = delta >= 0.0 ? delta : -delta;
                    if (s < 0) ex[k] -= 1.0;
                    R.T[k] = ad - (ex[k] - (double)R.r[k]) * delta;
                    R.s[k] = s;
                    R.af[k] = (float)ad;
                    R.ia[k] = __builtin_amdgcn_rcpf((float)ad);
                }
                // (deltaPos restarts from the shader's origin, not the current cell: |T| / absDelta
                // is bounded by the distance travelled, so the initial budget is held below 2^19 to
                // keep the count estimates within 1/2 — count_est)
                fast = !(P.flags & SVO_CAST_ITERATIVE) && budget < (1 << 19) && axis_ok(R.T[0], R.a(0)) && axis_ok(R.T[1], R.a(1)) &&
                       axis_ok(R.T[2], R.a(2)) && span_ok(R);
                lin = fast && exact_axis(R.T[0], R.a(0), R.steps) && exact_axis(R.T[1], R.a(1), R.steps) && exact_axis(R.T[2], R.a(2), R.steps);
                if (!SEG) fast = lin;  // (REFLECT runs in SEG instances)
            }
            dda_step(R);
            done = false;
            const uint32_t keep = mat;
            mat = kNoHit;
            if (kind == R_SOLID) {
                // the rest of a uniform refractive region (a lake's body): the same block voxel after
                // voxel — tint and step without lookups; its 2^sh-wide aligned region is the child
                // slot of `par` the lookup ended in.  A voxel reached with no budget left is the hit.
                for (;;) {
                    uint32_t w[3];
                    wrap3(R, wm, w);
                    if (((w[0] ^ wr[0]) | (w[1] ^ wr[1]) | (w[2] ^ wr[2])) >> par.sh) break;
                    if (R.steps <= 0) {
                        mat = keep;
                        done = true;
                        break;
                    }
                    bounce->m[0] *= t0;
                    bounce->m[1] *= t1;
                    bounce->m[2] *= t2;
                    if (STATS) st.tints++;
                    dda_step(R);
                }
            } else if (kind == R_BRICK) {
                // the rest of the brick (a lake's surface layer: water and air in one brick): its voxel mask and
                // materials are at hand, so refractive voxels are passed (each tints with its own block) and empty
                // ones stepped without lookups; any other block ends the ray there (a mirror with budget left is
                // left to the next iteration, which reflects it), and leaving the brick ends the pass (a lookup)
                for (;;) {
                    uint32_t w[3];
                    wrap3(R, wm, w);
                    if (((w[0] ^ wr[0]) | (w[1] ^ wr[1]) | (w[2] ^ wr[2])) >> 2) break;
                    const uint32_t v = child_slot(w[0], w[1], w[2], 0u);
                    if ((bmask >> v) & 1ull) {
                        const uint32_t m2 = brick_material(mats, bmask, bref, binfo, v);
                        const uint32_t f2 = P.mat_flags[m2];
                        if ((f2 & 7u) != 5u || R.steps <= 0) {
                            if ((f2 & 7u) != 3u || R.steps <= 0) {
                                mat = m2;  // the hit
                                done = true;
                            }
                            break;
                        }
                        const bool lq = (f2 & 0x10u) != 0u;
                        bounce->m[0] *= lq ? 0.94f : 0.95f;
                        bounce->m[1] *= lq ? 0.97f : 0.95f;
                        bounce->m[2] *= lq ? 1.0f : 0.95f;
                        if (STATS) st.tints++;
                    } else if (R.steps <= 0) {
                        done = true;  // the budget ends in an empty voxel
                        break;
                    }
                    dda_step(R);
                }
            }
        }
        // Progress guard, by construction: every iteration that does not end the ray takes at least one
        // DDA step (a crossing takes its exit step, a brick walk its first step, a reflection / refraction
        // its next one), so the budget strictly decreases.  An iteration that left the budget where it was,
        // or grew it — only a wrong crossing count could (a saturated or wrapped estimate, as before commit
        // 1a85dd6) — ends the ray: the launch always ends.  (STATS counts the trips: 0 in every test.)
        if (R.steps >= steps_in && !done) {
            if (STATS) st.no_progress++;
            R.steps = -1;  // marked in every build: the record's steps_left is -1 and the tree's trip counter counts it
            done = true;
        }
    }
    const bool hit = mat != kNoHit;
    // (out of the loop, so the stepping loop's state copies stay off every skip, and the lanes
    // whose budget ends in empty space take their last steps together).  Every other way out of
    // the loop without a hit has spent the budget.
    if (!hit && !escaped) {
        while (R.steps > 0) {
            dda_step(R);
            if (STATS) st.plain_steps++;
        }
    }
    if (par_out) *par_out = par;
    if (XS == T_XS_SAVE && hit) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            xs->T[k] = R.T[k];
            xs->r[k] = R.r[k];
        }
        xs->steps = R.steps;
        xs->axis = R.axis;
    }
    if (STATS) {
        // SIMD efficiency: a lane's work units (lookups + voxel steps) against the wave's maximum
        const uint32_t work = st.lookups + st.brick_steps + st.plain_steps;
        const uint32_t wmax = wave_max(work), wsum = wave_sum(work);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(P.stats + S_LANE_WORK, (unsigned long long)wsum);
            atomicAdd(P.stats + S_WAVE_MAX_WORK_X64, (unsigned long long)wmax * 64ull);
        }
        atomicAdd(P.stats + S_RAYS, 1ull);
        atomicAdd(P.stats + S_LOOKUPS, (unsigned long long)st.lookups);
        atomicAdd(P.stats + S_LOADS, (unsigned long long)st.loads);
        atomicAdd(P.stats + S_SKIPS, (unsigned long long)st.skips);
        atomicAdd(P.stats + S_SKIP_OUT, (unsigned long long)st.skip_out);
        atomicAdd(P.stats + S_BRICK_STEPS, (unsigned long long)st.brick_steps);
        atomicAdd(P.stats + S_PLAIN_STEPS, (unsigned long long)st.plain_steps);
        for (int k = 0; k < 4; k++) atomicAdd(P.stats + S_SKIPS_4 + k, (unsigned long long)st.skip_by_sh[k]);
        atomicAdd(P.stats + S_BRICKS, (unsigned long long)st.bricks);
        atomicAdd(P.stats + S_WV_ITERS, (unsigned long long)st.wv_iters);
        atomicAdd(P.stats + S_WV_BRICK, (unsigned long long)st.wv_brick);
        atomicAdd(P.stats + S_ROOT_STARTS, (unsigned long long)st.root_starts);
        atomicAdd(P.stats + S_CACHE_EMPTY, (unsigned long long)st.cache_empty);
        atomicAdd(P.stats + S_WV_SKIPS, (unsigned long long)st.wv_skips);
        atomicAdd(P.stats + S_WV_DESCENTS, (unsigned long long)st.wv_descents);
        atomicAdd(P.stats + S_PATH_STARTS, (unsigned long long)st.path_starts);
        if (st.no_progress) atomicAdd(P.stats + S_NO_PROGRESS, (unsigned long long)st.no_progress);
        atomicAdd(P.stats + S_CEIL_MOVES, (unsigned long long)st.ceil_moves);
        atomicAdd(P.stats + S_ABOVE_TOP, (unsigned long long)st.above_top);
        atomicAdd(P.stats + S_BENDS, (unsigned long long)st.bends);
        atomicAdd(P.stats + S_TINTS, (unsigned long long)st.tints);
        atomicAdd(P.stats + S_TINT_ITERS, (unsigned long long)st.tint_iters);
        atomicAdd(P.stats + S_MARCH_FINE, (unsigned long long)st.march_fine);
        atomicAdd(P.stats + S_MARCH_DESCENTS, (unsigned long long)st.march_descents);
        atomicAdd(P.stats + S_MARCH_64, (unsigned long long)st.march_64);
        atomicAdd(P.stats + S_MARCH_256, (unsigned long long)st.march_256);
        // per-ray work (offline analysis, bench.py SVO_RAY_WORK): 16-bit fields, lookups | iterations | brick steps | node loads
        if (ray_work)
            *ray_work = (unsigned long long)min(st.lookups, 65535u) | ((unsigned long long)min(st.iters, 65535u) << 16) |
                        ((unsigned long long)min(st.brick_steps, 65535u) << 32) | ((unsigned long long)min(st.loads, 65535u) << 48);
    }
    if (!TRACK && !NO_T && R.axis < 3u) {
        // the last step's crossing: T - a exactly (exact sums); an infinite absDelta only comes
        // with an infinite crossing (deltaPos = inf - frac * inf), which stays inf
        const double Ta = R.axis == 0u ? R.T[0] : (R.axis == 1u ? R.T[1] : R.T[2]);
        const float aa = R.axis == 0u ? R.af[0] : (R.axis == 1u ? R.af[1] : R.af[2]);
        R.tlast = __builtin_isinf(aa) ? Ta : Ta - (double)aa;
    }
    Hit h;
    h.x = R.r[0];
    h.y = R.r[1];
    h.z = R.r[2];
    // (a miss has spent its budget or escaped: 0; a progress-guard trip: -1)
    h.steps_left = hit ? R.steps : min(R.steps, 0);
    if (R.steps < 0 && P.guard_trips) atomicAdd(P.guard_trips, 1u);
    h.t = (float)R.tlast;  // (one rounding of the same double as before)
    const int32_t sa = R.axis == 0u ? R.s[0] : (R.axis == 1u ? R.s[1] : R.s[2]);
    const uint32_t neg = (R.axis < 3u && sa < 0) ? 1u : 0u;
    h.info = (hit ? HIT_BIT : 0u) | (R.axis << AXIS_SHIFT) | (neg ? NEG_BIT : 0u) | (hit ? mat & MAT_MASK : 0u);
    if (ESCAPE && escaped) h.info |= ESC_BIT;  // (its position is where the escape began, not where the budget ends)
    return h;
}
