// svo_cast_kernel.h — the gfx950 cast kernel of libsvo_rt: the primary-ray SVO traversal that replaces
// RAY_CASTER::castRayFromCam (src/ray_caster.cpp:54-87) and the DDA + tree walk of
// src/shaders/low_res.frag:256-333,446-531.
//
// Semantics are castRayFromCam's, bit for bit: FP64 DDA from trunc(origin), strict-< axis choice
// with ties / NaN falling to z, one voxel per step, the start voxel never tested, LIQUID and empty
// blocks passed through, coordinates wrapped modulo the extent.  What the kernel changes is how a
// step finds its block: the ray keeps the deepest region it knows (an empty child region of some
// level, or a 4^3 brick whose 64-bit solid mask sits in registers) and only walks the tree again
// when a step leaves that region, so most steps touch no memory.
//
// k_cast is defined here and instantiated, one family per file, by svo_cast_inst_*.hip; svo_cast.hip launches them.
#pragma once

#include <type_traits>

#include "svo_cast_instances.h"
#include "svo_shade.h"
#include "svo_wire.h"

// Frame mode: the pixel of this lane of launch block blk (its ray o, d and record index out; out = -1 for lanes past the
// frame's edge).  8-pixel tile rows, one wavefront per 2^(6-lh) x 2^lh footprint; frames interleave wave by wave (every
// frame's long top rows first); the frame and tile indices are wave-uniform: their divisions run on the scalar unit.
__device__ __forceinline__ void frame_pixel(const CastParams& P, int64_t blk, float o[3], float d[3], int64_t& out, uint32_t& frm,
                                            int32_t* pxy = nullptr) {
    const uint32_t wv = (uint32_t)blk * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t fr = wv % (uint32_t)P.n_frames, tile = wv / (uint32_t)P.n_frames;
    frm = fr;
    const int32_t lane = (int32_t)(threadIdx.x & 63u);
    // (small launches: the first half_rows tile rows dispatched are cast by half footprints — two adjacent waves of 32
    // lanes per footprint, 2^(lh-1) pixel rows each; frame_half_rows)
    const uint32_t h2 = (uint32_t)P.half_rows * 2u * (uint32_t)P.tiles_x;
    uint32_t tq, tx_;
    int32_t half = -1;
    if (tile < h2) {
        tq = tile / (2u * (uint32_t)P.tiles_x);
        const uint32_t t2 = tile - tq * 2u * (uint32_t)P.tiles_x;
        tx_ = t2 >> 1;
        half = (int32_t)(t2 & 1u);
    } else {
        const uint32_t t = tile - h2 + (uint32_t)P.half_rows * (uint32_t)P.tiles_x;
        tq = t / (uint32_t)P.tiles_x;
        tx_ = t - tq * (uint32_t)P.tiles_x;
    }
    int32_t trl = (int32_t)tq;
    // default order: top tile rows first (rays nearest the horizon travel furthest; dispatching
    // them first keeps the long tiles out of the launch's tail)
    if (!(P.flags & SVO_CAST_BOTTOM_FIRST)) trl = P.tile_rows_local - 1 - trl;
    const int32_t tx = (int32_t)tx_;
    const int32_t tr = P.tile_row_start + trl * P.tile_row_step;
    // the wavefront's 2^(6-lh) x 2^lh pixels of its 8-pixel tile row (lh = 3: an 8x8 tile); the
    // sub-rows of one column of footprints are adjacent waves
    const int32_t lh = P.tile_lh, lw = 6 - lh, sub = 3 - lh;
    const int32_t rr = ((tx & ((1 << sub) - 1)) << lh) + (half >= 0 ? (half << (lh - 1)) : 0) + (lane >> lw);
    const int32_t px = ((tx >> sub) << lw) + (lane & ((1 << lw) - 1)), py = tr * 8 + rr;
    if (trl >= 0 && trl < P.tile_rows_local && px < P.width && py < P.height && !(half >= 0 && lane >= 32)) {
        raygen_pixel(P.rg, px, py, d);
        o[0] = P.frame_org[3 * fr + 0];
        o[1] = P.frame_org[3 * fr + 1];
        o[2] = P.frame_org[3 * fr + 2];
        out = (int64_t)fr * P.frame_records + ((int64_t)trl * 8 + rr) * P.width + px;
        if (pxy) {
            pxy[0] = px;
            pxy[1] = py;
        }
    }
}

template <bool STATS, bool STAMPS, bool AO, bool SHADE, bool WIDE, bool SEG, int DIRS = 0, bool NOREC = false>
// primary rays: 64 VGPRs = 8 waves per SIMD without spills; the AO instances run 8 waves too (4 spilled VGPRs; with
// the hemisphere table read from the kernel arguments instead of LDS, the LDS allows 8 waves: C4 0.2441 -> 0.2311 ms
// against 6 waves at 79 VGPRs, 0.2349 at 7); the diagnostics instances 6; the shading instances 7 waves on the camera's
// octant (kShadeWaves), 6 with generic signs
__global__ __launch_bounds__(kBlock, STATS ? 6 : (SHADE ? (DIRS != 0 ? kShadeWaves : 6) : 8)) void k_cast(const CastParams P) {
    using Mem = typename std::conditional<WIDE, WideNodes, BufNodes>::type;
    const Mem mem(P.nodes);
    const Mem smem(SHADE ? P.snodes : P.nodes);  // shading: shadow rays walk the solid view
    // diagnostics: block start / end stamps (100 MHz s_memrealtime) after the 16 counters
    // (frame schedules: shading instances only — sched_attach; the primary instances compile without the hooks)
    const bool sched = SHADE && P.sched_cost;
    const unsigned long long t_start = (STAMPS || sched) ? __builtin_amdgcn_s_memrealtime() : 0ull;
    // per-lane node path (mask and first-child index of the interior node at each depth of the
    // last descent), [depth][lane]
    // (dynamic LDS: the launch's own depth, path_lds — a 6-level tree's shading launch fits 7 blocks per SIMD)
    extern __shared__ uint32_t path_words[];
    const Path path = {path_words + threadIdx.x};
    // (the hemisphere AO sample set is read from the kernel arguments: uniform loads, no LDS)
    __shared__ Bounce shade_bn[SHADE ? kBlock : 1];  // shading: the rays' bounce state (k_cast SHADE below)
    int64_t blk = blockIdx.x;
    // (frame mode: the schedule's group of kSchedGroup blocks at this dispatch slot's group)
    if (SHADE && P.sched_order) blk = (int64_t)P.sched_order[blockIdx.x / kSchedGroup] * kSchedGroup + blockIdx.x % kSchedGroup;
    const int64_t g = blk * kBlock + threadIdx.x;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    int64_t out = -1;
    uint32_t frm = 0u;  // the wave's frame (frame mode)
    if (P.mode == MODE_FRAME) {
        frame_pixel(P, blk, o, d, out, frm);
    } else if (P.mode == MODE_EXPLICIT) {
        if (g < P.n_rays) {
            d[0] = P.rdir[3 * g + 0];
            d[1] = P.rdir[3 * g + 1];
            d[2] = P.rdir[3 * g + 2];
            if (P.rorg) {
                o[0] = P.rorg[3 * g + 0];
                o[1] = P.rorg[3 * g + 1];
                o[2] = P.rorg[3 * g + 2];
            } else {
                o[0] = P.org[0];
                o[1] = P.org[1];
                o[2] = P.org[2];
            }
            out = g;
        }
    } else if (g == 0) {
        for (int a = 0; a < 3; a++) {
            d[a] = P.sdir[a];
            o[a] = P.org[a];
        }
        out = 0;
    }
    if (SHADE && out >= 0) {
        // the ray's bounce state lives in LDS: the trace touches it only at reflections / refractions, and in registers
        // it cost the loop spills (22 VGPRs at 8 waves; 0.4748 -> 0.4660 ms per shaded C3 frame at 5 waves without them)
        Bounce& bn = shade_bn[threadIdx.x];
        bn = {{d[0], d[1], d[2]}, 0, {1.0f, 1.0f, 1.0f}};
        // rays may escape (stop early once only empty voxels lie ahead) unless their end position is output (hit records)
        // or could be the highlighted lookingAtBlock (low_res.frag:347 compares every ray's end, misses too): a look-at
        // voxel the scene may not store — the host's, checked on the host, or a device pick record that is not a sure hit
        // (stepsLeft 0: a miss or a hit on the last step) (uniform)
        const bool look_risk = P.look_dev ? P.look_dev[6] <= 0 : (P.look_valid && P.look_empty);
        const int32_t esc = (P.pos || look_risk) ? -1 : P.top_scene;
        unsigned long long* const rw = P.stats ? P.stats + SVO_STATS_HEADER + 2 * (int64_t)gridDim.x * (kBlock / 64) + out : nullptr;
        if (STATS || STAMPS) {  // (diagnostics: one trace, bounces included)
            const Hit h = trace<t_if(STATS, T_STATS) | T_REFLECT | T_ESCAPE | t_if(SEG, T_SEG) | T_CEIL_QUADS | t_if(NOREC, T_NO_T)>(
                P, mem, P.mats, path, o, d, P.steps, rw, &bn, nullptr, esc, P.top_scene);
            shade_out<0>(P, smem, path, h, bn, out);
        } else {
            // the straight trace to the first block hit — no reflection / refraction upkeep per step, on the camera's step
            // octant (DIRS) — and only a mirror or a refractive block with budget left hands its state on to the bouncing
            // trace, which resumes there (shaded C3 0.3103 -> 0.3027 ms, then 0.2914 with the octant; the straight trace's
            // state on its first hit is the one the bouncing trace from the origin reaches: both take castRayFromCam's
            // exact steps).  Its column ceilings: the launch's two levels (T_CEIL_PAIRS, as primary casts: 0.8 % faster than
            // the walk over every level, T_CEIL_QUADS, which the bouncing trace keeps)
            RayState xs;
            Hit h = trace<T_ESCAPE | t_if(SEG, T_SEG) | t_dirs(DIRS) | T_CEIL_PAIRS | t_if(NOREC, T_NO_T) | T_XS_SAVE>(
                P, mem, P.mats, path, o, d, P.steps, nullptr, nullptr, nullptr, esc, P.top_scene, DIRS != 0 ? &P.fax[frm] : nullptr, &xs);
            const uint32_t mf = ((h.info & HIT_BIT) && h.steps_left > 0) ? P.mat_flags[h.info & MAT_MASK] & 7u : 0u;
            if (mf == 3u || mf == 5u)
                h = trace<T_REFLECT | T_ESCAPE | T_SEG | T_CEIL_QUADS | t_if(NOREC, T_NO_T) | T_XS_RESUME>(
                    P, mem, P.mats, path, o, d, P.steps, nullptr, &bn, nullptr, esc, P.top_scene, nullptr, &xs);
            shade_out<0>(P, smem, path, h, bn, out);
        }
    } else if (out >= 0) {
        Parent pfin;
        const Hit h = trace<t_if(STATS, T_STATS) | t_if(SEG, T_SEG) | t_dirs(DIRS) | t_if(AO, T_KEEPPAR) | T_CEIL_PAIRS>(
            P, mem, P.mats, path, o, d, P.steps, P.stats ? P.stats + SVO_STATS_HEADER + 2 * (int64_t)gridDim.x * (kBlock / 64) + out : nullptr,
            nullptr, AO ? &pfin : nullptr, -1, P.top_solid, DIRS != 0 ? &P.fax[frm] : nullptr);
        if (!SHADE && P.wire) {  // (wave-uniform: one launch writes one kind of record)
            wire_put(P.wire, P.wire_compact != 0, out, o, h.x, h.y, h.z, h.t, h.info);
        } else {
            reinterpret_cast<int4*>(P.pos)[out] = make_int4(h.x, h.y, h.z, h.steps_left);
            P.t[out] = h.t;
            P.info[out] = h.info;
        }
        if (AO) {
            // AO rays from the centre of lastPos, pole turned to the hit face's normal (A8)
            uint32_t cnt = 0u;
            if (h.info & HIT_BIT) {
                const uint32_t ax = (h.info >> AXIS_SHIFT) & 3u;
                const int32_t st = (h.info & NEG_BIT) ? -1 : 1;  // step on the hit axis
                const int32_t lx = h.x - (ax == 0u ? st : 0), ly = h.y - (ax == 1u ? st : 0), lz = h.z - (ax == 2u ? st : 0);
                const int32_t l[3] = {lx, ly, lz};
                if (P.ao_plan && pfin.sh < 2u * (uint32_t)P.levels && (uint32_t)lx < (1u << 23) && (uint32_t)ly < (1u << 23) && (uint32_t)lz < (1u << 23)) {
                    uint32_t aol = 0u;
                    cnt = ao_count_plan(P, mem, path, pfin, h, l, ax, -st, aol);
                    if (STATS) atomicAdd(P.stats + S_AO_NODE_LOADS, (unsigned long long)aol);
                } else {
                    const float ao_o[3] = {(float)lx + 0.5f, (float)ly + 0.5f, (float)lz + 0.5f};
                    for (int32_t i = 0; i < P.ao_n; i++) {
                        const float hv[3] = {P.ao_tab[3 * i], P.ao_tab[3 * i + 1], P.ao_tab[3 * i + 2]};
                        float ad[3];
                        ao_dir(hv, ax, -st, ad);
                        const Hit a = trace<T_PLAIN>(P, mem, P.mats, path, ao_o, ad, P.ao_steps);
                        cnt += (a.info & HIT_BIT) ? 1u : 0u;
                    }
                }
            }
            P.ao[out] = (uint8_t)cnt;
        }
    }
    if (STAMPS || sched) {
        const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();  // (one wavefront per block: every lane is done)
        if (threadIdx.x == 0) {
            if (STAMPS) {
                P.stats[SVO_STATS_HEADER + 2 * blockIdx.x] = t_start;
                P.stats[SVO_STATS_HEADER + 2 * blockIdx.x + 1] = t_end;
            }
            if (sched) P.sched_cost[blk] = (uint32_t)std::min(t_end - t_start, 0xFFFFFFFFull);
        }
    }
}

// every svo_cast_inst_*.hip defines one family of svo_cast_instances.h, every other translation unit only declares them
#define SVO_CAST_INSTANCE(...) template __global__ void k_cast<__VA_ARGS__>(const CastParams P);
#define SVO_CAST_EXTERN(...) extern SVO_CAST_INSTANCE(__VA_ARGS__)
SVO_CAST_PRIMARY(SVO_CAST_EXTERN)
SVO_CAST_AO(SVO_CAST_EXTERN)
SVO_CAST_SHADING(SVO_CAST_EXTERN)
SVO_CAST_SHADING_NOREC(SVO_CAST_EXTERN)
SVO_CAST_DIAGNOSTICS(SVO_CAST_EXTERN)
