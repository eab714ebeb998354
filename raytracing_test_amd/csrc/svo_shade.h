// svo_shade.h — device code of the shading pass and of the planned hemisphere AO over trace()'s hits.
#pragma once

#include "svo_trace.h"

// ------------------------------------------------------------------------------------------------
// Shading: low_res.frag's colour model over castRayFromCam hits — sky
// (genSkyBox :157-168), sun lighting (calcLightIntensity :242-252), 75-step shadow ray (:373-391),
// the looked-at block highlight (:340-343), reflections (:170-189) and refractions of solids
// (:196-240); the last two are applied inside trace.
// Single precision in the shader's operation order (-ffp-contract=off).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float3 color_of(uint64_t c) {  // color_int_to_vec3 (:139-145)
    const double sc = 1.0 / 2097152.0;
    return make_float3((float)((double)(c >> 42) * sc), (float)((double)((c >> 21) & 0x1FFFFFull) * sc),
                       (float)((double)(c & 0x1FFFFFull) * sc));
}

__device__ __forceinline__ float sigmoidf(float x, float scale, float k) { return 1.0f / (1.0f + expf(-x * k)) * scale; }

__device__ __forceinline__ float3 sky_color(const float d[3], const float sun[3]) {
    float dy = d[1];
    if (dy < 0.0f) dy *= 1.4f;
    const float haze = (0.1f - fabsf(fminf(fmaxf(dy, -0.3f), 0.3f))) * 0.8f + 0.1f;
    const float modifier = fminf(fmaxf(sigmoidf(1.0f - (haze * 2.0f), 1.0f, 2.0f), 0.0f), 1.0f);
    const float ex = d[0] - sun[0], ey = dy - sun[1], ez = d[2] - sun[2];
    const float b = sqrtf((ex * ex + ey * ey) + ez * ez) * 50.0f;
    const float sv = sigmoidf(1.5f - b, 1.0f, 1.6f);
    const float h3 = fminf(fmaxf(haze, 0.0f), 1.0f) * 3.0f;
    return make_float3((0.2f + h3) * modifier + sv, (0.4f + h3) * modifier + sv, (1.0f + h3) * modifier + 0.0f);
}

// ------------------------------------------------------------------------------------------------
// Hemisphere AO from a plan (A8).  An AO ray starts at the centre of lastPos: for a cell c >= 0,
// dda_axis gives deltaPos = absDelta - (+-0.5) * delta whatever c is, so the voxels a ray of
// direction d visits are lastPos + a fixed offset sequence, and the ray hits iff one of its
// ao_steps voxels is solid (castRayFromCam never tests the start voxel).  The host simulates the
// DDA of every (sample, hit face) once (ao_plan_get); per face the distinct offsets, each with the
// mask of samples passing through it, are grouped by the 4^3 brick they fall in — which depends on
// where lastPos sits in its brick, so there is one group list per (face, alignment).  Per hit,
// each brick is looked up once (skipped when all its samples already hit), starting at the deepest
// node of the primary ray's LDS path holding both the hit voxel and the brick; its solid plan voxels
// add their samples.  The count is the popcount of the samples hit.
// Plan layout (u32 words): [2g, 2g+1] = first record (16-B units), bricks, for g = face*64 + align
// (face = 2*axis + (sign < 0), align = lastPos & 3 per axis as z<<4|y<<2|x); per brick: {packed
// brick offset (bx+128 | by+128 << 8 | bz+128 << 16), 0, voxel mask lo, hi}, {union of its sample
// masks lo, hi, 0, 0}, then one u64 sample mask per voxel of the voxel mask in bit order (padded
// to 16 B).
// ------------------------------------------------------------------------------------------------
// A plan brick's lookup starts at the deepest node of the primary ray's LDS path holding both the hit voxel and the
// brick's corner w (mask / ref / child shift); an empty or SOLID region of any level covers whole bricks (0 or ~0)
__device__ __forceinline__ void brick_start(const CastParams& P, const Path& path, const uint32_t w[3], const uint32_t hw[3], int32_t dmax,
                                            uint64_t& mask, uint32_t& ref, uint32_t& sh) {
    const uint32_t diff = ((w[0] ^ hw[0]) | (w[1] ^ hw[1]) | (w[2] ^ hw[2])) | 1u;
    const int32_t da = min(P.levels - 1 - (int32_t)((31u - (uint32_t)__builtin_clz(diff)) >> 1), dmax);  // (diff != 0)
    mask = path.mask(da);
    ref = path.ref(da);
    sh = (uint32_t)(2 * (P.levels - 1 - da));
}

// loads: node loads of the plan's brick lookups (counted for SVO_CAST_STATS; dead code elsewhere)
template <class Mem>
__device__ __forceinline__ uint32_t ao_count_plan(const CastParams& P, const Mem& mem, const Path& path,
                                                  const Parent& pfin, const Hit& h, const int32_t l[3], uint32_t ax, int32_t sg,
                                                  uint32_t& loads) {
    const uint32_t face = 2u * ax + (sg < 0 ? 1u : 0u);
    const uint32_t al = ((uint32_t)l[0] & 3u) | (((uint32_t)l[1] & 3u) << 2) | (((uint32_t)l[2] & 3u) << 4);
    const uint2 hd = reinterpret_cast<const uint2*>(P.ao_plan)[face * 64u + al];
    const uint4* r = reinterpret_cast<const uint4*>(P.ao_plan) + hd.x;
    const uint32_t wm = P.wmask;
    const uint32_t hw[3] = {(uint32_t)h.x & wm, (uint32_t)h.y & wm, (uint32_t)h.z & wm};
    const uint32_t hb[3] = {(uint32_t)l[0] >> 2, (uint32_t)l[1] >> 2, (uint32_t)l[2] >> 2};
    const int32_t dmax = P.levels - 1 - (int32_t)(pfin.sh >> 1);
    const uint64_t all = P.ao_n >= 64 ? ~0ull : ((1ull << P.ao_n) - 1ull);
    uint64_t hits = 0ull;
    // the plan's bricks two at a time: both lookups descend in one loop, so their node loads are in flight together
    // (C4 -1.2 %, 20 AO rays -1.5 %: profiles/r06/ab_aopair_*.txt; three or four at a time spill 38 / 72 VGPRs).  A brick
    // whose samples all hit before its pair started is not looked up; one the pair's first brick would have covered is
    // looked up anyway — the union of the samples hit, the count, is the same
    for (uint32_t j = 0; j < hd.y && hits != all; j += 2u) {
        const uint4 e0 = r[0], u0 = r[1];
        const uint64_t vm0 = (uint64_t)e0.z | ((uint64_t)e0.w << 32), um0 = (uint64_t)u0.x | ((uint64_t)u0.y << 32);
        const uint2* sm0 = reinterpret_cast<const uint2*>(r + 2);
        r += 2u + (((uint32_t)__popcll(vm0) + 1u) >> 1);
        const bool has1 = j + 1u < hd.y;
        uint4 e1 = make_uint4(0u, 0u, 0u, 0u), u1 = make_uint4(0u, 0u, 0u, 0u);
        const uint2* sm1 = nullptr;
        if (has1) {
            e1 = r[0];
            u1 = r[1];
            sm1 = reinterpret_cast<const uint2*>(r + 2);
            r += 2u + (((uint32_t)__popcll((uint64_t)e1.z | ((uint64_t)e1.w << 32)) + 1u) >> 1);
        }
        const uint64_t vm1 = (uint64_t)e1.z | ((uint64_t)e1.w << 32), um1 = (uint64_t)u1.x | ((uint64_t)u1.y << 32);
        bool more0 = (hits & um0) != um0, more1 = has1 && (hits & um1) != um1;
        uint64_t mk0 = 0ull, mk1 = 0ull, res0 = 0ull, res1 = 0ull;
        uint32_t rf0 = 0u, rf1 = 0u, sh0 = 0u, sh1 = 0u, w0[3], w1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            w0[k] = ((hb[k] + ((e0.x >> (8 * k)) & 255u) - 128u) << 2) & wm;
            w1[k] = ((hb[k] + ((e1.x >> (8 * k)) & 255u) - 128u) << 2) & wm;
        }
        if (more0) brick_start(P, path, w0, hw, dmax, mk0, rf0, sh0);
        if (more1) brick_start(P, path, w1, hw, dmax, mk1, rf1, sh1);
        while (more0 || more1) {
            Node n0, n1;
            bool ld0 = false, ld1 = false;
            if (more0) {
                const uint64_t t = slot_top(mk0, child_slot(w0[0], w0[1], w0[2], sh0));
                ld0 = (int64_t)t < 0;
                if (ld0) n0 = mem.load(popc_add(t, rf0));
                more0 = false;
            }
            if (more1) {
                const uint64_t t = slot_top(mk1, child_slot(w1[0], w1[1], w1[2], sh1));
                ld1 = (int64_t)t < 0;
                if (ld1) n1 = mem.load(popc_add(t, rf1));
                more1 = false;
            }
            if (ld0) {
                loads++;
                const uint32_t kind = n0.info & K_KIND_MASK;
                if (kind == K_INTERIOR) {
                    mk0 = n0.mask;
                    rf0 = n0.ref;
                    sh0 -= 2u;
                    more0 = true;
                } else {
                    res0 = kind == K_SOLID ? ~0ull : n0.mask;
                }
            }
            if (ld1) {
                loads++;
                const uint32_t kind = n1.info & K_KIND_MASK;
                if (kind == K_INTERIOR) {
                    mk1 = n1.mask;
                    rf1 = n1.ref;
                    sh1 -= 2u;
                    more1 = true;
                } else {
                    res1 = kind == K_SOLID ? ~0ull : n1.mask;
                }
            }
        }
        uint64_t m = res0 & vm0;
        while (m) {  // the plan voxels of this brick that are solid: their samples hit
            const uint32_t v = (uint32_t)__builtin_ctzll(m);
            const uint2 smv = sm0[__popcll(vm0 & ((1ull << v) - 1ull))];
            hits |= (uint64_t)smv.x | ((uint64_t)smv.y << 32);
            m &= m - 1ull;
        }
        m = res1 & vm1;
        while (m) {
            const uint32_t v = (uint32_t)__builtin_ctzll(m);
            const uint2 smv = sm1[__popcll(vm1 & ((1ull << v) - 1ull))];
            hits |= (uint64_t)smv.x | ((uint64_t)smv.y << 32);
            m &= m - 1ull;
        }
    }
    return (uint32_t)__popcll(hits);
}

// WIDE: 64-bit node addresses (trees above kNarrowNodes nodes, or SVO_CAST_WIDE_ADDR)
// The shading of a finished ray (low_res.frag:319-391 over castRayFromCam hits): its hit record (when requested) and its
// colour — the looked-at highlight, the sky of its final direction, or the lit / shadowed block (a 75-step shadow ray
// from the centre of lastPos through the solid view, smem); bn: its reflections / refraction (Bounce).  DIRS: the sun's
// step octant (0: per-wave sign flags)
template <int DIRS, class Mem>
__device__ __forceinline__ void shade_out(const CastParams& P, const Mem& smem, const Path& path, const Hit& h, const Bounce& bn, int64_t out) {
    if (P.pos) {
        reinterpret_cast<int4*>(P.pos)[out] = make_int4(h.x, h.y, h.z, h.steps_left);
        P.t[out] = h.t;
        P.info[out] = h.info;
    }
    const bool hit = (h.info & HIT_BIT) != 0u;
    const float* m = bn.m;  // finalColorMod
    float3 c;
    int32_t lk[3] = {P.look[0], P.look[1], P.look[2]};
    bool lv = P.look_valid != 0;
    if (P.look_dev) {  // (uniform: the pick ray's record, written on this stream before the launch)
        lk[0] = P.look_dev[0];
        lk[1] = P.look_dev[1];
        lk[2] = P.look_dev[2];
        lv = true;
    }
    // (an escaped ray's position is not its end; it can only end on a voxel the scene does not store, and the launch lets
    // rays escape only when the look-at voxel is stored: k_cast's `esc`)
    if (lv && !(h.info & ESC_BIT) && h.x == lk[0] && h.y == lk[1] && h.z == lk[2]) {
        const float3 b = color_of(P.mat_color[hit ? (h.info & MAT_MASK) : 0u]);
        c = make_float3(b.x * 2.0f + 0.3f, b.y * 2.0f + 0.3f, b.z * 2.0f + 0.3f);
    } else if (!hit) {
        const float3 sk = sky_color(bn.d, P.sun);
        c = make_float3(sk.x * m[0], sk.y * m[1], sk.z * m[2]);
    } else {
        const float3 col = color_of(P.mat_color[h.info & MAT_MASK]);
        const uint32_t ax = (h.info >> AXIS_SHIFT) & 3u;
        const int32_t sg = (h.info & NEG_BIT) ? -1 : 1;  // the ray's step on the hit axis
        const float l = (ax == 0u ? P.sun[0] : (ax == 1u ? P.sun[1] : P.sun[2])) * (float)(-sg);
        const bool facing = l > 0.0f;
        const float inten = fminf(fmaxf(0.0f, l) + 0.4f + (facing ? 0.15f : 0.0f), 1.0f);
        c = make_float3(col.x * inten * m[0], col.y * inten * m[1], col.z * inten * m[2]);
        bool dark = false;
        if ((bn.n & ~kBent) == 0) {  // (not reflected)
            if (!facing) {
                dark = true;
            } else {
                // shadow ray towards the sun from the centre of lastPos, through empty and liquid
                const float so[3] = {(float)(h.x - (ax == 0u ? sg : 0)) + 0.5f, (float)(h.y - (ax == 1u ? sg : 0)) + 0.5f,
                                     (float)(h.z - (ax == 2u ? sg : 0)) + 0.5f};
                // (DIRS: a sign octant every shadow ray of the launch steps with; shading launches pass 0 — their instances are
                // specialised on the camera's octant instead, k_cast)
                // the reference's sun, normalize(2, 1, 4) (globals.cpp:23; uniform), steps + on every axis: its octant is
                // compiled into a second copy of the shadow trace (shaded C3 -3.0 %, profiles/r06/ab_sun_octant_shadows.txt);
                // any other sun takes per-wave sign flags
                constexpr uint32_t SHADOW = T_ESCAPE | T_CEIL_SHADOW;
                constexpr int kSunAllPlus = 1;  // (frame_dirs' code of the octant + + +)
                if (DIRS == 0 && P.sun_dirs == kSunAllPlus)
                    dark = (trace<SHADOW | t_dirs(kSunAllPlus)>(P, smem, P.smats, path, so, P.sun, P.shadow_steps, nullptr, nullptr, nullptr,
                                                                P.top_solid).info & HIT_BIT) != 0u;
                else
                    dark = (trace<SHADOW | t_dirs(DIRS)>(P, smem, P.smats, path, so, P.sun, P.shadow_steps, nullptr, nullptr, nullptr,
                                                         P.top_solid).info & HIT_BIT) != 0u;
            }
        }
        if (dark) c = make_float3(col.x * 0.3f * m[0], col.y * 0.3f * m[1], col.z * 0.3f * m[2]);
    }
    P.rgba[out] = make_float4(c.x, c.y, c.z, 0.0f);
}
