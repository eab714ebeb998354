// svo_exact.h — the exact arithmetic of one ray's DDA: the note on exact closed-form skipping, the tests for the rays it
// covers (axis_ok, exact_axis, span_ok), the ray's state (Ray), its voxel step (dda_step) and the wave's step-sign flags.
// Used by svo_skip.h (the crossing built on it), svo_lookup.h, svo_brick.h, svo_ceil_march.h and trace() in svo_trace.h.
#pragma once

#include "svo_cast_params.h"

// ------------------------------------------------------------------------------------------------
// Exact closed-form skipping.  castRayFromCam's axis choice (ray_caster.cpp:71-80) is, for non-NaN
// values, the lexicographic minimum of (T_axis, rank) with rank z < y < x: x wins only when
// strictly smallest, y beats z only when strictly smaller.  Each axis' crossings form the sequence
// T, fl(T+a), fl(fl(T+a)+a), ... (deltaPos += absDelta in double).  absDelta is an f32 value
// widened to f64: 24 significant bits, a multiple of 2^(ea-23).
//  * Linear rays: when every partial sum a ray can reach (<= budget+2 terms) stays below
//    2^(lsb+53) — lsb = lowest set bit of T and a — every sum is exact and T + k*a computed directly
//    equals the k-fold accumulation bit for bit (e.g. always from integral camera positions).
//  * Every other ray (budget < 2^20, finite values): |T| stays below 2^(ea+22), so a is a multiple
//    of ulp(T) and every crossing below B = 2^(e+1) (e = the binade of |T|) is an exact,
//    representable multiple of ulp(T); the first crossing at or above B is that exact sum rounded
//    once, which fma(k, a, T) also computes.  Only later crossings (one more rounding per binade
//    entered) drift from the closed form, so the crossings are exact segment by segment
//    (seg_cap), and an empty region is crossed in a few moves (skip_box with seg).
// A ray crosses an empty region in O(1): the first event to leave the region is the lexicographic
// minimum of the three per-axis exit events, and the events before it on the other axes are
// counted by division (with an exact fix-up).  Rays outside both domains step voxel by voxel
// (still without memory traffic inside known-empty regions).  All paths give identical results
// (tests).
// ------------------------------------------------------------------------------------------------
// lowest set bit (power of two) of |x|: x finite and nonzero; denormals -> 1 << 20 ("not fast")
// (svo_skip.h's lsb_exp looks like a duplicate but answers -1074 for subnormals: the two stay apart)
__device__ __forceinline__ int dbl_lsb(uint32_t hi, uint32_t lo) {
    const int e = (int)((hi >> 20) & 0x7FFu);
    const uint32_t mh = (hi & 0xFFFFFu) | 0x100000u;  // hidden bit
    const int tz = lo ? (int)__builtin_ctz(lo) : 32 + (int)__builtin_ctz(mh);
    return e == 0 ? (1 << 20) : e - 1075 + tz;
}

// a: positive, normal, finite; T: finite (the closed forms' domain)
__device__ __forceinline__ bool axis_ok(double T, double a) {
    const uint32_t th = (uint32_t)((uint64_t)__double_as_longlong(T) >> 32) & 0x7FFFFFFFu;
    const uint32_t ah = (uint32_t)((uint64_t)__double_as_longlong(a) >> 32);
    const uint32_t et = th >> 20, ea = (ah >> 20) & 0x7FFu;
    return ((unsigned)((ah >> 31) == 0u) & (unsigned)(ea - 1u < 0x7FEu) & (unsigned)(et != 0x7FFu)) != 0u;  // (branch-free)
}

// every partial sum exact ("linear" axis: no rounding at all); axis_ok(T, a) holds
__device__ __forceinline__ bool exact_axis(double T, double a, int32_t budget) {
    const uint32_t th = (uint32_t)((uint64_t)__double_as_longlong(T) >> 32) & 0x7FFFFFFFu, tl = (uint32_t)__double_as_longlong(T);
    const uint32_t ah = (uint32_t)((uint64_t)__double_as_longlong(a) >> 32), al = (uint32_t)__double_as_longlong(a);
    const int u = (th | tl) ? min(dbl_lsb(th, tl), dbl_lsb(ah, al)) : dbl_lsb(ah, al);
    const double bound = __builtin_fabs(T) + (double)(budget + 2) * a;
    const int eb = (int)((uint32_t)((uint64_t)__double_as_longlong(bound) >> 52) & 0x7FFu) - 1023;
    return eb + 1 <= u + 52;  // bound < 2^(u+52): the unrounded bound < 2^(u+53)
}

struct Ray {
    int32_t r[3];   // current voxel (unwrapped)
    double T[3];    // next crossing per axis (deltaPos)
    float af[3];    // absDelta: an f32 value widened to f64 by the reference (ray_caster.cpp:35-41)
    int32_t s[3];   // step
    int32_t steps;  // budget left
    uint32_t axis;  // axis of the last step (3: none)
    double tlast;   // crossing value of the last step (converted to the f32 output once, at the end)
    float ia[3];    // f32 estimate of 1/absDelta (crossing counts only estimate with it)
    int32_t rb[3];  // segment-cached instances (skip_box RB): the cell of each axis' last exact crossing
    __device__ __forceinline__ float inv_a(int k) const { return ia[k]; }
    __device__ __forceinline__ double a(int k) const { return (double)af[k]; }
};

// T + k*a for a fast ray: exact (exact_axis), so one fused operation gives the same double
__device__ __forceinline__ double on_grid(double T, int32_t k, double a) {
    return __builtin_fma((double)k, a, T);
}

// The f32 count estimates (count_est) need every exit event V in f32 range: V is at most the
// smallest absDelta times budget + 2 (< 2^21), so a ray whose every absDelta is 2^100 or more (a
// direction vector with every component below 2^-100) takes the stepping path.  (Frame rays have unit
// directions: their smallest absDelta is at most sqrt(3).)
__device__ __forceinline__ bool span_ok(const Ray& R) {
    return __builtin_fminf(__builtin_fminf(R.af[0], R.af[1]), R.af[2]) < 0x1p100f;
}

// one DDA step (ray_caster.cpp:70-80), branch-free
__device__ __forceinline__ void dda_step(Ray& R) {
    const bool cx = (R.T[0] < R.T[1]) && (R.T[0] < R.T[2]);
    const bool cy = !cx && (R.T[1] < R.T[2]);
    const bool cz = !cx && !cy;
    R.tlast = cx ? R.T[0] : (cy ? R.T[1] : R.T[2]);
    R.axis = cx ? 0u : (cy ? 1u : 2u);
    R.r[0] += cx ? R.s[0] : 0;
    R.r[1] += cy ? R.s[1] : 0;
    R.r[2] += cz ? R.s[2] : 0;
    R.T[0] = cx ? R.T[0] + R.a(0) : R.T[0];
    R.T[1] = cy ? R.T[1] + R.a(1) : R.T[1];
    R.T[2] = cz ? R.T[2] + R.a(2) : R.T[2];
    R.steps--;
}

// Wave-uniform step directions per axis: 1 = every active lane steps +, 2 = every one steps -,
// 0 = mixed.  Lanes only retire while a ray runs, so flags taken at its start stay true.
__device__ __forceinline__ void dir_flags(const int32_t s[3], uint32_t ud[3]) {
    const uint64_t ex = __builtin_amdgcn_read_exec();
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t b = __ballot(s[k] > 0);
        ud[k] = b == ex ? 1u : (b == 0ull ? 2u : 0u);
    }
}

// r + n or r - n by the step sign s; ud: wave-uniform sign (dir_flags) or 0
__device__ __forceinline__ int32_t step_by(int32_t r, int32_t n, int32_t s, uint32_t ud) {
    if (ud == 1u) return r + n;
    if (ud == 2u) return r - n;
    return s > 0 ? r + n : r - n;  // (s * n as a 24-bit multiply-add became v_mad_u64_u32)
}
