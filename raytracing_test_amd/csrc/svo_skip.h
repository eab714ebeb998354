// svo_skip.h — the closed-form crossing of an empty box (skip_box): the per-axis crossing counts (count_est), the exact
// segments of rays that are not linear (lsb_exp, seg_cap) and the lane-mask selects they use.  The proof is the note
// at the head of svo_exact.h.  Used by trace() in svo_trace.h, for the forward boxes, the ceiling boxes and the march.
#pragma once

#include <algorithm>

#include "svo_exact.h"

// #{ j >= 0 : T + j*a < V } or #{ j >= 0 : T + j*a <= V } = m + [E < V] or m + [E <= V] with
// E = T + m*a and the estimate m = floor((V-T)/a + 1/2) (for <=, the count is floor(x) + 1 with
// x = (V-T)/a, and m is that or one less)
// per-lane selects and a carry-in add on a wave mask held in SGPRs
__device__ __forceinline__ uint32_t sel32(uint64_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %2, %1, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
__device__ __forceinline__ double sel64(uint64_t m, double a, double b) {
    const uint64_t ua = (uint64_t)__double_as_longlong(a), ub = (uint64_t)__double_as_longlong(b);
    const uint32_t lo = sel32(m, (uint32_t)ua, (uint32_t)ub), hi = sel32(m, (uint32_t)(ua >> 32), (uint32_t)(ub >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ int32_t add_bit(int32_t x, uint64_t m) {
    int32_t r;
    uint64_t co;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(co) : "v"(x), "s"(m));
    return r;
}
// The difference V - T is taken in f32 from f32 copies of both (one conversion of V serves the three
// axes; V < 2^121 by span_ok, so its copy is finite, and a T beyond the f32 range only makes the
// estimate 0, its count): T / a and V / a stay below budget + 2 < 2^20 + 2 (V is at most T + steps * a on every axis),
// so the two conversions, the subtraction, the 1-ulp reciprocal and the fma move the estimate by less
// than 6 * 2^20 * 2^-24 = 3/8 < 1/2 — m stays c - 1 or c
// V, or nextup(V) on the lanes of m (V >= 0 and finite: the bits plus one)
__device__ __forceinline__ double next_if(double V, uint64_t m) {
    const uint64_t b = (uint64_t)__double_as_longlong(V);
    uint32_t lo, hi;
    uint64_t c, c2;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(lo), "=s"(c) : "v"((uint32_t)b), "s"(m));
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(hi), "=s"(c2) : "v"((uint32_t)(b >> 32)), "s"(c));
    (void)c2;
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ int32_t count_est(double T, double a, float inva, double V, float Vf, double& E) {
    uint32_t mu;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(mu) : "v"(__builtin_fmaf(Vf - (float)T, inva, 0.5f)));
    E = on_grid(T, (int32_t)mu, a);
    return (int32_t)mu;
}

// Exact segments.  From any state (T, a), the crossings T + i*a are multiples of 2^v, v = the lower
// of the lowest set bits of T and a, so every crossing below B = 2^(v+53) is exact and representable,
// and the first one at or above B is that sum rounded once, as fma(i, a, T) computes it too.  B is at
// least 2^(e+1) (e = the binade of |T|: T is a multiple of ulp(T), and a of 2^(ea-23) > ulp(T) as
// |T| < 2^(ea+22)); for a ray from a non-integral origin it is typically hundreds of crossings away,
// and past it each binade the crossings enter costs one rounding.  seg_cap returns an index of a
// crossing below B (at most the last one): the crossings 0 .. seg_cap + 1 are fma-exact.
// lowest set bit exponent of |T| (zero: none, 2^20; subnormal: -1074, a safe underestimate)
// (not svo_exact.h's dbl_lsb, which answers 2^20 for subnormals: merging the two would change the segment instances)
__device__ __forceinline__ int32_t lsb_exp(double T) {
    const uint64_t b = (uint64_t)__double_as_longlong(T);
    const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    const int32_t e = (int32_t)((hi >> 20) & 0x7FFu);
    const int32_t tz = lo ? (int32_t)__builtin_ctz(lo) : 32 + (int32_t)__builtin_ctz((hi & 0xFFFFFu) | 0x100000u);
    return e != 0 ? e - 1075 + tz : ((b << 1) == 0ull ? (1 << 20) : -1074);
}
// A ray is linear, by a cheap sufficient test on its origin, when every coordinate is integral or
// half-integral: dda_axis then starts at T = a, 0, a/2, 3a/2 or -a/2 (a multiple of half of a's
// lowest set bit, 2^(la-1)), and with a budget below 2^20 every sum stays below 2^(la-1+53) — the
// camera positions of integral poses, and the cell centres shadow and AO rays start from.
__device__ __forceinline__ bool lin_origin(float o) {
    const float o2 = o + o;
    return o2 == __builtin_truncf(o2) && __builtin_fabsf(o) < 1073741824.0f;
}

// x = (B - T)/a is estimated as x~ within 2^-22 relative (f32 roundings, the 1-ulp reciprocal), so
// floor(x~ * (1 - 2^-20)) < x: at most the count of crossings below B, less one (almost always equal)
__device__ __forceinline__ int32_t seg_cap(double T, float af, float inva) {
    const uint32_t ab = __float_as_uint(af);
    const int32_t la = (int32_t)((ab >> 23) & 0xFFu) - 150 + (int32_t)__builtin_ctz(ab | 0x800000u);  // a: normal
    const int32_t be = min(max(min(lsb_exp(T), la) + 53 + 1023, 1), 0x7FF);  // biased exponent of B (0x7FF: inf)
    const double B = __longlong_as_double((long long)((uint64_t)(uint32_t)(be << 20) << 32));
    uint32_t c;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(c) : "v"((float)(B - T) * inva * 0.99999905f));  // saturates (inf: 2^32 - 1)
    return (int32_t)min(c, 1u << 30);  // (never negative: every skip takes at least its exit step)
}

// Cross an empty box, branch-free over the exit axis: ex[k] = steps along axis k that leave the box,
// less one.  Returns false (state unchanged) when the budget ends inside the box.  seg (wave-uniform:
// the wave holds rays that are not linear): each axis' exit event is also held to its exact segment (seg_cap); an exit on such a
// bound is a virtual one inside the box (the next lookup finds the same empty cell in the parent's
// mask, without a load, and the crossing continues).
// RB: segment bounds cached as cells (R.rb): crossing i of axis k from the current state is the one
// into cell r + s*i, so the bound seg_cap gave at some earlier state stays s*(rb - r) crossings ahead
// while the ray has not passed it (every sum up to there is exact, from any state on the way); a
// negative count means it has, and seg_cap is taken again from the current state
template <bool TRACK = true, bool RB = false>
__device__ __forceinline__ bool skip_box(Ray& R, const int32_t ex[3], bool seg) {
    // exits beyond the budget are clamped (safe: total > steps)
    int32_t e[3];
#pragma unroll
    for (int k = 0; k < 3; k++) e[k] = min(ex[k], R.steps);
    if (seg && RB) {  // wave-uniform
        int32_t cap[3];
#pragma unroll
        for (int k = 0; k < 3; k++)  // (wrapping differences: |cap| < 2^31)
            cap[k] = (int32_t)(R.s[k] > 0 ? (uint32_t)R.rb[k] - (uint32_t)R.r[k] : (uint32_t)R.r[k] - (uint32_t)R.rb[k]);
        if (__ballot(min(min(cap[0], cap[1]), cap[2]) < 0) != 0ull) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (cap[k] < 0) {
                    cap[k] = seg_cap(R.T[k], R.af[k], R.inv_a(k));
                    R.rb[k] = (int32_t)(R.s[k] > 0 ? (uint32_t)R.r[k] + (uint32_t)cap[k] : (uint32_t)R.r[k] - (uint32_t)cap[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = min(e[k], cap[k]);
    } else if (seg) {  // wave-uniform
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = min(e[k], seg_cap(R.T[k], R.af[k], R.inv_a(k)));
    }
    double E[3];
#pragma unroll
    for (int k = 0; k < 3; k++) E[k] = on_grid(R.T[k], e[k], R.a(k));
    // lexicographic minimum of (E, rank) with rank z < y < x (the DDA rule applied to exits)
    // exit flags as lane masks (SGPRs): selects and tie terms read them directly
    // (ballots of single compares are the compare masks themselves)
    const uint64_t mx = __ballot(E[0] < E[1]) & __ballot(E[0] < E[2]);
    const uint64_t my = __ballot(E[1] < E[2]) & ~mx;
    const double V = sel64(mx, E[0], sel64(my, E[1], E[2]));
    // Events of another axis k that precede the exit event: T + j*a < V when k loses ties
    // (rank_k > rank_b, i.e. k < b), else T + j*a <= V, which on doubles is < nextup(V).
    // strict: x only when the exit is on y or z, y only when it is on z, z never.  On the exit
    // axis b, E = V exactly (V is its e_b-th crossing, m = e_b): there the tie term is the flag b_b
    // itself, so x and y need no second compare of their own for it.
    int32_t n[3];
    double F[3];
    const float Vf = (float)V;
    n[0] = count_est(R.T[0], R.a(0), R.inv_a(0), V, Vf, F[0]);
    n[1] = count_est(R.T[1], R.a(1), R.inv_a(1), V, Vf, F[1]);
    n[2] = count_est(R.T[2], R.a(2), R.inv_a(2), V, Vf, F[2]);
    // (the terms of one axis are disjoint: a tie term implies F = V)
    n[0] = add_bit(n[0], __ballot(F[0] < V) | mx);
    // y's tie term: exit on x counts y's events <= V, i.e. < nextup(V) (V >= 0 finite: its bits + 1),
    // taken by one integer add with the carry-in on mx instead of a second f64 compare
    n[1] = add_bit(n[1], __ballot(F[1] < next_if(V, mx)) | my);
    n[2] = add_bit(n[2], __ballot(F[2] <= V));
    const int32_t total = n[0] + n[1] + n[2];
    if (total > R.steps) return false;  // (a wrong count cannot hang the launch either: trace's progress guard)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        R.T[k] = on_grid(R.T[k], n[k], R.a(k));
        // a compile-time step (sign octant instances) adds or subtracts; else a 24-bit multiply-add
        // (full rate; s = +-1, |n| < 2^21)
        R.r[k] += __builtin_constant_p(R.s[k]) ? (R.s[k] > 0 ? n[k] : -n[k]) : __mul24(R.s[k], n[k]);
    }
    if (TRACK) R.tlast = V;  // (else recovered at the end of the ray: trace)
    R.axis = sel32(mx, 0u, sel32(my, 1u, 2u));
    R.steps -= total;
    return true;
}
