// svo_trace.h — device code of one ray: the exact closed-form skipping, the region lookup, the brick walk, the
// column-ceiling march and trace() itself (the semantics are in svo_cast_kernel.h's header note).
#pragma once

#include <algorithm>

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

struct Stats {
    uint32_t lookups, loads, skips, skip_out, brick_steps, plain_steps;
    uint32_t skip_by_sh[4];  // crossings whose box is made of 2^sh cells: sh = 2, 4, 6, >= 8
    uint32_t bricks;         // brick visits
    uint32_t wv_iters, wv_brick;  // wave-level executions (counted on the first active lane): outer
                                  // loop iterations, brick voxel steps
    uint32_t root_starts, cache_empty;  // lookups started at the root; lookups answered by the
                                        // parent mask
    uint32_t path_starts;                          // lookups restarted from the LDS path
    uint32_t wv_skips, wv_descents;                // wave-level crossings, descent levels
    uint32_t no_progress;                          // loop iterations that consumed no budget (the guard's trips: 0)
    uint32_t ceil_moves;                           // crossings of a column-ceiling box (no lookup)
    uint32_t iters;                                // this lane's traversal iterations
    uint32_t above_top;                            // iterations that start above the tree's highest stored row
    uint32_t bends;                                // reflections and refractions (shading)
    uint32_t tints, tint_iters;                    // refractive voxels passed; iterations that ended passing one
};

// true on one lane of the active lanes (wave-level counters)
__device__ __forceinline__ bool wave_lead() {
    return (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
}

// wave-wide max / sum (diagnostics only)
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// Region lookup of a wrapped voxel: SOLID hit, an empty child cell (returns its shift), or the
// brick holding the voxel (mask / ref / info returned).  tetrahexa_tree.cpp:124-152 on the
// breadth-first layout.
enum : uint32_t { R_EMPTY = 0u, R_BRICK = 1u, R_SOLID = 2u, R_CEIL = 3u };
// Hit.info of a shading ray that left the loop early (ESCAPE): a miss whose remaining steps are all in empty voxels
// (never written to a hit record: escaping is off when records are requested)
constexpr uint32_t ESC_BIT = 1u << 19;

// The interior node whose child region holds the ray's current cell, kept in registers: a move to
// a sibling region reads the cached child mask (no load when the sibling is empty) and restarts
// the descent at most one level down; leaving the parent's region restarts at the root, whose top
// levels are staged in LDS.
// per-lane path of the last descent in LDS
struct Path {
    // [depth][mask low, mask high, first child][lane] dwords: one address per depth (the three
    // words at +0, +256, +512 bytes: ds_write2st64 / ds_read2st64 and one more)
    uint32_t* __restrict__ w;
    __device__ __forceinline__ void put(int32_t d, uint64_t mask, uint32_t ref) const {
        uint32_t* e = w + d * (3 * kBlock);
        e[0] = (uint32_t)mask;
        e[kBlock] = (uint32_t)(mask >> 32);
        e[2 * kBlock] = ref;
    }
    __device__ __forceinline__ uint64_t mask(int32_t d) const {
        const uint32_t* e = w + d * (3 * kBlock);
        return (uint64_t)e[0] | ((uint64_t)e[kBlock] << 32);
    }
    __device__ __forceinline__ uint32_t ref(int32_t d) const { return w[d * (3 * kBlock) + 2 * kBlock]; }
};

struct Parent {
    uint64_t mask;
    uint32_t ref;
    uint32_t sh;  // child shift: a child region is 2^sh voxels wide, the parent's 2^(sh+2)
};

// Node reads.  Trees of up to kNarrowNodes nodes (4 GiB) read through a buffer resource with 32-bit
// byte offsets (one shift per load, and buffer loads are never merged with the LDS path); larger
// trees — the builders accept up to 2^32 nodes, 64 GiB — through 64-bit global addresses.  The host
// picks the instance per tree (svo_cast.hip: node_addressing), so no index can wrap or fall outside
// the resource and read zeros (an empty node) silently.
// Loads take "one past" indices: ni1 = node index + 1 = first child + rank + 1, which is the popcount
// of the child mask shifted so the child's own bit stays in (slot_top: no further shift), and the
// bases sit one node before the array.
constexpr uint64_t kNarrowNodes = 1ull << 28;  // below it, ni1 << 4 stays below 2^32

struct BufNodes {
    __amdgpu_buffer_rsrc_t rsrc;
    const Node* __restrict__ base;
    __device__ __forceinline__ explicit BufNodes(const Node* p)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<Node*>(p - 1), (short)0, (int)0xFFFFFFFFu, (int)0x00020000)), base(p) {}
    __device__ __forceinline__ Node root() const { return base[0]; }  // (uniform: a scalar load)
    __device__ __forceinline__ Node load(uint32_t ni) const {  // node ni - 1
        const uint32_t off = ni << 4;
        Node n;
        n.mask = ((uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0)) |
                 ((uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4, 0, 0) << 32);
        n.ref = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 8, 0, 0);
        n.info = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 12, 0, 0);
        return n;
    }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct WideNodes {
    const __attribute__((address_space(1))) u32x4* p;
    const Node* __restrict__ base;
    __device__ __forceinline__ explicit WideNodes(const Node* q) : p((const __attribute__((address_space(1))) u32x4*)(q - 1)), base(q) {}
    __device__ __forceinline__ Node root() const { return base[0]; }  // (uniform: a scalar load)
    __device__ __forceinline__ Node load(uint32_t ni) const {  // node ni - 1
        const u32x4 v = p[ni];  // 64-bit address: base + (u64)ni * 16
        Node n;
        n.mask = (uint64_t)v.x | ((uint64_t)v.y << 32);
        n.ref = v.z;
        n.info = v.w;
        return n;
    }
};

// lookup()'s compile-time options, one word (lookup<OPT>)
enum : uint32_t {
    L_STATS = 1u << 0,  // count into st (diagnostics)
    // the levels above the bricks hold interior nodes or SOLID regions only; a SOLID region ends the ray, so the parent
    // may be overwritten by it, and those levels need no leaf branch and no copies of the loaded node (the shading
    // pass, whose callers read the final parent's regions, keeps the general loop)
    L_SPLIT = 1u << 1,
    // (AO instances: ao_count_plan reads the final parent's shift only) a SOLID region above the bricks leaves the shift
    // of its own parent, so no path entry at or below the SOLID node is read back
    L_PSH = 1u << 2,
};
template <uint32_t OPT, class Mem>
__device__ __forceinline__ uint32_t lookup(const CastParams& P, const Mem& mem, const Path& path,
                                           const uint32_t w[3], uint32_t moved, Parent& par, uint32_t& sh_out, uint64_t& bmask,
                                           uint32_t& bref, uint32_t& binfo, Stats& st) {
    static_assert((OPT & ~(L_STATS | L_SPLIT | L_PSH)) == 0u, "lookup: unknown option");
    constexpr bool STATS = (OPT & L_STATS) != 0u, SPLIT = (OPT & L_SPLIT) != 0u, PSH = (OPT & L_PSH) != 0u;
    uint32_t ni = 0u;
    int32_t dd = 0;
    if (STATS) st.lookups++;
    {
        // the previous voxel lies in the parent's region (every move starts inside it), so the
        // bits in which the last step changed the stepped coordinate tell whether the ray left it
        const uint32_t diff = moved;
        if (diff >= (4u << par.sh)) {  // a bit at or above the parent region's size changed
            // left the parent's region: the deepest node of the last descent whose region also
            // holds this cell (depth levels-1-floor(h/2), h = highest differing bit) becomes the
            // parent, read back from the per-lane path in LDS
            const int32_t da = P.levels - 1 - (int32_t)((31u - (uint32_t)__builtin_clz(diff)) >> 1);  // (diff != 0)
            par.mask = path.mask(da);
            par.ref = path.ref(da);
            par.sh = (uint32_t)(2 * (P.levels - 1 - da));
            if (STATS) st.path_starts++;
        }
        sh_out = par.sh;
        const uint64_t t = slot_top(par.mask, child_slot(w[0], w[1], w[2], par.sh));
        if ((int64_t)t >= 0) {
            if (STATS) st.cache_empty++;
            return R_EMPTY;
        }
        ni = popc_add(t, par.ref);  // (one past: BufNodes)
        dd = P.levels - (int32_t)(par.sh >> 1);  // depth of that child
        if (STATS && dd == 0) st.root_starts++;
    }
    // descend (one exit: no per-exit register copies)
    uint32_t res = R_EMPTY;
    if (SPLIT) {
        // Node ni - 1 occupies the cell and is not loaded yet.  Across the back-edge go ni, dd and one flag: dd counts
        // only the levels whose child is pending (occupied, under an interior node), so a lane leaves the loop with
        // dd == levels - 1 exactly when its brick-level node is pending (also a lane that starts there), and the
        // other lanes' outcome is read after the loop from the last node they loaded (binfo; par.sh is its shift).
        const int32_t dl = P.levels - 1;
        bool more = dd < dl;
        while (more) {
            if (STATS) {
                st.wv_descents += wave_lead();
                st.loads++;
            }
            const Node n = mem.load(ni);
            const uint32_t sh = (uint32_t)(2 * (dl - dd));
            path.put(dd, n.mask, n.ref);
            par.mask = n.mask;
            par.ref = n.ref;
            binfo = n.info;
            const uint64_t t = slot_top(n.mask, child_slot(w[0], w[1], w[2], sh));
            const bool solid = (n.info & K_KIND_MASK) == K_SOLID;
            par.sh = PSH && solid ? sh + 2u : sh;
            ni = popc_add(t, n.ref);
            const bool pend = (int64_t)t < 0 && !solid;
            dd += pend ? 1 : 0;
            more = pend && dd < dl;
        }
        // ended above the bricks: a SOLID region, or an empty child cell of the last node (shift par.sh; sh_out is read
        // for R_EMPTY only).  (Taken on every lane: the brick level's lanes overwrite it.)
        sh_out = par.sh;
        res = (binfo & K_KIND_MASK) == K_SOLID ? R_SOLID : R_EMPTY;
        if (dd == dl) {  // the brick level: a BRICK or SOLID leaf
            if (STATS) {
                st.wv_descents += wave_lead();
                st.loads++;
            }
            const Node n = mem.load(ni);
            bmask = n.mask;
            bref = n.ref;
            binfo = n.info;
            sh_out = 2u;
            res = (n.info & K_KIND_MASK) == K_SOLID ? R_SOLID : R_BRICK;
        }
        return res;
    }
    bool more = dd < P.levels;
    while (more) {
        if (STATS) {
            st.wv_descents += wave_lead();
            st.loads++;
        }
        const Node n = mem.load(ni);
        const uint32_t kind = n.info & K_KIND_MASK;
        // (read only for BRICK / SOLID results: written on every load, so the previous values need
        // no copies around it)
        bmask = n.mask;
        bref = n.ref;
        binfo = n.info;
        if (kind == K_INTERIOR) {
            const uint32_t sh = (uint32_t)(2 * (P.levels - 1 - dd));
            path.put(dd, n.mask, n.ref);
            par.mask = n.mask;
            par.ref = n.ref;
            par.sh = sh;
            const uint64_t t = slot_top(n.mask, child_slot(w[0], w[1], w[2], sh));
            const bool occ = (int64_t)t < 0;
            ni = popc_add(t, n.ref);
            dd++;
            more = occ && dd < P.levels;
            sh_out = occ ? 0u : sh;  // (occupied at the last level only in a malformed tree: one voxel)
        } else {
            sh_out = 2u;
            res = kind == K_SOLID ? R_SOLID : R_BRICK;
            more = false;
        }
    }
    return res;
}

__device__ __forceinline__ uint32_t brick_material(const uint16_t* mats, uint64_t mask, uint32_t ref, uint32_t info, uint32_t v) {
    return (info & K_UNIFORM) ? (info >> 16) : (uint32_t)mats[ref + (uint32_t)__popcll(mask & ((1ull << v) - 1ull))];
}

__device__ __forceinline__ void wrap3(const Ray& R, uint32_t wm, uint32_t w[3]) {
    w[0] = (uint32_t)R.r[0] & wm;
    w[1] = (uint32_t)R.r[1] & wm;
    w[2] = (uint32_t)R.r[2] & wm;
}

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

// Column-ceiling march (round 5).  A descending ray above the ceiling of its 16-column block crosses, cell by cell,
// only empty voxels until its row reaches that ceiling or it leaves the block; castRayFromCam's DDA (ray_caster.cpp:71-80)
// takes its x / z / y steps at the crossing values T_k + j * a_k, so every event that matters here is one fma of an
// integer index: the x (z) event entering the next block, j = the cells left in the block on that axis, and the y event
// entering the ceiling row c, j = y - 1 - c.  The march walks the blocks the ray's column path crosses (their order
// follows from the x / z boundary events alone) comparing exact event values, one 32-bit ceiling load per block (the
// next block's load issued before this one is judged), until the ceiling event comes first or the ray enters a block
// at or below its ceiling; every voxel entered before that event is then empty, and one closed-form crossing
// (skip_box) moves the ray to the state right after it — the cell that event enters is the loop's next untested
// voxel.  This replaces the chain of per-block ceiling moves of a ray's descent (C3: ~6 of its ~11 loop iterations,
// each a full iteration with its own exact crossing) by one crossing and a few integer / fma steps per block.
// Linear rays only (every sum exact: `fast` in the non-segment instances), stepping down (R.s[1] < 0); a tie between
// the x and z boundary events (a block corner) or between a boundary and the ceiling event stops the march there.
// Returns whether the ray moved.
// The march's end: ex (skip_box's exits) of the first event whose voxel it could not prove empty.  Returns false when
// nothing beyond the current voxel is proven (its own row is at or below its block's ceiling).
template <bool STATS>
__device__ __forceinline__ bool ceil_march(const CastParams& P, const uint32_t* __restrict__ ceilp, const Ray& R, uint32_t wm, int32_t ex[3],
                                           Stats& st) {
    const uint32_t lsh = P.ceil_sh[0];  // the finest level's blocks: 2^lsh columns
    const uint32_t bm = (1u << lsh) - 1u, rows = (wm + 1u) >> lsh, rm = rows - 1u;
    const int32_t wy = (int32_t)((uint32_t)R.r[1] & wm);
    const uint32_t wx = (uint32_t)R.r[0] & wm, wz = (uint32_t)R.r[2] & wm;
    // per axis the next block-boundary event: its index from the current state (the cells left in the block) and value
    int32_t jx = (int32_t)(R.s[0] > 0 ? bm - (wx & bm) : (wx & bm)), jz = (int32_t)(R.s[2] > 0 ? bm - (wz & bm) : (wz & bm));
    double Ex = on_grid(R.T[0], jx, R.a(0)), Ez = on_grid(R.T[2], jz, R.a(2));
    uint32_t bx = wx >> lsh, bz = wz >> lsh;
    const uint32_t dx = R.s[0] > 0 ? 1u : rm, dz = R.s[2] > 0 ? 1u : rm;  // (one block on, wrapped)
    uint32_t cv = ceilp[__umul24(bz, rows) + bx];
    double Ein = -__builtin_inf();  // the event that entered the current block (none for the first)
    int32_t ein_axis = -1, ein_j = 0, stop_axis = -1, stop_j = 0;
    for (int32_t it = 0;; it++) {
        const bool xn = Ex < Ez;
        // the next block's ceiling, loaded before this block is judged (the blocks' order follows from x / z alone)
        const uint32_t nbx = xn ? (bx + dx) & rm : bx, nbz = xn ? bz : (bz + dz) & rm;
        const uint32_t ncv = ceilp[__umul24(nbz, rows) + nbx];
        const int32_t jy = wy - 1 - (int32_t)(int16_t)(cv & 0xFFFFu);  // the y event entering the ceiling row
        const double tc = jy >= 0 ? on_grid(R.T[1], jy, R.a(1)) : -__builtin_inf();
        if (!(tc > Ein) || it == 1024) {  // the voxel entering this block is at or below its ceiling: end before that event
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
        if (STATS) st.ceil_moves++;
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
    // (selects on values: a dynamically indexed register array would go through scratch)
    ex[0] = stop_axis == 0 ? stop_j : R.steps;
    ex[1] = stop_axis == 1 ? stop_j : R.steps;
    ex[2] = stop_axis == 2 ? stop_j : R.steps;
    return stop_axis >= 0;
}

// A shading ray's DDA state on entering the first block it hits (the cell, crossing values, budget and last step axis):
// the straight trace before any bounce hands it to the reflection / refraction trace, which resumes from it (trace: T_XS_SAVE / T_XS_RESUME)
struct RayState {
    double T[3];
    int32_t r[3];
    int32_t steps;
    uint32_t axis;
};

// Reflections and refractions of the shading pass (reflectRay / refractRay, low_res.frag:170-240):
// direction after them, reflection count, finalColorMod (a vec3: liquid tints per channel), and
// whether the ray was bent (kBent, a bit of the reflection count's word: 28 B per lane in LDS, which with the launch's own
// path depth lets the shading instances run 7 waves per SIMD).
constexpr int32_t kBent = 1 << 30;
struct Bounce {
    float d[3];
    int32_t n;  // reflections | kBent
    float m[3];
};

// refractRay(vec3, vec3, float, float) (low_res.frag:196-209), n1 = 1.0, n2 = 1.1; dot as
// ((x + y) + z), no fused operations (-ffp-contract=off)
__device__ __forceinline__ void refract_dir(float d[3], const float nin[3]) {
    const float r = 1.0f / 1.1f;
    float n[3] = {nin[0], nin[1], nin[2]};
    float c1 = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    if (c1 < 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = -n[k];
        c1 = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    }
    const float c2 = svo::sqrt_rn(1.0f - r * r * (1.0f - c1 * c1));
    const float kf = r * c1 - c2;
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = r * d[k] + kf * n[k];
}

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
        if (ceil_march<STATS>(P, ceilp, R, wm, ex, st)) (void)skip_box<TRACK, RB>(R, ex, wseg);
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
            atomicAdd(P.stats + 7, (unsigned long long)wsum);
            atomicAdd(P.stats + 8, (unsigned long long)wmax * 64ull);
        }
        atomicAdd(P.stats + 0, 1ull);
        atomicAdd(P.stats + 1, (unsigned long long)st.lookups);
        atomicAdd(P.stats + 2, (unsigned long long)st.loads);
        atomicAdd(P.stats + 3, (unsigned long long)st.skips);
        atomicAdd(P.stats + 4, (unsigned long long)st.skip_out);
        atomicAdd(P.stats + 5, (unsigned long long)st.brick_steps);
        atomicAdd(P.stats + 6, (unsigned long long)st.plain_steps);
        for (int k = 0; k < 4; k++) atomicAdd(P.stats + 9 + k, (unsigned long long)st.skip_by_sh[k]);
        atomicAdd(P.stats + 13, (unsigned long long)st.bricks);
        atomicAdd(P.stats + 14, (unsigned long long)st.wv_iters);
        atomicAdd(P.stats + 15, (unsigned long long)st.wv_brick);
        atomicAdd(P.stats + 17, (unsigned long long)st.root_starts);
        atomicAdd(P.stats + 18, (unsigned long long)st.cache_empty);
        atomicAdd(P.stats + 19, (unsigned long long)st.wv_skips);
        atomicAdd(P.stats + 20, (unsigned long long)st.wv_descents);
        atomicAdd(P.stats + 21, (unsigned long long)st.path_starts);
        if (st.no_progress) atomicAdd(P.stats + 16, (unsigned long long)st.no_progress);
        atomicAdd(P.stats + 23, (unsigned long long)st.ceil_moves);
        atomicAdd(P.stats + 24, (unsigned long long)st.above_top);
        atomicAdd(P.stats + 25, (unsigned long long)st.bends);
        atomicAdd(P.stats + 26, (unsigned long long)st.tints);
        atomicAdd(P.stats + 27, (unsigned long long)st.tint_iters);
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
