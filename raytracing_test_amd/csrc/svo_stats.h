// svo_stats.h — the diagnostics counters of the T_STATS / L_STATS instances: a lane's counters (Stats), the wave-level
// helpers, and the slots of the launch's counter buffer (S_*).  Used by svo_lookup.h, svo_brick.h, svo_ceil_march.h,
// trace() in svo_trace.h and k_cast (svo_cast_kernel.h).
#pragma once

#include "svo_cast_params.h"

struct Stats {
    uint32_t lookups, loads, skips, skip_out, brick_steps, plain_steps;
    uint32_t skip_by_sh[4];  // crossings whose box is made of 2^sh cells: sh = 2, 4, 6, >= 8
    uint32_t bricks;         // brick visits
    uint32_t wv_iters, wv_brick;  // wave-level executions (counted on the first active lane): outer
                                  // loop iterations, brick voxel steps
    uint32_t root_starts, cache_empty;  // lookups started at the root (a load of it, or a path restart at depth 0, where
                                        // it stands once a trace has seeded it); lookups answered by the parent mask
    uint32_t path_starts;                          // lookups restarted from the LDS path
    uint32_t wv_skips, wv_descents;                // wave-level crossings, descent levels
    uint32_t no_progress;                          // loop iterations that consumed no budget (the guard's trips: 0)
    uint32_t ceil_moves;                           // crossings of a column-ceiling box (no lookup)
    uint32_t iters;                                // this lane's traversal iterations
    uint32_t above_top;                            // iterations that start above the tree's highest stored row
    uint32_t bends;                                // reflections and refractions (shading)
    uint32_t tints, tint_iters;                    // refractive voxels passed; iterations that ended passing one
    uint32_t march_fine, march_descents;           // the march before the loop: 4-column blocks passed; descents onto them
    uint32_t march_64, march_256;                  // ... and the blocks passed at its 64- and 256-column levels
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

// The slots of the launch's counter buffer (CastParams::stats, the first SVO_STATS_HEADER words): where trace() adds a
// ray's Stats when it ends, and k_cast the AO rays' node loads.  The mirror of STAT_NAMES in raytracing_test_amd/__init__.py,
// which names the same slots in the same order for the host (tests/test_host.py holds the two together): a counter is
// added to both, at the end.
enum : int32_t {
    S_RAYS = 0,
    S_LOOKUPS,
    S_LOADS,
    S_SKIPS,
    S_SKIP_OUT,
    S_BRICK_STEPS,
    S_PLAIN_STEPS,
    S_LANE_WORK,           // the lanes' work units, summed over the wave (once per wave)
    S_WAVE_MAX_WORK_X64,   // the wave's largest lane work times 64 (once per wave): lane_work / this = SIMD efficiency
    S_SKIPS_4,             // skip_by_sh[0..3]
    S_SKIPS_16,
    S_SKIPS_64,
    S_SKIPS_256PLUS,
    S_BRICKS,
    S_WV_ITERS,
    S_WV_BRICK,
    S_NO_PROGRESS = 16,
    S_ROOT_STARTS,
    S_CACHE_EMPTY,
    S_WV_SKIPS,
    S_WV_DESCENTS,
    S_PATH_STARTS,
    S_AO_NODE_LOADS = 22,  // (k_cast: the node loads of a pixel's AO rays)
    S_CEIL_MOVES,
    S_ABOVE_TOP,
    S_BENDS,
    S_TINTS,
    S_TINT_ITERS = 27,
};
// The march's counters, after them: a list of their own (MARCH_STAT_NAMES in raytracing_test_amd/__init__.py, in the
// same order), so that the list above and STAT_NAMES stay the 28 slots every earlier reader of the buffer indexes.
enum : int32_t {
    S_MARCH_FINE = 28,
    S_MARCH_DESCENTS,
    S_MARCH_64,
    S_MARCH_256,
};
static_assert(S_MARCH_FINE == S_TINT_ITERS + 1 && S_MARCH_256 + 1 <= SVO_STATS_HEADER,
              "the counters' slots end before the per-block stamps");
