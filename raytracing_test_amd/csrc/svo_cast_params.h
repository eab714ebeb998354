// svo_cast_params.h — what a cast launch passes to its kernel (CastParams), the hit a ray returns and the launch
// constants, shared by the translation units that launch k_cast (svo_cast.hip) and those that define its
// instances (svo_cast_inst_*.hip).  No device code.
#pragma once

#include <hip/hip_runtime.h>

#include "svo_internal.h"

using namespace svo;

enum : int32_t { MODE_FRAME = 0, MODE_EXPLICIT = 1, MODE_SINGLE = 2 };

// dda_axis for a ray from origin o along a direction whose step signs are known: cell = trunc(o)
// and frac = exact - cell (exact = o, or o - 1 when the step is negative), both exact; a ray's
// first crossing is then adelta - frac * delta (frac * delta exact in double: one rounding, as
// dda_axis' product and difference)
struct FrameAxes {
    double frac[3];
    int32_t cell[3];
};

struct CastParams {
    const Node* nodes;
    const uint16_t* mats;
    int32_t levels;
    uint32_t wmask;
    int32_t mode;
    int32_t steps;
    int32_t flags;
    unsigned long long* stats;
    // frame mode
    RayGen rg;
    float org[3];
    float sdir[3];
    int32_t width, height, tiles_x, tile_row_start, tile_row_step, tile_rows_local;
    int32_t tile_lh;  // log2 of a wavefront's pixel rows (frame_wave_lh)
    int32_t half_rows;  // the first tile rows dispatched, cast by half footprints (frame_half_rows: small launches)
    int32_t n_frames;        // frames in this launch (>= 1); frame f casts from frame_org[3f..]
    int64_t frame_records;   // records of one frame (this shard)
    float frame_org[3 * SVO_MAX_FRAMES];
    // octant instances (frame_dirs): dda_axis' per-axis set-up of each frame origin, hoisted to the
    // host (the same for every ray of the frame: the steps' signs are the octant's)
    FrameAxes fax[SVO_MAX_FRAMES];
    // explicit mode
    const float* rdir;
    const float* rorg;
    int64_t n_rays;
    // outputs
    int32_t* pos;
    float* t;
    uint32_t* info;
    uint8_t* ao;
    uint32_t* wire;        // svo_cast_wire: the wire record of each ray instead of its hit record (svo_wire.h)
    int32_t wire_compact;  // 8-B records
    // hemisphere AO (A8)
    int32_t ao_n, ao_steps;
    float ao_tab[3 * 64];
    const uint32_t* ao_plan;  // device AO plan (ao_plan_get) or null
    // shading: palette colours / flags, sun, highlighted block, shadow budget
    const uint64_t* mat_color;
    const uint32_t* mat_flags;
    float4* rgba;
    float sun[3];
    int32_t sun_dirs;  // the shadow rays' step-sign octant (dirs_sign numbering, 1..8): every shadow ray steps with the sun's signs
    int32_t look[3];
    int32_t look_valid, shadow_steps;
    int32_t look_empty;         // the host look-at voxel is not stored in the scene (an escaped ray could end on it)
    const int32_t* look_dev;    // device lookingAtBlock record (svo_ray_result: pos first) or null
    float time;                 // deltaTime of the liquid wobble (low_res.frag:226)
    const Node* snodes;         // shading: the solid-view tree the shadow rays walk (nodes: the scene)
    const uint16_t* smats;
    // the highest stored voxel row of the scene / of the solid tree (tree_top_y; casts: top_solid); a ray
    // moving up above it that cannot wrap in y before its budget ends can hit nothing more
    int32_t top_scene, top_solid;
    // column ceilings of the tree the rays walk (the scene, for shading): two levels of the tree's table
    // (set_ceilings), blocks 2^ceil_sh[j] columns wide, row-major at ceil + ceil_off[j] (svo_internal.h
    // tree_ceilings); ceil_levels: how many of the two the tree has
    const int16_t* ceil;
    int32_t ceil_levels;
    uint32_t ceil_sh[2];
    int64_t ceil_off[2];
    const uint32_t* ceilp;  // the launch's two levels paired (svo_tree.d_ceilp at its first level's offset)
    const uint32_t* sceilp;  // shading: the same pairs of the solid-view tree the shadow rays walk (trace T_CEIL_SHADOW)
    int32_t sceil_levels;
    const uint64_t* ceilq;  // every level per finest block (svo_tree.d_ceilq; trace CEIL == 2)
    // the fine ceilings of the tree the rays walk (svo_tree.d_ceilf: 4-column blocks, row-major), which the march before
    // the loop descends onto (ceil_march); null: none, or the launch's first level is not the table's finest
    const int16_t* ceilf;
    // the levels of `ceil` coarser than the launch's first that the march walks before it, coarsest first (march_levels,
    // svo_plan.h): blocks 2^march_sh[j] columns wide, row-major at ceil + march_off[j]; each 4 times as wide as the next, the
    // last 4 times as wide as the launch's first level.  march_n 0: the march starts on the first level's blocks
    int32_t march_n;
    uint32_t march_sh[2];
    int64_t march_off[2];
    uint32_t* guard_trips;  // the tree's counter of progress-guard trips (svo_tree_guard_trips)
    // frame schedule (sched_attach): launch block b casts frame block sched_order[b] (null: b) and, with sched_cost,
    // writes its duration (100 MHz ticks) to sched_cost[frame block]
    const uint32_t* sched_order;
    uint32_t* sched_cost;
};

constexpr int kBlock = 64;    // threads per block: one wavefront per tile footprint
constexpr int kSchedGroup = SVO_SCHED_GROUP;  // frame schedules order groups of this many consecutive blocks (sched_attach)
// (round 3's A/B switches — ceiling caching and packing, wave-gated boxes, XCD grouping, issue priority —
// were resolved to their measured winners and removed from the source; the losing sides are in git history
// (DESIGN.md cites the commits) and build_variant.py --rev rebuilds them.  The critical-path diagnostics
// (an iteration cap, dropping the top tile rows) are patches: tools/variants/*.patch, build_variant.py --patch)
// waves per SIMD of the shading instances on the camera's octant: 72 VGPRs (0-4 spilled).  The LDS allows 7 blocks per
// SIMD when the launch's path depth is its own (dynamic, path_lds: 3.75 KB for 6 levels) and the bounce state packs into
// 28 B per lane: 7 waves measured 4 % faster than 6 (80 VGPRs), which was 0.7 % faster than 5 (85 VGPRs) with the straight
// trace on the camera's octant (profiles/r05/shade_split_ab.json); 8 with the bounce state in registers spilled 22 VGPRs.
// The generic-sign instance (no octant) runs 6 (80 VGPRs: 7 would spill 29)
constexpr int kShadeWaves = 7;

struct Hit {
    int32_t x, y, z, steps_left;
    float t;
    uint32_t info;
};

using CastKernel = void (*)(CastParams);
