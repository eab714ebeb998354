// svo_cast.hip — launching the cast kernel (k_cast, svo_cast_kernel.h; its instances: svo_cast_inst_*.hip): a launch's
// parameters and instance, the frame schedules, the pick ray, the cast entry points of include/svo_rt.h and the
// introspection calls.  Device residency is svo_device.hip's, the hit-record wire format svo_hits_wire.hip's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "svo_cast_kernel.h"
#include "svo_hip.h"
#include "svo_plan.h"

namespace {

// The next frame's dispatch order from this frame's block durations (one workgroup): a counting sort, longest first, of
// groups of kSchedGroup consecutive blocks (a group's duration: its longest block's) on 256 logarithmic buckets (8 per
// octave: durations within 12.5 % share one; groups within a bucket in any order).  Its cost is the LDS atomics, which
// serialise on a bucket (most blocks share a few): per block 24 us for a 1080p frame, per group of 4 a quarter; the
// groups also keep 64 x 4-pixel strips of a tile row together.  All of a thread's loads go out together (kSchedBatch
// per thread, kept in registers for the scatter up to 32768 groups).  The key is a function of the duration alone,
// and every group index lands once: the order is a permutation whatever the durations.
constexpr int kSchedThreads = 1024, kSchedBuckets = 256, kSchedBatch = 32;
__device__ __forceinline__ uint32_t sched_key(uint32_t c) {
    // bits 20.. of the f32 value: exponent and 3 mantissa bits; c >= 1 gives 0 .. 255 from 1 to 2^32 (c near 2^32 rounds
    // to 2^32: 256, clamped)
    if (c == 0u) return (uint32_t)(kSchedBuckets - 1);
    return (uint32_t)(kSchedBuckets - 1) - std::min((__float_as_uint((float)c) >> 20) - (127u << 3), (uint32_t)(kSchedBuckets - 1));
}
// the duration of group i: its longest block (kSchedGroup == 4: one 16-B load)
__device__ __forceinline__ void sched_load(const uint32_t* __restrict__ cost, uint32_t n, uint32_t base, uint32_t (&c)[kSchedBatch]) {
    static_assert(kSchedGroup == 4, "one uint4 per group");
#pragma unroll
    for (int j = 0; j < kSchedBatch; j++) {
        const uint32_t i = base + (uint32_t)j * kSchedThreads + threadIdx.x;
        const uint4 q = i < n ? reinterpret_cast<const uint4*>(cost)[i] : make_uint4(0u, 0u, 0u, 0u);
        c[j] = std::max(std::max(q.x, q.y), std::max(q.z, q.w));
    }
}
// n: groups
__global__ __launch_bounds__(kSchedThreads) void k_sched_order(const uint32_t* __restrict__ cost, uint32_t* __restrict__ order, uint32_t n) {
    __shared__ uint32_t hist[kSchedBuckets];
    __shared__ uint32_t wsum[kSchedBuckets / 64];
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t kRound = (uint32_t)kSchedThreads * kSchedBatch;
    uint32_t c[kSchedBatch];
    sched_load(cost, n, 0u, c);
    if (tid < kSchedBuckets) hist[tid] = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += kRound) {
        if (base) sched_load(cost, n, base, c);
#pragma unroll
        for (int j = 0; j < kSchedBatch; j++)
            if (base + (uint32_t)j * kSchedThreads + tid < n) atomicAdd(&hist[sched_key(c[j])], 1u);
    }
    __syncthreads();
    // exclusive scan of the histogram: per wavefront, then the wavefronts' totals
    uint32_t v = 0u, inc = 0u;
    if (tid < kSchedBuckets) {
        v = hist[tid];
        inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
            if ((tid & 63u) >= (uint32_t)o) inc += u;
        }
        if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
    }
    __syncthreads();
    if (tid < kSchedBuckets) {
        uint32_t b = 0u;
        for (uint32_t w = 0; w < (tid >> 6); w++) b += wsum[w];
        hist[tid] = b + inc - v;
    }
    __syncthreads();
    for (uint32_t base = 0; base < n; base += kRound) {
        if (n > kRound) sched_load(cost, n, base, c);  // (one round: the durations are still in c)
#pragma unroll
        for (int j = 0; j < kSchedBatch; j++) {
            const uint32_t i = base + (uint32_t)j * kSchedThreads + tid;
            if (i < n) order[atomicAdd(&hist[sched_key(c[j])], 1u)] = i;
        }
    }
}

// The AO plan of (n samples, `steps`) (ao_plan_image; see ao_count_plan) on the device.  Cached on the tree.
static int ao_plan_get(const svo_tree* t, int32_t n, int32_t steps, const float* tab, const uint32_t** out) {
    *out = nullptr;
    if (t->d_ao_plan && t->ao_plan_n == n && t->ao_plan_steps == steps) {
        *out = reinterpret_cast<const uint32_t*>(t->d_ao_plan);
        return SVO_OK;
    }
    const std::vector<uint32_t> img = ao_plan_image(n, steps, tab);
    if (img.empty()) return SVO_OK;
    if (t->d_ao_plan) (void)hipFree(t->d_ao_plan);
    t->d_ao_plan = nullptr;
    t->ao_plan_steps = -1;
    HIP_TRY(hipMalloc(&t->d_ao_plan, img.size() * sizeof(uint32_t)), SVO_ENOMEM);
    HIP_TRY(hipMemcpy(t->d_ao_plan, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    t->ao_plan_n = n;
    t->ao_plan_steps = steps;
    *out = reinterpret_cast<const uint32_t*>(t->d_ao_plan);
    return SVO_OK;
}

// node addressing of a cast over t: 64-bit when its device allocation holds more nodes than a 32-bit
// buffer offset reaches (or on request)
bool wide_nodes(const svo_tree* t, int32_t flags) { return t->dev_node_cap >= kNarrowNodes || (flags & SVO_CAST_WIDE_ADDR); }

// The per-lane LDS path of k_cast (Path): 3 dwords per interior depth (levels - 1 of them) per lane of the block
size_t path_lds(const CastParams& P) { return (size_t)(P.levels > 1 ? P.levels - 1 : 1) * 3 * kBlock * sizeof(uint32_t); }

// svo_plan.h's launch set-up, from a launch's parameters
int frame_dirs(const CastParams& P) { return P.mode == MODE_FRAME ? svo::frame_dirs(P.rg, P.width, P.height, P.flags) : 0; }
bool need_seg(const CastParams& P) {
    const bool frame = P.mode == MODE_FRAME;
    return svo::need_seg(P.flags, P.mode == MODE_EXPLICIT, P.steps, frame ? P.frame_org : P.org, frame ? P.n_frames : 1);
}
void frame_axes(CastParams& P, int dirs) {
    for (int32_t f = 0; dirs && f < P.n_frames; f++) svo::frame_axes(dirs, P.frame_org + 3 * f, P.fax[f].frac, P.fax[f].cell);
}
// what decides a launch's instance (svo_plan.h), with the frame set-up of its octant; shade: the shading pass
svo::CastRequest cast_request(CastParams& P, bool shade, bool wide) {
    svo::CastRequest q = {};
    q.stats = (P.flags & SVO_CAST_STATS) != 0;
    q.timeline = (P.flags & SVO_CAST_TIMELINE) != 0;
    q.ao = P.ao_n > 0;
    q.shade = shade;
    q.records = P.pos != nullptr;
    q.wide = wide;
    q.seg = need_seg(P);
    q.dirs = frame_dirs(P);
    frame_axes(P, q.dirs);
    return q;
}

// Every instance with its template arguments, from the lists that instantiate them; a launch runs the one that
// svo::cast_instance (svo_plan.h) picks for it
struct CastEntry {
    svo::CastInstance inst;
    CastKernel fn;
};
#define SVO_CAST_ENTRY(...) {{__VA_ARGS__}, &k_cast<__VA_ARGS__>},
const CastEntry kCastTable[] = {SVO_CAST_ALL(SVO_CAST_ENTRY)};
int launch_cast(const svo::CastRequest& q, dim3 grid, dim3 block, hipStream_t st, const CastParams& P) {
    const svo::CastInstance k = svo::cast_instance(q);
    for (const CastEntry& e : kCastTable) {
        const svo::CastInstance& i = e.inst;
        if (i.stats != k.stats || i.stamps != k.stamps || i.ao != k.ao || i.shade != k.shade || i.wide != k.wide || i.seg != k.seg ||
            i.dirs != k.dirs || i.norec != k.norec)
            continue;
        CastParams arg = P;
        void* args[] = {&arg};
        (void)hipLaunchKernel(reinterpret_cast<const void*>(e.fn), grid, block, args, path_lds(P), st);
        return SVO_OK;
    }
    SVO_FAIL(SVO_EDEVICE, "k_cast: no instance <" + std::to_string(k.stats) + ", " + std::to_string(k.stamps) + ", " + std::to_string(k.ao) + ", " +
                              std::to_string(k.shade) + ", " + std::to_string(k.wide) + ", " + std::to_string(k.seg) + ", " + std::to_string(k.dirs) +
                              ", " + std::to_string(k.norec) + "> (svo_cast_instances.h)");
}

// The two ceiling levels a launch checks, as levels of the tree's table (4^(kCeilK0 + j) columns per block).
// Primary casts: 16 and 64 columns (C3 0.1824 -> 0.1787 ms, C5 0.562 -> 0.543 against 64 / 256; 16 / 256 was
// slower than both: profiles/r03/ab_j_*.log).  The shading pass walks every level (trace T_CEIL_QUADS: P.ceilq); its
// pair levels are unused.
constexpr int kCeilPrimary[2] = {0, kCeilPairStep}, kCeilShade[2] = {0, kCeilPairStep};
// (a launch's second level is read from the pair table, whose high half is level lv[0] + kCeilPairStep: the box of
// level lv[1] must come with the ceiling of a block that holds it)
static_assert(kCeilPrimary[1] - kCeilPrimary[0] == kCeilPairStep && kCeilShade[1] - kCeilShade[0] == kCeilPairStep,
              "ceiling pairs: the second level must be the pair table's partner level");

static void set_ceilings(const svo_tree* t, const svo_cast_desc* d, CastParams& P, const int lv[2]) {
    P.ceil = nullptr;
    P.ceil_levels = 0;
    P.march_n = 0;
    if (d->flags & SVO_CAST_NO_CEILINGS) return;
    P.ceil = reinterpret_cast<const int16_t*>(t->d_ceil);
    P.ceil_levels = t->ceil_levels > lv[1] ? 2 : (t->ceil_levels > lv[0] ? 1 : 0);
    // (the pair table of level lv[0] holds lv[0] + kCeilPairStep = lv[1] when the tree has it, else its coarsest level, whose
    // blocks hold level lv[0]'s: with one level the kernel's second box is then level lv[0]'s — as below — under a ceiling
    // at least as high as that block's own, which is safe)
    P.ceilp = P.ceil_levels > 0 ? reinterpret_cast<const uint32_t*>(t->d_ceilp) + t->ceilp_off[lv[0]] : nullptr;
    P.ceilq = P.ceil_levels > 0 ? reinterpret_cast<const uint64_t*>(t->d_ceilq) : nullptr;
    P.ceilf = ceil_fine_for(P.ceil_levels, lv[0]) ? reinterpret_cast<const int16_t*>(t->d_ceilf) : nullptr;
    for (int j = 0; j < 2; j++) {
        // (one level only: the second is a copy of the first, so the kernel may read both unconditionally)
        const int l = j < P.ceil_levels ? lv[j] : lv[0];
        P.ceil_sh[j] = 2u * (uint32_t)(kCeilK0 + l);
        P.ceil_off[j] = t->ceil_off[l];
    }
    // the coarser levels the march walks first (already in d_ceil: no table of their own)
    const MarchParams mp = march_params(t, P.ceil_levels, lv[0]);
    P.march_n = mp.n;
    for (int j = 0; j < kMarchCoarseMax; j++) {
        P.march_sh[j] = mp.sh[j];
        P.march_off[j] = mp.off[j];
    }
}

// the tree's progress-guard trip counter: a u32 in its device side buffer (svo_internal.h kSideGuard)
uint32_t* guard_word(const svo_tree* t) { return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(t->d_pick) + kSideGuard); }

int fill_params(const svo_tree* t, const svo_cast_desc* d, const svo_hits* o, CastParams& P, int64_t& nthreads) {
    memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const Node*>(t->d_nodes);
    P.mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    P.mat_color = reinterpret_cast<const uint64_t*>(t->d_pal);
    P.mat_flags = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(t->d_pal) + t->dev_pal_n * 8);
    P.levels = t->levels;
    P.wmask = (1u << (2 * t->levels)) - 1u;
    P.top_solid = t->dev_top_y;  // the empty region above the tree's highest voxel row (trace: pre_top)
    P.guard_trips = guard_word(t);
    set_ceilings(t, d, P, kCeilPrimary);
    P.steps = d->steps;
    P.flags = d->flags;
    P.stats = reinterpret_cast<unsigned long long*>(d->stats);
    P.org[0] = d->origin[0];
    P.org[1] = d->origin[1];
    P.org[2] = d->origin[2];
    P.pos = o->pos_steps;
    P.t = o->t;
    P.info = o->info;
    P.ao = o->ao;
    P.ao_n = d->ao_samples;
    P.ao_steps = d->ao_steps;
    if (P.ao_n > 0) {
        hemisphere_table(P.ao_n, P.ao_tab);
        if (!(P.flags & SVO_CAST_AO_TRACE)) {
            int rc = ao_plan_get(t, P.ao_n, P.ao_steps, P.ao_tab, &P.ao_plan);
            if (rc) return rc;
        }
    }
    if (d->ray_dirs) {
        P.mode = MODE_EXPLICIT;
        P.rdir = d->ray_dirs;
        P.rorg = d->ray_origins;
        P.n_rays = d->n_rays;
        nthreads = d->n_rays;
        return SVO_OK;
    }
    P.mode = MODE_FRAME;
    raygen_init(P.rg, d->cam_dir, d->ppx, d->ppy, d->width, d->height);
    P.width = d->width;
    P.height = d->height;
    // wavefronts per tile row: one per 16x4 footprint (or 8x8 / 32x2: svo_rt.h)
    P.tile_lh = frame_wave_lh(d->flags);
    P.tiles_x = frame_wave_cols(d->width, P.tile_lh);
    P.tile_row_start = d->tile_row_start;
    P.tile_row_step = d->tile_row_step;
    const int32_t tile_rows = (d->height + 7) / 8;
    P.tile_rows_local = d->tile_row_start < tile_rows ? (tile_rows - d->tile_row_start + d->tile_row_step - 1) / d->tile_row_step : 0;
    if (d->n_frames < 0 || d->n_frames > SVO_MAX_FRAMES) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: n_frames outside [0, SVO_MAX_FRAMES]");
    if (d->n_frames > 1 && !d->frame_origins) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: n_frames > 1 without frame_origins");
    P.n_frames = d->n_frames > 1 ? d->n_frames : 1;
    P.half_rows = frame_half_rows(P.tile_rows_local, d->flags, P.tile_lh, P.tiles_x, P.n_frames);
    for (int32_t f = 0; f < P.n_frames; f++)
        for (int k = 0; k < 3; k++) P.frame_org[3 * f + k] = d->n_frames > 1 ? d->frame_origins[3 * f + k] : d->origin[k];
    int64_t per_frame = 0;
    for (int32_t r = d->tile_row_start; r < tile_rows; r += d->tile_row_step) per_frame += std::min(8, d->height - r * 8);
    P.frame_records = per_frame * d->width;
    // (a dispatch holds fewer than 2^32 work-items: the HSA packet's grid size is 32-bit)
    if ((int64_t)(P.tile_rows_local + P.half_rows) * P.tiles_x * P.n_frames >= (int64_t)1 << 26)
        SVO_FAIL(SVO_ERANGE, "svo_cast_rays: frame too large (2^26 wavefronts or more in one launch)");
    nthreads = (int64_t)(P.tile_rows_local + P.half_rows) * P.tiles_x * P.n_frames * 64;
    return SVO_OK;
}

// Frame schedules: a shading launch of more than SVO_SCHED_MIN_BLOCKS blocks finds the schedule of its (stream, kind)
// and, when the frame geometry matches the last one, dispatches in its order; every block writes its duration, and
// sched_order() (after the launch, same stream) sorts them into the next frame's order.  One schedule per stream:
// launches on one stream run in order, so the sort never overlaps a launch reading its order.
// Measured (r04_at, 1080p frames): the shaded C3 frame 0.4667 -> 0.3782 ms — its bent-ray waves (up to 250 us) start at
// once instead of mid-launch, and the launch packs to its work (span 363 us against 340 us of block time per wave
// slot).  Primary casts keep the default order (kinds 0 / 1 are not scheduled): their longest waves are already
// dispatched first (top tile rows), and the sorted order loses the neighbouring tiles' shared node reads — C3 0.1678 ->
// 0.1941 ms, C4 0.2314 -> 0.2569, C5 0.5078 -> 0.6209 when scheduled.
constexpr size_t kSchedMax = 16;  // schedules per tree (least recently used replaced)
struct SchedUse {  // a launch's schedule (sched_attach), by value: the tree's list may change under other threads
    uint32_t* base = nullptr;
    int64_t blocks = 0;
    int32_t kind = 0;
};
// `lock` (the tree's sched_mu) is taken here and stays held by the caller until the launch and its sort are queued
// (sched_order): the buffer handed out cannot be freed by another thread's eviction or resize before the work that uses
// it is on its stream (hipFree synchronises the device, which protects queued work only)
SchedUse sched_attach(const svo_tree* t, const svo_cast_desc* d, CastParams& P, int32_t kind, int64_t blocks, hipStream_t st,
                      std::unique_lock<std::mutex>& lock) {
    if (P.mode != MODE_FRAME || (P.flags & (SVO_CAST_NO_SCHEDULE | SVO_CAST_STATS)) || blocks <= SVO_SCHED_MIN_BLOCKS ||
        blocks > 0x7FFFFFFFll || blocks % kSchedGroup)
        return SchedUse{};
    const int64_t sig[7] = {P.width, P.height, P.n_frames, P.tile_row_start, P.tile_row_step, P.tile_lh, (int64_t)(P.flags & SVO_CAST_BOTTOM_FIRST)};
    lock = std::unique_lock<std::mutex>(t->sched_mu);
    svo_tree::Sched* s = nullptr;
    for (auto& e : t->scheds)
        if (e.stream == (void*)st && e.kind == kind) s = &e;
    if (!s) {
        if (t->scheds.size() >= kSchedMax) {
            auto lru = std::min_element(t->scheds.begin(), t->scheds.end(),
                                        [](const svo_tree::Sched& a, const svo_tree::Sched& b) { return a.last_use < b.last_use; });
            (void)hipFree(lru->d_buf);  // (synchronises the device: no launch still reads it)
            t->scheds.erase(lru);
        }
        t->scheds.push_back(svo_tree::Sched{(void*)st, kind, {0}, 0, nullptr, 0, false, 0, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f},
                                            {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}});
        s = &t->scheds.back();
    }
    s->last_use = ++t->sched_clock;
    if (s->blocks < blocks) {
        if (s->d_buf) (void)hipFree(s->d_buf);
        s->d_buf = nullptr;
        s->blocks = 0;
        if (hipMalloc(&s->d_buf, (size_t)blocks * 8) != hipSuccess) {  // (no schedule; the launch runs unscheduled)
            (void)hipGetLastError();
            s->d_buf = nullptr;
            return SchedUse{};
        }
    }
    const float cam[6] = {P.frame_org[0], P.frame_org[1], P.frame_org[2], d->cam_dir[0], d->cam_dir[1], d->cam_dir[2]};
    const SchedPlan plan = sched_decide(*s, blocks, sig, cam);
    uint32_t* base = reinterpret_cast<uint32_t*>(s->d_buf);
    P.sched_order = plan.use_order ? base : nullptr;
    P.sched_cost = plan.write_cost ? base + blocks : nullptr;
    return SchedUse{plan.sort ? base : nullptr, blocks, kind};
}
// after the launch of a scheduled frame: the next frame's order (the schedule counts as sorted once the sort is queued);
// called with sched_attach's lock still held
int sched_order(const svo_tree* t, const SchedUse& u, hipStream_t st) {
    if (!u.base) return SVO_OK;
    hipLaunchKernelGGL(k_sched_order, dim3(1), dim3(kSchedThreads), 0, st, u.base + u.blocks, u.base, (uint32_t)(u.blocks / kSchedGroup));
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    for (auto& e : t->scheds)
        if (e.stream == (void*)st && e.kind == u.kind && e.d_buf == (void*)u.base && e.blocks == u.blocks) e.primed = true;
    return SVO_OK;
}

}  // namespace

// ================================================================================================
// casting
// ================================================================================================
// the checks of a tree and a desc that svo_shade_rays and svo_cast_rays / svo_cast_wire share (fn: the messages' prefix)
static int check_desc(const char* fn, const char* view_msg, const svo_tree* t, const svo_cast_desc* d) {
    const std::string f = std::string(fn) + ": ";
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, f + "tree not uploaded (svo_upload)");
    if (t->view != SVO_VIEW_SOLID) SVO_FAIL(SVO_EINVAL, f + view_msg);
    if (d->steps < 0) SVO_FAIL(SVO_EINVAL, f + "negative step budget");
    if ((d->flags & (SVO_CAST_STATS | SVO_CAST_TIMELINE)) && !d->stats) SVO_FAIL(SVO_EINVAL, f + "SVO_CAST_STATS / TIMELINE without a stats buffer");
    if (d->ray_dirs) {
        if (d->n_rays < 0) SVO_FAIL(SVO_EINVAL, f + "negative ray count");
    } else if (d->width <= 0 || d->height <= 0 || d->tile_row_step <= 0 || d->tile_row_start < 0) {
        SVO_FAIL(SVO_EINVAL, f + "bad frame geometry");
    }
    return SVO_OK;
}

extern "C" int svo_shade_rays(const svo_tree* t, const svo_cast_desc* d, const svo_shade_desc* sd, float* rgba,
                              const svo_hits* o, void* stream) {
    if (!t || !d || !sd || !rgba) SVO_FAIL(SVO_EINVAL, "svo_shade_rays: NULL argument");
    int rc = check_desc("svo_shade_rays", "t must be a solid-view tree (the scene goes in svo_shade_desc.scene)", t, d);
    if (rc) return rc;
    if (sd->shadow_steps < 0) SVO_FAIL(SVO_EINVAL, "svo_shade_rays: negative step budget");
    if (d->ao_samples != 0) SVO_FAIL(SVO_EINVAL, "svo_shade_rays: AO is a separate pass (ao_samples must be 0)");
    if (o && (!o->pos_steps || !o->t || !o->info)) SVO_FAIL(SVO_EINVAL, "svo_shade_rays: incomplete hit buffers");
    const svo_tree* sc = sd->scene ? sd->scene : t;
    if (sc->device != t->device) SVO_FAIL(SVO_ESTATE, "svo_shade_rays: scene tree not uploaded to the tree's device");
    if (sc->levels != t->levels) SVO_FAIL(SVO_EINVAL, "svo_shade_rays: scene and tree differ in levels");
    const svo_hits none = {nullptr, nullptr, nullptr, nullptr};
    CastParams P;
    int64_t n = 0;
    rc = fill_params(sc, d, o ? o : &none, P, n);
    if (rc) return rc;
    set_ceilings(sc, d, P, kCeilShade);
    // shadow rays walk t: its own column ceilings (the scene's hold for the scene's voxels, which is t's world only when
    // both trees are synced to the same edits), and t's guard-trip counter (svo_tree_guard_trips counts launches over t)
    {
        CastParams S{};  // (set_ceilings leaves it untouched under SVO_CAST_NO_CEILINGS: compared zeroed)
        set_ceilings(t, d, S, kCeilShade);
        const bool same = S.ceil_levels == P.ceil_levels && S.ceil_sh[0] == P.ceil_sh[0] && S.ceil_sh[1] == P.ceil_sh[1];
        P.sceilp = same ? S.ceilp : nullptr;
        P.sceil_levels = same ? S.ceil_levels : 0;  // (shadow rays then walk the tree)
    }
    P.guard_trips = guard_word(t);
    P.snodes = reinterpret_cast<const Node*>(t->d_nodes);
    P.smats = reinterpret_cast<const uint16_t*>(t->d_mats);
    P.time = sd->time;
    P.top_scene = sc->dev_top_y;
    P.top_solid = t->dev_top_y;
    P.rgba = reinterpret_cast<float4*>(rgba);
    P.sun_dirs = (d->flags & SVO_CAST_NO_OCTANT) ? 0 : 1;  // (0: per-wave sign flags for the shadow rays as well)
    for (int k = 0; k < 3; k++) {
        P.sun[k] = sd->sun_dir[k];
        if (P.sun_dirs) P.sun_dirs += (sd->sun_dir[k] < 0.0f ? 1 : 0) << k;  // (dda_axis' step: -1 only below zero; -0.0, NaN: +)
        P.look[k] = sd->look_at[k];
    }
    P.look_valid = sd->look_at_valid != 0;
    if (P.look_valid && !sd->look_at_dev) {
        svo_block b;
        uint32_t mid = 0;
        rc = svo_tree_get_block(sc, sd->look_at[0], sd->look_at[1], sd->look_at[2], &b, &mid);
        if (rc) return rc;
        // (palette entry 0: no block).  The host image runs ahead of HBM between svo_tree_update and svo_tree_sync: with
        // edits not yet synced the device scene may still lack (or hold) that voxel, so it is taken as possibly empty
        // there — no shading ray escapes early then, and an escaped miss cannot lose the highlight
        P.look_empty = mid == 0u || tree_unsynced(sc);
    }
    P.look_dev = reinterpret_cast<const int32_t*>(sd->look_at_dev);
    P.shadow_steps = sd->shadow_steps;
    if (n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks * kBlock > 0xFFFFFFFFll) SVO_FAIL(SVO_ERANGE, "svo_shade_rays: too many rays for one launch");
    const bool wide = wide_nodes(t, d->flags) || wide_nodes(sc, d->flags);
    std::unique_lock<std::mutex> sched_lock;  // (held from here until the launch and the sort are queued)
    const SchedUse sch = sched_attach(t, d, P, 2, blocks, (hipStream_t)stream, sched_lock);
    // the straight trace runs on the camera's step octant (frame launches whose every pixel steps with it: frame_dirs;
    // shaded C3 0.3050 -> 0.2914 ms against generic sign flags, with the shadow rays' sun-octant instances given up
    // for it: profiles/r05/shade_split_ab.json); its segment bounds only when an origin needs them (0.2887 -> 0.2831)
    const svo::CastRequest q = cast_request(P, true, wide);
    rc = launch_cast(q, dim3((uint32_t)blocks), dim3(kBlock), (hipStream_t)stream, P);
    if (rc) return rc;
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return sched_order(t, sch, (hipStream_t)stream);
}

static int cast_launch(const svo_tree* t, const svo_cast_desc* d, const svo_hits* o, void* wire, void* stream);

extern "C" int svo_cast_rays(const svo_tree* t, const svo_cast_desc* d, const svo_hits* o, void* stream) {
    if (!t || !d || !o) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: NULL argument");
    if (!o->pos_steps || !o->t || !o->info) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: NULL output buffer");
    return cast_launch(t, d, o, nullptr, stream);
}

extern "C" int svo_cast_wire(const svo_tree* t, const svo_cast_desc* d, void* wire, uint8_t* ao, void* stream) {
    if (!t || !d || !wire) SVO_FAIL(SVO_EINVAL, "svo_cast_wire: NULL argument");
    if (d->flags & (SVO_CAST_STATS | SVO_CAST_TIMELINE)) SVO_FAIL(SVO_EINVAL, "svo_cast_wire: no diagnostics (svo_cast_rays has them)");
    WireParams Q;
    int rc = wire_params(t, d, "svo_cast_wire", Q);  // (the wire formats' limits)
    if (rc) return rc;
    const svo_hits o = {nullptr, nullptr, nullptr, ao};
    return cast_launch(t, d, &o, wire, stream);
}

static int cast_launch(const svo_tree* t, const svo_cast_desc* d, const svo_hits* o, void* wire, void* stream) {
    int rc = check_desc("svo_cast_rays", "castRayFromCam semantics need a solid-view tree", t, d);
    if (rc) return rc;
    if (d->ao_samples < 0 || d->ao_samples > 64) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: ao_samples must be in [0, 64]");
    if (d->ao_samples > 0 && (!o->ao || d->ao_steps < 0)) SVO_FAIL(SVO_EINVAL, "svo_cast_rays: AO needs an ao buffer and ao_steps >= 0");
    CastParams P;
    int64_t n = 0;
    rc = fill_params(t, d, o, P, n);
    if (rc) return rc;
    P.wire = reinterpret_cast<uint32_t*>(wire);
    P.wire_compact = wire && wire_bytes_for(t, d) == 8;
    if (n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks * kBlock > 0xFFFFFFFFll) SVO_FAIL(SVO_ERANGE, "svo_cast_rays: too many rays for one launch");
    const dim3 grid((uint32_t)blocks), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    const svo::CastRequest q = cast_request(P, false, wide_nodes(t, d->flags));
    const SchedUse sch = {};  // (primary casts: the default order; see sched_attach)
    rc = launch_cast(q, grid, block, st, P);
    if (rc) return rc;
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return sched_order(t, sch, st);
}

namespace {
// one pick ray's hit record (int4 pos + steps, f32 t, u32 info at +0 / +16 / +20 of buf) on `stream`
int pick_launch(const svo_tree* t, const float pos[3], const float dir[3], int32_t steps, void* buf, hipStream_t stream, const char* fn) {
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, std::string(fn) + ": tree not uploaded (svo_upload)");
    if (t->view != SVO_VIEW_SOLID) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": castRayFromCam semantics need a solid-view tree");
    if (steps < 0) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": negative step budget");
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    CastParams P;
    memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const Node*>(t->d_nodes);
    P.mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    P.levels = t->levels;
    P.wmask = (1u << (2 * t->levels)) - 1u;
    P.mode = MODE_SINGLE;
    P.top_solid = t->dev_top_y;
    P.guard_trips = guard_word(t);
    P.steps = steps;
    for (int a = 0; a < 3; a++) {
        P.org[a] = pos[a];
        P.sdir[a] = dir[a];
    }
    P.pos = reinterpret_cast<int32_t*>(buf);
    P.t = reinterpret_cast<float*>(reinterpret_cast<char*>(buf) + 16);
    P.info = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(buf) + 20);
    const svo::CastRequest q = cast_request(P, false, wide_nodes(t, 0));  // (no frame, no octant: dirs 0)
    const int rc = launch_cast(q, dim3(1), dim3(kBlock), stream, P);
    if (rc) return rc;
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return SVO_OK;
}

// the hit record at r (pick_launch) rewritten in place as a RayResult {pos, lastPos, steps} (ray_caster.hpp:6-10)
__global__ __launch_bounds__(64) void k_pick_result(int32_t* r) {
    if (threadIdx.x != 0) return;
    const int32_t x = r[0], y = r[1], z = r[2], st = r[3];
    const uint32_t info = (uint32_t)r[5];
    int32_t last[3] = {x, y, z};
    const uint32_t axis = (info >> AXIS_SHIFT) & 3u;
    if (axis < 3u) last[axis] -= (info & NEG_BIT) ? -1 : 1;
    r[0] = x;
    r[1] = y;
    r[2] = z;
    r[3] = last[0];
    r[4] = last[1];
    r[5] = last[2];
    r[6] = st;
}
}  // namespace

extern "C" int svo_cast_ray_from_cam_async(const svo_tree* t, const float pos[3], const float dir[3], int32_t steps, svo_ray_result* d_result,
                                           void* stream) {
    if (!t || !pos || !dir || !d_result) SVO_FAIL(SVO_EINVAL, "svo_cast_ray_from_cam_async: NULL argument");
    if (reinterpret_cast<uintptr_t>(d_result) & 15u) SVO_FAIL(SVO_EINVAL, "svo_cast_ray_from_cam_async: d_result not 16-byte aligned");
    int rc = pick_launch(t, pos, dir, steps, d_result, (hipStream_t)stream, "svo_cast_ray_from_cam_async");
    if (rc) return rc;
    hipLaunchKernelGGL(k_pick_result, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<int32_t*>(d_result));
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return SVO_OK;
}

extern "C" int svo_cast_ray_from_cam(const svo_tree* t, const float pos[3], const float dir[3], int32_t steps, svo_ray_result* out,
                                     svo_block* block) {
    if (!t || !pos || !dir || !out) SVO_FAIL(SVO_EINVAL, "svo_cast_ray_from_cam: NULL argument");
    // the tree's own result record: no allocation per pick (the reference casts one every frame, main.cpp:81);
    // one synchronous pick at a time per tree
    std::lock_guard<std::mutex> lock(t->pick_mu);
    void* buf = reinterpret_cast<char*>(t->d_pick) + kSidePick;
    int rc = pick_launch(t, pos, dir, steps, buf, nullptr, "svo_cast_ray_from_cam");
    if (rc) return rc;
    unsigned char host[32];
    hipError_t e = hipMemcpy(host, buf, 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) SVO_FAIL(SVO_EDEVICE, std::string("svo_cast_ray_from_cam: ") + hipGetErrorString(e));
    int32_t p4[4];
    uint32_t info;
    memcpy(p4, host, 16);
    memcpy(&info, host + 20, 4);
    for (int a = 0; a < 3; a++) out->pos[a] = out->last_pos[a] = p4[a];
    out->steps = p4[3];
    const uint32_t axis = (info >> AXIS_SHIFT) & 3u;
    if (axis < 3u) out->last_pos[axis] -= (info & NEG_BIT) ? -1 : 1;
    if (block) {
        const Material& m = t->palette[(info & HIT_BIT) ? (info & MAT_MASK) : 0u];
        *block = svo_block{m.flags, m.color, m.meta};
    }
    return SVO_OK;
}

extern "C" int svo_tree_device_ceilings(const svo_tree* t, int16_t* ceil, uint32_t* pairs, int64_t cap, int32_t* levels, int64_t* n) {
    if (!t || !levels || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_device_ceilings: NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_device_ceilings: tree not uploaded (svo_upload)");
    *levels = t->ceil_levels;
    *n = t->ceil_levels > 0 ? t->ceil_dev_n : 0;
    if ((ceil || pairs) && cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_device_ceilings: buffer too small");
    if (*n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    if (ceil) HIP_TRY(hipMemcpy(ceil, t->d_ceil, *n * sizeof(int16_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (pairs) HIP_TRY(hipMemcpy(pairs, t->d_ceilp, *n * sizeof(uint32_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    return SVO_OK;
}

extern "C" int svo_tree_device_ceiling_quads(const svo_tree* t, uint64_t* quads, int64_t cap, int64_t* n) {
    if (!t || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_device_ceiling_quads: NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_device_ceiling_quads: tree not uploaded (svo_upload)");
    *n = t->ceil_levels > 0 && t->d_ceilq ? (int64_t)t->ceilq_host.size() : 0;
    if (quads && cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_device_ceiling_quads: buffer too small");
    if (*n == 0 || !quads) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(quads, t->d_ceilq, *n * sizeof(uint64_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    return SVO_OK;
}

extern "C" int svo_tree_device_ceilings_fine(const svo_tree* t, int16_t* fine, int64_t cap, int64_t* n) {
    if (!t || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_device_ceilings_fine: NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_device_ceilings_fine: tree not uploaded (svo_upload)");
    *n = t->ceil_levels > 0 && t->d_ceilf ? (int64_t)t->ceil_fine_host.size() : 0;
    if (fine && cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_device_ceilings_fine: buffer too small");
    if (*n == 0 || !fine) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(fine, t->d_ceilf, *n * sizeof(int16_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    return SVO_OK;
}

extern "C" int svo_tree_schedule(const svo_tree* t, void* stream, int32_t kind, uint32_t* order, uint32_t* cost, int64_t cap, int64_t* n) {
    if (!t || !n) SVO_FAIL(SVO_EINVAL, "svo_tree_schedule: NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_schedule: tree not uploaded (svo_upload)");
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream), SVO_EDEVICE);
    std::lock_guard<std::mutex> lock(t->sched_mu);
    *n = 0;
    for (const auto& e : t->scheds) {
        if (e.stream != stream || e.kind != kind || !e.primed) continue;
        *n = e.blocks;
        if ((order || cost) && cap < *n) SVO_FAIL(SVO_ERANGE, "svo_tree_schedule: buffer too small");
        const uint32_t* base = reinterpret_cast<const uint32_t*>(e.d_buf);
        if (order) HIP_TRY(hipMemcpy(order, base, *n / kSchedGroup * sizeof(uint32_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
        if (cost) HIP_TRY(hipMemcpy(cost, base + e.blocks, *n * sizeof(uint32_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    }
    return SVO_OK;
}

extern "C" int svo_ceiling_layout(int32_t* k0, int32_t* pair_step) {
    if (k0) *k0 = kCeilK0;
    if (pair_step) *pair_step = kCeilPairStep;
    return SVO_OK;
}

extern "C" int svo_tree_guard_trips(const svo_tree* t, uint64_t* trips, int32_t reset) {
    if (!t || !trips) SVO_FAIL(SVO_EINVAL, "svo_tree_guard_trips: NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_guard_trips: tree not uploaded (svo_upload)");
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    uint32_t v = 0;
    // every launch over t finished, on whatever stream (a null-stream copy does not wait for non-blocking streams)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(&v, guard_word(t), sizeof(v), hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (reset) HIP_TRY(hipMemset(guard_word(t), 0, sizeof(v)), SVO_EDEVICE);
    *trips = v;
    return SVO_OK;
}

extern "C" int svo_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream), SVO_EDEVICE);
    return SVO_OK;
}
