/*
 * svo_rt.h — C ABI of the MI355X-native sparse-voxel-tree primary raycaster (libsvo_rt.so).
 *
 * Drop-in boundary for reedthorngag/raytracing_test's hot path (paths relative to the reference):
 *   - src/ray_caster.hpp:6-14          RayResult / RAY_CASTER::castRayFromCam(int steps)
 *   - src/voxel_data/tetrahexa_tree.hpp:12-22  initTetraHexaTree / putBlock / getBlock / deleteBlock
 *   - src/world_gen.hpp:3              genWorld()
 *   - src/voxel_data/voxel_allocator.hpp:38-91  updateSsboData / initVoxelDataAllocator (device upload)
 *   - src/shaders/low_res.frag:256-333,446-531  the per-pixel DDA + tree traversal, replaced by
 *                                      svo_cast_rays() (a hand-written gfx950 HIP kernel)
 *
 * Conventions: every function returns an int status (SVO_OK = 0, negative on error) and never
 * exits; svo_last_error() gives the message of the calling thread's last failure.  Pointers marked
 * "device" are HBM pointers on the tree's device (e.g. a torch tensor's data_ptr()); a hip_stream
 * argument is a hipStream_t (NULL = the null stream).  The tree is read-only during a cast.
 */
#ifndef SVO_RT_H
#define SVO_RT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_RT_VERSION 7  /* 2: svo_cast_desc.n_frames / frame_origins, wire records; 3: svo_exchange_*, 64-bit node addressing;
                             4: tree views (liquid stored for the shading pass), svo_shade_desc.scene / time;
                             6: svo_tree_save / svo_tree_load (5, a cost-ordered dispatch, was measured slower
                             and removed); 7: 8-B compact wire records, svo_wire_bytes / svo_cast_wire /
                             svo_wire_scatter / svo_exchange_wire.  Entry points added since keep the number and are
                             detected by symbol (dlsym / hasattr): svo_build_volume_gpu, svo_tree_read_volume,
                             svo_volume_classify_pass, svo_tree_patch_volume_gpu, svo_tree_garbage,
                             svo_tree_patch_times, svo_tree_compact_gpu, svo_tree_compact_times,
                             svo_build_points_gpu, svo_tree_get_blocks_gpu,
                             svo_tree_patch_points_gpu, svo_tree_list_voxels_gpu, svo_tree_diff_gpu,
                             svo_tree_patch_shapes_gpu, svo_tree_patch_tree_gpu, svo_tree_patch_tree_oriented_gpu,
                             svo_tree_patch_tree_rule_gpu */

enum {
    SVO_OK = 0,
    SVO_EINVAL = -1,  /* bad argument */
    SVO_ENOMEM = -2,  /* host or device allocation failed */
    SVO_EDEVICE = -3, /* HIP runtime error / no GPU */
    SVO_ESTATE = -4,  /* object not in the required state (e.g. tree not uploaded) */
    SVO_ERANGE = -5,  /* value outside what the structure supports */
    SVO_EIO = -6      /* file I/O failed, or the file is not a valid tree (svo_tree_load) */
};

/* Block (src/globals.hpp:76-80): leaf flags (bit 0 set for a stored voxel; REFLECTIVE 0x2,
   REFRACTIVE 0x4, LUMINESCENT 0x8, LIQUID 0x10), 3 x 21-bit packed colour (src/types.hpp:6-9),
   metadata.  The empty block is {0, ~0ull, 0}. */
typedef struct {
    uint32_t flags;
    uint64_t color;
    float metadata;
} svo_block;

/* RayResult (src/ray_caster.hpp:6-10) */
typedef struct {
    int32_t pos[3];
    int32_t last_pos[3];
    int32_t steps;
} svo_ray_result;

typedef struct svo_world svo_world; /* host-side editable 64-ary voxel tree */
typedef struct svo_tree svo_tree;   /* breadth-first linearised tree (host image + HBM copy) */

const char* svo_last_error(void);
int svo_version(void);
/* sha256 of the sources, headers and compile flags this library was built from (raytracing_test_amd/build.py
   sources_sha256; 64 hex digits): ties a measurement to the committed files */
const char* svo_build_id(void);

/* ---------------------------------------------------------------- world (host, editable) ---- */
/* levels = descending tree levels; extent = 4^levels voxels per axis (reference: 5 -> 1024^3,
   maxDepth 6 at src/voxel_data/tetrahexa_tree.hpp:6).  1 <= levels <= 7. */
int svo_world_create(int32_t levels, svo_world** out);
void svo_world_destroy(svo_world* w);
/* initTetraHexaTree (tetrahexa_tree.cpp:13-41): root + the reference's 8 debug blocks.  The
   reference's aliased root child array is NOT reproduced: the block at
   (1000,1000,1000) exists here, while the reference cannot reach it. */
int svo_init_tetra_hexa_tree(svo_world* w);
/* putBlock (tetrahexa_tree.cpp:176-291): level levels+1 = one voxel (reference: 6), levels = a
   4^3 block (reference: 5), ... 1 = the whole world.  Stored flags = 1 | b.flags. */
int svo_put_block(svo_world* w, int32_t x, int32_t y, int32_t z, const svo_block* b, int32_t level);
/* getBlock (tetrahexa_tree.cpp:113-157); coordinates wrap modulo the extent */
int svo_get_block(const svo_world* w, int32_t x, int32_t y, int32_t z, svo_block* out);
/* deleteBlock (tetrahexa_tree.cpp:293-359) with its intended meaning: clears the level-`level`
   region containing (x,y,z) (level as putBlock's) and returns the block found there. */
int svo_delete_block(svo_world* w, int32_t x, int32_t y, int32_t z, int32_t level, svo_block* removed);
/* genWorld (world_gen.cpp:13-42) over width x length columns (reference: 200 x 200) */
int svo_gen_world(svo_world* w, int32_t width, int32_t length);
/* genWorld's column puts (world_gen.cpp:24-39) from caller-given tops heights[x*length + z] */
int svo_gen_heightfield(svo_world* w, int32_t width, int32_t length, const int32_t* heights);
/* number of putBlock-visible tree nodes (diagnostics) */
int svo_world_node_count(const svo_world* w, uint64_t* nodes);
/* batched getBlock over n positions (xyz = 3 x int32 each) — the traverseTree batch lookup of
   tetrahexa_tree.cpp:43-111, made usable */
int svo_get_blocks(const svo_world* w, const int32_t* xyz, int64_t n, svo_block* out);
/* batched putBlock of n blocks, all at `level`, applied in order.  It stops at the first block that fails and returns
   that block's error: on SVO_ERANGE (a 65535th distinct block) the blocks before it are stored, it and the blocks
   after it are not, and the palette is unchanged by it */
int svo_put_blocks(svo_world* w, const int32_t* xyz, const svo_block* blocks, int64_t n, int32_t level);
/* OpenSimplex 2D (include/OpenSimplexNoise.cpp:77-208) for n points, and genWorld's column tops
   (world_gen.cpp:22) for x in [0,width), z in [0,length): out[x*length + z] */
int svo_noise2(int64_t seed, const double* x, const double* y, int64_t n, double* out);
int svo_terrain_heights(int32_t width, int32_t length, int32_t nthreads, int32_t* out);

/* ------------------------------------------------------------ tree (BFS, HBM-resident) ------ */
typedef struct {
    int32_t levels;
    uint32_t n_materials;         /* palette entries including id 0 (empty) */
    uint64_t n_nodes;             /* 16 B nodes */
    uint64_t n_mat_bytes;         /* per-voxel material bytes of mixed-material bricks */
    uint64_t n_bricks;            /* 4^3 brick nodes */
    uint64_t nodes_per_level[8];  /* nodes at depth 0..levels-1 */
    uint64_t device_bytes;        /* HBM footprint after svo_upload (0 before) */
    int32_t device;               /* -1 before svo_upload */
    int32_t view;                 /* SVO_VIEW_SOLID / SVO_VIEW_ALL */
} svo_tree_info;

/* Tree views.  SVO_VIEW_SOLID (every cast): the blocks castRayFromCam hits (ray_caster.cpp:82) —
   empty and LIQUID blocks are empty.  SVO_VIEW_ALL (the scene of the shading pass,
   svo_shade_desc.scene): every stored block, liquid included, as low_res.frag's getBlock sees it. */
#define SVO_VIEW_SOLID 0
#define SVO_VIEW_ALL 1

/* Linearise a world: collapse uniform regions, drop non-solid (empty / LIQUID) voxels, emit the
   breadth-first node array + material bytes + palette. */
int svo_build(const svo_world* w, svo_tree** out);
/* the same for a view (svo_build = SVO_VIEW_SOLID); edits (svo_tree_update) keep the tree's view */
int svo_build_view(const svo_world* w, int32_t view, svo_tree** out);
/* Build the same tree straight from genWorld's column formula over width x length columns
   (no per-voxel putBlock: depth-12 / depth-14 terrain); nthreads host threads (0 = all). */
int svo_build_terrain(int32_t levels, int32_t width, int32_t length, int32_t nthreads, svo_tree** out);
int svo_build_terrain_view(int32_t levels, int32_t width, int32_t length, int32_t nthreads, int32_t view, svo_tree** out);
/* the same builder from caller-given column tops heights[x*length + z] (0 <= h <= extent-2) */
int svo_build_heightfield(int32_t levels, int32_t width, int32_t length, const int32_t* heights, int32_t nthreads,
                          svo_tree** out);
/* The same two builders on the GPU: noise per column, min/max pyramid and a
   level-synchronous breadth-first build in HBM (one wavefront per region, ballots + scans).  The
   node / material arrays equal svo_build_terrain's byte for byte; the tree comes back already
   uploaded to `device` (plus its host image). */
int svo_build_terrain_gpu(int32_t levels, int32_t width, int32_t length, int32_t device, svo_tree** out);
int svo_build_terrain_gpu_view(int32_t levels, int32_t width, int32_t length, int32_t device, int32_t view, svo_tree** out);
int svo_build_heightfield_gpu(int32_t levels, int32_t width, int32_t length, const int32_t* heights, int32_t device, svo_tree** out);
/* A tree from a dense voxel volume already in HBM (a torch tensor from a generator, a voxelised model, a simulation
   grid): arbitrary content — overhangs, caves, floating blocks, any palette — without a host world.  A class pyramid
   over the volume's world-aligned bounding box (level 1 reads the volume once: one class per 4^3 brick; each level
   above folds 64 children) feeds the level-synchronous emitter of the terrain builders.  The output is the canonical
   linearisation: nodes, material runs, nodes_per_level, n_bricks and palette equal, byte for byte, what svo_build_view
   emits for a world holding the same blocks under the same palette ids.
     palette   entries other than 0 are stored with flags 1 | flags, as putBlock stores them
     view      an id is stored when the view holds its palette entry: LIQUID ids and ids whose colour is ~0 are empty
               in SVO_VIEW_SOLID, only ids whose colour is ~0 in SVO_VIEW_ALL
   SVO_EINVAL: NULL pointers, levels outside 2..7, a non-positive dimension, a box that leaves the extent, an unknown
   view, palette[0] not the empty block; SVO_ERANGE: n_palette outside 1..65535, a voxel id >= n_palette (found on
   the device by the first pass; nothing is emitted); SVO_ENOMEM: no scratch.  Arguments are checked before the first
   HIP call.  The device is synchronised on entry (the volume may come from any stream); the build runs on the null
   stream.  Such a tree has no svo_world behind it: svo_tree_update stays a world-only path, and a volume tree is
   changed in HBM by svo_tree_patch_volume_gpu. */
typedef struct {
    int32_t levels;              /* extent 4^levels per axis; 2..7 like the other GPU builders */
    int32_t nx, ny, nz;          /* voxels; voxels[((int64)z * ny + y) * nx + x] — a contiguous (nz, ny, nx) tensor */
    int32_t origin[3];           /* world position of voxels[0]; any integers with origin + n <= extent, >= 0 (no wrap) */
    const uint16_t* voxels;      /* DEVICE pointer on `device`: palette ids, 0 = empty */
    const svo_block* palette;    /* HOST: n_palette entries; entry 0 must be the empty block {0, ~0ull, 0} */
    uint32_t n_palette;          /* 1..65535 */
    int32_t view;                /* SVO_VIEW_SOLID / SVO_VIEW_ALL */
    int32_t device;
} svo_volume_desc;
/* the canonical tree of that content, built in HBM, returned uploaded to `device` with its host image
   (like svo_build_terrain_gpu); voxels outside the box are empty */
int svo_build_volume_gpu(const svo_volume_desc* v, svo_tree** out);
/* the palette id the tree stores (its view) for every voxel of the box origin .. origin + n, written to a
   device buffer in the same (nz, ny, nx) layout; coordinates wrap modulo the extent as svo_tree_get_blocks'
   do; asynchronous on hip_stream; tree must be uploaded (SVO_ESTATE otherwise) */
int svo_tree_read_volume(const svo_tree* t, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                         uint16_t* voxels, void* hip_stream);
/* diagnostics (tools/volume_build_timing.py): svo_build_volume_gpu's first pass alone — the level-1 classification,
   which reads the whole volume — run `runs` times into scratch, each timed by HIP events: ms[0 .. runs-1] */
int svo_volume_classify_pass(const svo_volume_desc* v, int32_t runs, float* ms);
/* A tree from a sparse list of voxels already in HBM (a voxelised mesh, a point cloud, a particle or fluid front,
   procedural scatter): the route to arbitrary content in worlds too large for a dense volume (levels 6 and 7).  The cost
   follows the number of points, never the extent's volume.  The points are applied in list order, as svo_put_blocks
   applies its blocks: when a voxel is listed more than once its last entry decides, and a last entry of id 0 leaves the
   voxel empty.  After that resolution an id is stored when the view holds its palette entry (svo_build_volume_gpu's
   rule: a LIQUID entry written last over a solid one gives an empty voxel in SVO_VIEW_SOLID, a liquid one in
   SVO_VIEW_ALL).  The output is the canonical linearisation: nodes, material runs, nodes_per_level, n_bricks,
   n_mat_bytes and palette equal, byte for byte, what svo_build_view emits for a world holding that content under the
   same palette ids, and what svo_build_volume_gpu emits for a dense volume of it.  n == 0 builds the empty tree, the
   lone record {0, 0, K_INTERIOR}; xyz and ids may then be NULL.
   One lane per point computes a 64-bit key (6 bits per level, the child slots from the root down) and checks the
   point; a stable radix sort of (key, id) puts every voxel's entries next to each other in list order; the stored
   voxels are compacted, and each level above holds the occupied 4^k cells with their classes (an id when all 64
   children carry it, else mixed), which the level-synchronous emitter of the other GPU builders searches.
   Scratch in HBM, freed on return: 24 B per point (two (key, id) pairs for the sort and a flag word), 10 B per stored
   voxel, 14 B per occupied cell of each of the `levels` levels above (a level never has more cells than the one below
   it, and 1/64 of them where the content is dense: at most 34 + 14 * levels B per point in all), hipCUB's sort and scan
   temporaries, and the emitter's own scratch per emitted region.
   SVO_EINVAL: NULL p or out, NULL xyz or ids with n > 0, NULL palette, levels outside 2..7, n < 0, an unknown view,
   palette[0] not the empty block; SVO_ERANGE: n_palette outside 1..65535, n > 2^31 - 1 — all checked before the first
   HIP call — and, found on the device by the first pass, an id >= n_palette or a coordinate outside [0, 4^levels):
   nothing is emitted, *out is untouched and the message says which of the two it was; SVO_ENOMEM: no scratch.  The
   device is synchronised on entry (the list may come from any stream); the build runs on the null stream.  The tree
   comes back uploaded to `device` with its host image, ceilings included.  It has no svo_world behind it:
   svo_tree_update returns SVO_ESTATE on it; svo_tree_patch_volume_gpu, svo_tree_patch_points_gpu and
   svo_tree_compact_gpu accept it. */
typedef struct {
    int32_t levels;              /* extent 4^levels per axis; 2..7 */
    int64_t n;                   /* points; 0 .. 2^31 - 1 */
    const int32_t* xyz;          /* DEVICE pointer on `device`: 3 x int32 per point (svo_get_blocks' layout); 0 <= c < 4^levels (no wrap) */
    const uint16_t* ids;         /* DEVICE pointer on `device`: palette id per point, 0 = empty */
    const svo_block* palette;    /* HOST: n_palette entries; entry 0 must be the empty block (as svo_volume_desc) */
    uint32_t n_palette;          /* 1..65535 */
    int32_t view;                /* SVO_VIEW_SOLID / SVO_VIEW_ALL */
    int32_t device;
} svo_points_desc;
int svo_build_points_gpu(const svo_points_desc* p, svo_tree** out);
/* the palette id the tree stores (its view) at each of n positions given in HBM (xyz = 3 x int32 each), written to the
   device buffer ids; coordinates wrap modulo the extent as svo_tree_get_blocks' and svo_tree_read_volume's do.  One lane
   per position descends the resident arrays (every index widened to 64 bits); asynchronous on hip_stream.  Any uploaded
   tree, however built, patched or not.  SVO_EINVAL: NULL tree, NULL buffers with n > 0, n < 0; SVO_ESTATE: the tree is
   not uploaded; n == 0 returns SVO_OK without a launch */
int svo_tree_get_blocks_gpu(const svo_tree* t, const int32_t* xyz, int64_t n, uint16_t* ids, void* hip_stream);
/* The voxels the tree stores (its view) inside the box origin .. origin + (nx, ny, nz), listed in HBM as (x, y, z, id): the
   inverse of svo_build_points_gpu, read from the device copy as svo_tree_get_blocks_gpu reads it.  origin == NULL means the
   whole extent (nx, ny, nz are then ignored); otherwise origin >= 0, origin + n <= 4^levels and positive dimensions (no
   wrap: the patch box's rule).  xyz and ids are DEVICE buffers in svo_tree_get_blocks_gpu's layout (three int32 and one
   uint16 per entry) with room for `cap` entries; *n is a HOST value, the exact number of stored voxels in the box, a 64-bit
   count, set on SVO_OK and on the capacity errors below.
   Order: the output is strictly increasing in the point builder's key — 6 bits per level, the top level first, each
   level's slot z<<4 | y<<2 | x of that level's base-4 digits of the coordinates.  That is the order in which
   svo_build_points_gpu holds a list after its sort, and the tree's own depth-first slot order; no sort takes place.
   Count only: xyz == NULL && ids == NULL && cap == 0 writes nothing and returns the count.  Uniform regions are never
   expanded for it: a K_SOLID region contributes the volume of its intersection with the box in closed form (the count of
   a solid 16384^3 root is 2^42).
   The cost follows the tree and the output, never the box's volume: records are reached top down only where their region
   meets the box (one list per depth), every record's total is folded bottom up, the output offsets are handed down as
   exclusive scans over the 64 slots, and the voxels are written by one wavefront per brick and, for K_SOLID regions, one
   lane per voxel that unranks its index digit by digit.  No position is looked up from the root.
   Scratch in HBM, freed on return: 60 B per reached record (a 16-B copy of the record, 16 B for its region's first voxel,
   8 B each for its total and its output offset, and 4 + 8 B for a count and its scan, used twice), 16 B per K_SOLID
   region written from, and hipCUB's scan temporaries.  A count-only call takes 52 B per reached record.
   Any uploaded tree: world-, terrain-, volume- or points-built, patched or not, compacted or not, either view, 1 to 7
   levels, in every layout the patches leave (records with mask 0, full one-material bricks that stayed bricks,
   superseded records, which are never reached).  The tree is only read: host image, ceilings, garbage counts and
   schedules stay as they are.
   SVO_EINVAL: NULL t or n; one of xyz / ids NULL with the other set or with cap > 0; cap < 0; a non-positive dimension; a
   box that leaves the extent.  SVO_ESTATE: the tree is not uploaded.  SVO_ERANGE, with *n set and nothing written: the
   count exceeds 2^31 - 1 when buffers are given, or the count exceeds cap.  SVO_ENOMEM: no scratch.  Arguments and state
   are checked before the first HIP call.
   The call runs on hip_stream and waits for it before returning (the count is a host value); it does not synchronise
   the device. */
int svo_tree_list_voxels_gpu(const svo_tree* t, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                             int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream);
/* List the voxels in which two resident trees differ, on the device: the voxels of the box at which the id that `a` stores
   differs from the id that `b` stores, written as (x, y, z, id_b) in svo_tree_list_voxels_gpu's buffer layout; id_b is 0
   where b stores nothing.  Each tree is read in its own view, from its device copy.  The output is the edit list that
   makes a into b: svo_tree_patch_points_gpu(a, xyz, ids, *n) leaves a's content in the box equal to b's (the ids are b's
   numbers: the patch refuses ids at or beyond a's palette size).  Ids are compared as numbers; the palettes are NOT
   compared, so the same number with different palette entries counts as equal.  The views may differ: a solid-view and a
   full-view tree of one world differ exactly in the liquid voxels.  a == b is allowed and yields 0.
   The box, the order, the count-only call, *n and the buffers follow svo_tree_list_voxels_gpu exactly: origin == NULL is the
   whole extent, else origin >= 0, origin + n <= 4^levels, positive dimensions, no wrap; the output is strictly increasing
   in the point builder's key and no sort takes place, so that the diff of an empty tree against t equals the listing of t
   entry for entry; xyz == NULL && ids == NULL && cap == 0 writes nothing and returns the count; *n is a HOST value, the
   exact 64-bit number of differing voxels, set on SVO_OK and on the capacity errors below.
   Uniform regions are never expanded: two K_SOLID regions, or a K_SOLID region and an empty one, contribute the clipped
   volume of the smaller region in closed form where their ids differ, and nothing, without being descended, where they
   are equal (a solid 16384^3 root against an empty tree counts 2^42).  The two trees are walked side by side, one list of
   pairs of regions per depth in the listing's four phases; a region uniform on both sides is never an item of a list, so
   the items number at most the records reached in a plus those reached in b.  No position is looked up from a root.
   Scratch in HBM, freed on return: 92 B per item (two 16-B record copies, 16 B for the region's first voxel, a 16-B
   link to its children, 8 B each for its total and its offset, 4 + 8 B for a count and its scan, used twice; 84 B for a
   count-only call), 36 B per uniform region written from, and hipCUB's scan temporaries.
   Any uploaded trees of 1 to 7 levels, either view, however built, in every layout the patches leave.  Both trees are only
   read: host images, ceilings, garbage counts and schedules stay as they are.
   SVO_EINVAL: NULL a, b or n; one of xyz / ids NULL with the other set or with cap > 0; cap < 0; a non-positive dimension;
   a box that leaves the extent; trees of different levels; trees on different devices (found after the upload check).
   SVO_ESTATE: either tree is not uploaded.  SVO_ERANGE, with *n set and nothing written: the count exceeds 2^31 - 1 when
   buffers are given, or the count exceeds cap.  SVO_ENOMEM: no scratch.  Arguments and state are checked before the first
   HIP call; after any error the caller's buffers and both trees are untouched.
   The call runs on hip_stream and waits for it before returning; it does not synchronise the device. */
int svo_tree_diff_gpu(const svo_tree* a, const svo_tree* b,
                      const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                      int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream);
/* Patch a resident tree from a dense box of voxels in HBM, on the device: after the call the tree's content inside the
   box is exactly `voxels` (ids the tree's view does not hold are stored empty, as in svo_build_volume_gpu); everything
   outside the box is as before.  Any uploaded tree (volume-, terrain- or world-built), either view, any size (nodes are
   read through 64-bit addresses).  Regions the box does not meet keep their records and subtrees; aligned regions wholly
   inside the box are emitted canonically from the box (svo_build_volume_gpu's class pyramid over the box, whose first
   pass reads the box once and checks the ids); regions the box cuts are re-emitted one level down, in new child blocks
   appended to the arrays, down to bricks classified from their 64 composite voxels (a brick that stores none clears its
   slot bit).  Only one record is rewritten in place: that of the deepest interior node whose region holds the box (the
   anchor).  As after svo_tree_update, the result is the tree's content, not its canonical layout: cut interior regions
   are not re-collapsed when they end up uniform or empty (records with mask 0 may result; traversal is unaffected).  A
   box that is the whole extent is a full build: the arrays restart and nothing stays superseded.
   The device arrays are reallocated (with the slack of a fresh upload) only when the appended tail would not fit; the
   host image, the column ceilings and svo_tree_garbage's counts are brought up to date.  A world-built tree patched
   this way no longer follows its svo_world: svo_tree_update on it returns SVO_ESTATE.
   SVO_EINVAL: a NULL pointer, a non-positive dimension, a box that leaves the extent; SVO_ESTATE: the tree is not
   uploaded, or has host edits not yet synced (svo_tree_sync); SVO_ERANGE: an id >= the tree's palette size (found by
   the first pass: nothing is appended, and the tree is unchanged on host and device), arrays that would pass 2^32
   elements, a tree of one level; SVO_ENOMEM: no scratch.  Arguments are checked before the first HIP call.
   The device is synchronised on entry (the box may come from any stream, and records and ceilings are rewritten in
   place: svo_tree_sync's contract: call it between frames); the call is complete on return.
   Not done here: palette growth (ids are the tree's own palette), and compaction of superseded records
   (svo_tree_garbage tells the caller when svo_tree_compact_gpu pays). */
typedef struct {
    int32_t nx, ny, nz;        /* voxels[((int64)z * ny + y) * nx + x], as svo_volume_desc */
    int32_t origin[3];         /* world position of voxels[0]; origin >= 0, origin + n <= extent (no wrap) */
    const uint16_t* voxels;    /* DEVICE pointer on the tree's device: ids of the tree's own palette, 0 = empty */
} svo_volume_box;
int svo_tree_patch_volume_gpu(svo_tree* t, const svo_volume_box* box);
/* Patch a resident tree from a sparse list of voxel edits in HBM, on the device: n entries (x, y, z, id) in
   svo_tree_get_blocks_gpu's layout — xyz and ids are DEVICE pointers on the tree's device, three int32 and one uint16 per
   entry — applied in list order.  When a voxel is listed more than once its last entry decides.  A last entry of id 0
   erases the voxel (here an id-0 entry is an edit; in svo_build_points_gpu it simply drops out); a last entry whose id the
   tree's view does not hold is stored empty (svo_tree_patch_volume_gpu's rule).  Ids are the tree's own palette: there is
   no palette growth.  After the call every listed voxel holds its resolved entry and every other voxel is as before.
   Any uploaded tree (world-, terrain-, volume- or points-built, patched or not), either view, any size (every node and
   material index is widened to 64 bits before it addresses memory).  The entries are keyed and sorted as in
   svo_build_points_gpu; the descent starts at the deepest interior node whose region holds every edit (the anchor, the
   only record rewritten in place) and re-emits every region an edit lies in one level down, in new child blocks
   appended to the arrays: untouched children are copied (below a K_SOLID region: synthesised K_SOLID records), touched
   bricks are classified from their 64 composite voxels.  As after svo_tree_patch_volume_gpu the result is the tree's
   content, not its canonical layout: touched interior regions are not re-collapsed (records with mask 0 may result), and
   a full one-material brick may stay a brick (svo_tree_compact_gpu restores the layout).  A touched brick that ends up
   storing nothing clears its slot bit in its parent: no K_BRICK record with mask 0 exists.
   The device arrays are reallocated (with the slack of a fresh upload) only when the appended tail would not fit; the
   host image, the column ceilings (exact, over the 16 x 16-column blocks the edits touch), the tree's top row and
   svo_tree_garbage's counts are brought up to date.  A world-built tree patched this way no longer follows its
   svo_world: svo_tree_update on it returns SVO_ESTATE.
   Scratch follows the edits, never the extent or the tree: 24 B per entry for the sort (as in svo_build_points_gpu) and
   12 B for its compaction, 26 B per distinct voxel for the edit list and its column blocks, 44 B per touched region and
   level (at most one region per edit per level), and 16 B per appended record.
   SVO_EINVAL: NULL tree, NULL xyz or ids with n > 0, n < 0; SVO_ERANGE, before the first HIP call: n > 2^31 - 1, a tree
   of one level; SVO_ESTATE: the tree is not uploaded, or has host edits not yet synced (svo_tree_sync); SVO_ERANGE, found
   on the device by the key pass: an id >= the tree's palette size or a coordinate outside [0, 4^levels) (no wrap, as in
   the builder; the message says which of the two it was); SVO_ERANGE: arrays that would pass 2^32 elements; SVO_ENOMEM:
   no scratch.  Everything goes to scratch first: after any error the tree and its garbage counts are unchanged on host
   and device.  n == 0 returns SVO_OK after the argument and state checks, without device work.
   The device is synchronised on entry (the list may come from any stream, and records and ceilings are rewritten in
   place: call it between frames); it runs on the null stream and the call is complete on return. */
int svo_tree_patch_points_gpu(svo_tree* t, const int32_t* xyz, const uint16_t* ids, int64_t n);
/* Patch a resident tree from a list of solid shapes — boxes and balls, each with the id it stores — on the device, at a
   cost that follows the shapes' surfaces and never their volumes: filling 1300^3 voxels of a 16384^3 world appends at
   most 64 records per aligned cell the box cuts (about two million, 32 MB), where a dense box would hold 4.4 GB and an
   edit list 2.2 * 10^9 entries, more than svo_tree_patch_points_gpu takes.  `shapes` is a HOST
   array of n shapes, applied in list order as svo_tree_patch_points_gpu's entries are: after the call a voxel holds the
   id of the last shape that contains it and a voxel inside no shape is as before.  Id 0 erases; an id the tree's view
   does not hold is stored empty (the other patches' rule, resolved per shape on the host).  Ids are the tree's own
   palette: there is no palette growth.  A box must lie within the extent (the patch box's rule); a ball is clipped to it,
   so its centre may lie outside.
   Any uploaded tree (world-, terrain-, volume- or points-built, patched or not), either view, every layout the patches
   leave, any size (every node and material index is widened to 64 bits before it addresses memory).  The descent is
   svo_tree_patch_volume_gpu's, with the box's class pyramid replaced by a closed form: an aligned cell no shape touches
   keeps its record and subtree; a cell wholly inside the deciding shape becomes one K_SOLID record at whatever level it
   sits (for id 0: a clear slot bit); a cell the deciding shape cuts is re-emitted one level down, in new child blocks
   appended to the arrays, down to bricks classified from their 64 composite voxels.  The shape that decides a cell is
   the last in the list that meets it; a cell cut by a late shape and covered by an earlier one therefore descends to
   bricks that come out uniform.  As after the other patches the result is the tree's content, not its canonical layout
   (records with mask 0 may result, full one-material bricks may stay bricks; svo_tree_compact_gpu restores the layout);
   no K_BRICK record with mask 0 exists.  Only one record is rewritten in place: that of the deepest interior node whose
   region holds every shape's clipped bounding box (the anchor).  The arrays restart — the tree becomes a lone K_SOLID
   root, or the lone empty root for id 0, and nothing stays superseded — only when the last shape that meets the extent
   covers all of it; a bounding box equal to the extent does not restart them.
   The device arrays are reallocated (with the slack of a fresh upload) only when the appended tail would not fit; the
   host image, the column ceilings (exact, over one rectangle per shape's clipped column footprint), the tree's top row
   and svo_tree_garbage's counts are brought up to date.  A world-built tree patched this way no longer follows its
   svo_world: svo_tree_update on it returns SVO_ESTATE.
   Scratch in HBM, freed on return: 40 B per shape, 24 + 24 B per cut cell and level (its work item and four scan words), 16 B per appended record.  Every
   cell is asked against every shape: there is no spatial index over the list, so the time is (cut cells) x n.
   All errors are found on the host before the first HIP call, and after any error the tree and its counts are unchanged.
   SVO_EINVAL: NULL tree, NULL shapes with n > 0, n < 0, an unknown kind, a box with a non-positive dimension or one
   that leaves the extent, r2 < 0.  SVO_ERANGE: n > 1024; a ball centre with |c| > 2^20 on an axis or r2 > 2^42 (within
   these limits every distance sum is exact in int64); an id >= the tree's palette size; a tree of one level; arrays that
   would pass 2^32 elements (found once the totals are known, before the tree is touched).  The first shape that fails
   decides, and the message gives its index.  SVO_ESTATE: the tree is not uploaded, or has host edits not yet synced
   (svo_tree_sync); it is checked after the arguments.  SVO_ENOMEM: no scratch.  n == 0, or every shape clipped away,
   returns SVO_OK after these checks without device work.
   The device is synchronised on entry (records and ceilings are rewritten in place: call it between frames); it runs on
   the null stream and the call is complete on return.  svo_tree_patch_times reports it. */
#define SVO_SHAPE_BOX 0  /* voxels a <= p < a + b; b positive; must lie within the extent (the patch box's rule) */
#define SVO_SHAPE_BALL 1 /* voxels with |p - a|^2 <= r2 in exact integers; clipped to the extent; b ignored */
typedef struct {
    int32_t kind;  /* SVO_SHAPE_BOX / SVO_SHAPE_BALL */
    int32_t a[3];  /* box: its first voxel; ball: its centre */
    int32_t b[3];  /* box: its dimensions (x, y, z) */
    int64_t r2;    /* ball: the squared radius, 0 .. 2^42 */
    uint16_t id;   /* the tree's own palette id the shape's voxels store, 0 = erase */
} svo_shape;
int svo_tree_patch_shapes_gpu(svo_tree* t, const svo_shape* shapes /* HOST */, int32_t n);
/* Paste a box of one resident tree (src) into another (dst), on the device, without going through the voxels: copy,
   paste, move and stamp for prefabs, regions of a world and snapshots.  For every voxel p of the box, q = dst_origin + p
   and s = src(src_origin + p), read from src's device copy in src's own view (a voxel src does not store reads as 0).
   SVO_PASTE_REPLACE: q takes s.  SVO_PASTE_KEEP_EMPTY: q takes s where s != 0 and is unchanged elsewhere (a prefab's air
   is transparent).  The mode is decided on src's id first; only then is the id resolved against dst's view: an id dst's
   view does not hold is stored empty (the other patches' rule), so pasting into the solid-view tree and into the
   full-view tree of one world leaves them the two views of one pasted world.  Every voxel outside the destination box is
   as before.  Ids are numbers in dst's palette and the palettes are not compared (svo_tree_diff_gpu's rule); there is no
   palette growth.
   src_origin == NULL means src's whole extent (nx, ny, nz are then ignored).  Both boxes must lie within their tree's
   extent, with positive dimensions and no wrap.  The trees may have different levels: src 1 to 7, dst at least 2 (the
   patches' rule).  The offset dst_origin - src_origin is arbitrary: it need not be a multiple of 4.  src == dst is
   allowed and the boxes may overlap: everything is read from the arrays as they were on entry and written to scratch
   first, as in every patch, so a self-paste copies the old content, never half-pasted content.  src is only ever read.
   The descent is svo_tree_patch_shapes_gpu's, asked per aligned destination cell how it stands to src: the cell is
   clipped to the box and shifted into src, where it meets at most 2 x 2 x 2 aligned src cells of its own width, each
   found by a walk from src's root (a K_SOLID record at or above it: uniform; a clear slot bit at or above it: empty; a
   record at its own level: mixed).  A cell outside the box, or (KEEP_EMPTY) over nothing src stores, keeps its record and
   subtree; a cell wholly inside the box over src cells of one id becomes one K_SOLID record at whatever level it sits
   (for id 0: a clear slot bit); every other cell is re-emitted one level down, in new child blocks appended to the arrays,
   down to bricks classified from their 64 composite voxels.  The answer is conservative: a mixed src cell whose
   overlapping part happens to be uniform descends and comes out right below, and a full one-material brick that stayed a
   brick or an interior record with mask 0 in src counts as mixed.  A cell is cut only where the box's surface cuts it or
   a src record of its level overlaps it, so the work follows the box's surface plus at most 8 destination cells per src
   record reached in the box, never the volume: a 1300^3 K_SOLID region pastes at the cost of its faces.
   As after the other patches the result is dst's content, not its canonical layout (records with mask 0 may result, full
   one-material bricks may stay bricks; svo_tree_compact_gpu restores the layout); no K_BRICK record with mask 0 exists.
   Only one record is rewritten in place: that of the deepest interior node whose region holds the destination box (the
   anchor).  A REPLACE paste whose destination box is the whole extent restarts the arrays and nothing stays superseded
   (the volume patch's rule; with src == dst too: the scratch is complete before the commit); KEEP_EMPTY never restarts.
   The device arrays are reallocated (with the slack of a fresh upload) only when the appended tail would not fit; the
   host image, the column ceilings (exact, over the destination box's column footprint), the tree's top row and
   svo_tree_garbage's counts are brought up to date.  A world-built dst no longer follows its svo_world: svo_tree_update
   on it returns SVO_ESTATE.
   Scratch in HBM, freed on return: 4 B per 32 palette entries, 24 + 24 B per cut cell and level, 16 B per appended record.
   All errors below but the last two are found on the host before the first HIP call: arguments first, then state, then
   the anchor.  After any error both trees and dst's garbage counts are unchanged on host and device.
   SVO_EINVAL: NULL dst, src or dst_origin; unknown flag bits; a non-positive dimension; either box leaving its extent.
   SVO_ERANGE: a dst of one level; src's palette holds more entries than dst's (so no id can be out of range on the
   device); arrays that would pass 2^32 elements (found once the totals are known, before dst is touched).
   SVO_ESTATE: either tree is not uploaded, the trees are on different devices, or either has host edits not yet synced
   (svo_tree_sync).  SVO_ENOMEM: no scratch.
   The device is synchronised on entry (records and ceilings are rewritten in place: call it between frames); it runs on
   the null stream and the call is complete on return.  svo_tree_patch_times reports it.
   Rotation, mirroring and id remapping are svo_tree_patch_tree_oriented_gpu's, below.  Not done here or there: lists of
   placements in one call. */
#define SVO_PASTE_REPLACE 0     /* the box of dst becomes the box of src, empties included */
#define SVO_PASTE_KEEP_EMPTY 1  /* voxels at which src stores nothing leave dst as it is (a prefab's air is transparent) */
int svo_tree_patch_tree_gpu(svo_tree* dst, const svo_tree* src,
                            const int32_t src_origin[3], int32_t nx, int32_t ny, int32_t nz,
                            const int32_t dst_origin[3], uint32_t flags);
/* The same paste turned, mirrored and with its ids remapped: a prefab built as its own small tree, with its own palette,
   stamped in any of the 48 axis-aligned orientations.  svo_tree_patch_tree_gpu is the case axis = {0, 1, 2},
   flip = {0, 0, 0}, id_map = NULL of this call, and keeps its own entry point.
   Content.  The destination box is dst_origin + [0, dn) with dn[a] = n[axis[a]].  A voxel q of it has d = q - dst_origin
   and reads src at s, where s[axis[a]] = src_origin[axis[a]] + (flip[a] ? n[axis[a]] - 1 - d[a] : d[a]): dst's axis a runs
   along src's axis axis[a], against it where flip[a] is 1.  All 48 signed permutations are valid; the 24 of determinant
   +1 are the rotations, the others mirrorings.  The id goes through four steps in this order: (1) src's id in src's own
   view (a voxel src does not store reads 0); (2) id_map[id] when a map is given; (3) the mode, decided on the mapped id:
   under SVO_PASTE_KEEP_EMPTY a material mapped to 0 is transparent, under SVO_PASTE_REPLACE it erases; (4) dst's view: an
   id it does not hold is stored empty.  id_map is a HOST array with one entry per entry of src's palette (svo_tree_get_info's
   n_materials of src), each an id of dst's palette; id_map[0] must be 0.  A map lifts the plain paste's rule that src's
   palette be no larger than dst's: the map is the check.  There is still no palette growth: the ids mapped to must exist
   in dst's palette.
   Everything else is svo_tree_patch_tree_gpu's contract: src_origin and n as there, except that the whole of src is given
   by its extent (there is no NULL origin in the struct); src == dst with overlapping boxes reads the content as it was
   on entry, so a region can be rotated in place; a REPLACE paste whose destination box is the whole extent restarts the
   arrays; one anchor record is rewritten in place; the host image, the ceilings over the destination box's footprint, the
   top row and svo_tree_garbage's counts are brought up to date; svo_tree_patch_times reports the call; it synchronises on
   entry and is complete on return.  The cost is the plain paste's: an orientation maps an aligned cell of cs voxels per
   axis to a box of cs voxels per axis in src, which still meets at most 2 x 2 x 2 aligned src cells, so the work follows
   the box's surface, never its volume.  The map is applied to what the walks return before cells are compared, so two src
   cells of different ids that map to one id are one uniform region, and a region mapped to 0 is skipped under KEEP_EMPTY.
   Scratch in HBM, freed on return: the plain paste's, and 2 B per entry of src's palette for the map.
   All errors but the plain paste's last two are found on the host before the first HIP call: arguments first, then state.
   After any error both trees are unchanged on host and device.
   SVO_EINVAL: NULL dst, src or p; unknown flag bits; axis not a permutation of 0, 1, 2; a flip entry other than 0 or 1; a
   non-positive dimension; either box leaving its extent (64-bit sums, no wrap); id_map[0] != 0.
   SVO_ERANGE: a dst of one level; with a map, an entry >= dst's palette size (the message names the first such index);
   without one, src's palette larger than dst's.  SVO_ESTATE, SVO_ENOMEM: as the plain paste.
   Not done here: lists of placements in one call, palette growth. */
typedef struct {
    int32_t src_origin[3];   /* first voxel of the box in src */
    int32_t n[3];            /* its dimensions along src's x, y, z; positive */
    int32_t dst_origin[3];   /* first voxel of the destination box in dst */
    uint32_t flags;          /* SVO_PASTE_REPLACE / SVO_PASTE_KEEP_EMPTY, no other bit */
    uint8_t axis[3];         /* dst axis a runs along src axis axis[a]: a permutation of 0, 1, 2 */
    uint8_t flip[3];         /* 0 or 1; 1: dst axis a runs against src axis axis[a] */
    const uint16_t* id_map;  /* HOST array, one entry per entry of src's palette, or NULL (ids unchanged) */
} svo_paste;
int svo_tree_patch_tree_oriented_gpu(svo_tree* dst, const svo_tree* src, const svo_paste* p);
/* The oriented paste under a rule over both sides: the two calls above decide every voxel from src alone, this one also
   asks what dst holds, so a prefab can fill only air (UNDER), recolour only what is solid (PAINT), carve (ERASE), or act as
   a mask, a stencil or a symmetric difference.  p gives the geometry, the orientation and the id map exactly as for
   svo_tree_patch_tree_oriented_gpu; p->flags must be 0, because the rule replaces it.
   For each voxel q of the destination box: s is src's id read through the orientation and then id_map (steps (1) and (2)
   above); d is the id dst stores at q on entry, IN DST'S OWN VIEW; R(s) is s resolved against dst's view (an id the view
   does not hold is stored empty).  The rule says what q holds afterwards in the three cases that are not trivially empty:
                                       SVO_RULE_KEEP   SVO_RULE_TAKE   SVO_RULE_CLEAR
     A "src only"  s != 0, d == 0           0              R(s)         not allowed
     B "both"      s != 0, d != 0           d              R(s)              0
     C "dst only"  s == 0, d != 0           d           not allowed          0
   and s == 0, d == 0 stays 0.  rule = SVO_RULE(A, B, C) = A | B << 2 | C << 4: 12 rules, the useful ones named below.
   SVO_RULE_OVER has SVO_PASTE_KEEP_EMPTY's content and SVO_RULE_REPLACE has SVO_PASTE_REPLACE's.  Rule 0 keeps everything:
   it returns SVO_OK after the argument and state checks, without device work.
   Because d is read in dst's own view, a rule whose outcome depends on d, pasted into the solid-view tree and into the
   full-view tree of one world, does NOT leave them the two views of one pasted world: a liquid voxel is d == 0 in the solid
   view, so SVO_RULE_UNDER of a solid material over water stores the solid in the solid-view tree and keeps the water in the
   full-view tree.
   Every voxel outside the destination box is as before; with src == dst and overlapping boxes everything is read as it was
   on entry; src is only read.  The call never restarts the arrays, whatever the rule and the box (svo_tree_compact_gpu
   exists).  Everything else is the oriented paste's contract: one anchor record is rewritten in place; the host image, the
   ceilings over the destination box's footprint, the top row and svo_tree_garbage's counts are brought up to date;
   svo_tree_patch_times reports the call; it synchronises on entry and is complete on return.
   Cost.  The descent is the paste's, with one more walk per cell: the destination cell itself is looked up in dst (uniform,
   empty, or a record at its level), and the two answers are combined.  Uniform against uniform is decided at the cell.  A
   cell is re-emitted one level down only where the box's surface cuts it, where a src record of its level overlaps it, or,
   for rules whose outcome depends on d, where dst holds a record of its level under a non-empty src region; where the rule
   keeps whatever dst holds the cell keeps its record and subtree.  The work follows surfaces and records, never the volume.
   Scratch in HBM: the oriented paste's.
   Errors are found on the host before the first HIP call, arguments first, then state; after any error both trees are
   unchanged on host and device.
   SVO_EINVAL: NULL dst, src or p; p->flags != 0; a rule with a bit above 5, with A not KEEP or TAKE, B == 3, or C not KEEP
   or CLEAR; and the oriented paste's own cases (axis, flip, dimensions, either extent, id_map[0] != 0).
   SVO_ERANGE, SVO_ESTATE, SVO_ENOMEM: as the oriented paste.
   Not done here: lists of placements in one call, palette growth. */
#define SVO_RULE_KEEP 0u  /* the voxel stays as dst has it (case A: empty) */
#define SVO_RULE_TAKE 1u  /* the voxel takes src's mapped id, resolved against dst's view (cases A and B) */
#define SVO_RULE_CLEAR 2u /* the voxel becomes empty (cases B and C) */
#define SVO_RULE(a, b, c) ((uint32_t)(a) | (uint32_t)(b) << 2 | (uint32_t)(c) << 4)
#define SVO_RULE_UNDER 1u    /* (TAKE, KEEP, KEEP): fill only air */
#define SVO_RULE_PAINT 4u    /* (KEEP, TAKE, KEEP): recolour only what is solid */
#define SVO_RULE_OVER 5u     /* (TAKE, TAKE, KEEP): src where it stores something (KEEP_EMPTY's content) */
#define SVO_RULE_ERASE 8u    /* (KEEP, CLEAR, KEEP): carve src's silhouette out of dst */
#define SVO_RULE_XOR 9u      /* (TAKE, CLEAR, KEEP): the symmetric difference */
#define SVO_RULE_MASK 32u    /* (KEEP, KEEP, CLEAR): keep dst only inside src's silhouette */
#define SVO_RULE_STENCIL 36u /* (KEEP, TAKE, CLEAR): src's ids inside the intersection, nothing else */
#define SVO_RULE_REPLACE 37u /* (TAKE, TAKE, CLEAR): the box of src, empties included (REPLACE's content) */
int svo_tree_patch_tree_rule_gpu(svo_tree* dst, const svo_tree* src, const svo_paste* p, uint32_t rule);
/* node records and material entries superseded by edits (svo_tree_update, svo_tree_patch_volume_gpu,
   svo_tree_patch_points_gpu, svo_tree_patch_shapes_gpu, svo_tree_patch_tree_gpu, svo_tree_patch_tree_oriented_gpu,
   svo_tree_patch_tree_rule_gpu) since the last full build: still in the arrays, no longer reachable (either may be NULL) */
int svo_tree_garbage(const svo_tree* t, uint64_t* nodes, uint64_t* mats);
/* diagnostics (tools/volume_patch_timing.py, tools/points_patch_timing.py): host-clock milliseconds of the tree's last
   svo_tree_patch_volume_gpu, svo_tree_patch_points_gpu, svo_tree_patch_shapes_gpu or svo_tree_patch_tree_gpu (or its oriented
   and rule forms), whichever ran last, after its entry
   synchronisation: ms[0] the device passes (volume: pyramid, count and write passes into scratch; points: keys, sort, edit
   list, column blocks, count and write passes; shapes and tree: the table's upload, the host's garbage walk, count and
   write passes), ms[1] the commit to the arrays and the copy back to the host image, ms[2] the host's ceiling update
   (with the tree's top row) */
int svo_tree_patch_times(const svo_tree* t, double ms[3]);
/* Re-emit an uploaded tree, on its device, as the canonical linearisation of its own content: after the call the node
   array, the material runs, nodes_per_level, n_bricks and n_mat_bytes equal, byte for byte, what svo_build_volume_gpu
   emits for the same content under the same palette and view (for a tree that still follows an svo_world: what
   svo_build_view emits for that world).  Uniform regions are K_SOLID at the highest level at which they are uniform,
   empty regions clear their slot bit (no K_INTERIOR record with mask 0 but the lone root of an empty tree), a full
   one-material brick is a K_SOLID child, a partial one K_BRICK | K_UNIFORM without a material run; svo_tree_garbage
   reports (0, 0).  Only the tree is read — reachable records top down, their classes bottom up, then the builders' own
   emitter — so the cost follows the tree's size, not the extent's volume.
   The device arrays are new allocations with the slack of a fresh upload and the old ones are freed (device_bytes is
   that of a freshly built tree of the same content); the host image mirrors them.  Unchanged: the palette (ids are not
   renumbered, unused entries stay), view and levels; the content, hence the column ceilings, which are kept and not
   recomputed; the guard-trip counter, the AO plan and the frame schedules; whether svo_tree_update accepts the tree (a
   world-built tree edited only through svo_tree_update still follows its world afterwards; one patched by
   svo_tree_patch_volume_gpu still gets SVO_ESTATE).
   SVO_EINVAL: NULL tree; SVO_ESTATE: the tree is not uploaded, or has host edits not yet synced (svo_tree_sync);
   SVO_ENOMEM: no scratch — everything is emitted beside the old arrays and swapped in at the end, so the tree is then
   untouched on host and device.  Arguments are checked before the first HIP call.  The device is synchronised on entry
   (the arrays are replaced: call it between frames); the call is complete on return.  Trees of any size (every index
   is widened to 64 bits before it addresses memory); trees of one level and lone roots return SVO_OK.  The caller
   decides when: svo_tree_patch_volume_gpu never compacts by itself. */
int svo_tree_compact_gpu(svo_tree* t);
/* diagnostics (tools/volume_compact_timing.py): host-clock milliseconds of the tree's last svo_tree_compact_gpu, after its
   entry synchronisation: ms[0] the device passes (reach, classes, emission into the new arrays), ms[1] the copy back
   to the host image and the swap, ms[2] the release of the scratch allocations and of the old host image */
int svo_tree_compact_times(const svo_tree* t, double ms[3]);
int svo_tree_get_info(const svo_tree* t, svo_tree_info* out);
/* palette entry `id` (id 0 = empty block) */
int svo_tree_palette(const svo_tree* t, uint32_t id, svo_block* out);
/* host-side lookup in the linearised tree; returns the solid-view block (empty for LIQUID) */
int svo_tree_get_block(const svo_tree* t, int32_t x, int32_t y, int32_t z, svo_block* out, uint32_t* material_id);
/* batched host lookup: palette ids (0 = empty) of n positions */
int svo_tree_get_blocks(const svo_tree* t, const int32_t* xyz, int64_t n, uint32_t* material_ids);
/* diagnostics: index of the deepest node a lookup of each voxel reads (the brick / SOLID node holding
   it, or the interior node whose child slot for it is empty) */
int svo_tree_node_indices(const svo_tree* t, const int32_t* xyz, int64_t n, uint64_t* node_index);
/* copy the host image out (for tests / serialisation); byte sizes from svo_tree_get_info */
int svo_tree_export(const svo_tree* t, void* nodes, uint64_t nodes_bytes, void* mats, uint64_t mats_bytes);
/* updateSsboData analogue: (re)upload the image to HBM of `device` (with room for edit blocks) */
int svo_upload(svo_tree* t, int32_t device);
/* Incremental edits: after putBlock / deleteBlock at `level` on the n positions
   xyz of `w` (the world `t` was built from), patch `t` in place: each edited region's subtree is
   re-linearised from `w` and its parent's child block rewritten at the end of the array (only
   that parent's 16-B record changes in place).  The content equals a fresh svo_build of `w`; the
   layout is not re-collapsed, and the tree is rebuilt from `w` when superseded blocks exceed half
   of it.  Host only; svo_tree_sync brings the device copy up to date. */
int svo_tree_update(svo_tree* t, const svo_world* w, const int32_t* xyz, int64_t n, int32_t level);
/* upload what svo_tree_update changed: the appended tail and the rewritten records (or everything
   after a rebuild / when the device allocation is outgrown).  Synchronises the device first (device
   memory is rewritten in place): call it between frames, as updateSsboData is (main.cpp:212). */
int svo_tree_sync(svo_tree* t);
void svo_tree_destroy(svo_tree* t);
/* The column ceilings the casts use (SVO_CAST_NO_CEILINGS): for k = SVO_CEIL_K0 .. min(levels - 1, SVO_CEIL_K0 + 3)
   (blocks of 16, 64, 256 and 1024 columns), per aligned block of 4^k x 4^k columns, the highest stored voxel row of
   the tree in those columns (-1: none), row-major [z][x], level after level (finest first; level j's blocks are
   4^(SVO_CEIL_K0 + j) columns wide).  out may be NULL (count only); levels = number of levels, n = elements. */
#define SVO_CEIL_K0 2
int svo_tree_ceilings(const svo_tree* t, int16_t* out, int64_t cap, int32_t* levels, int64_t* n);
/* The pairs the casts read: level j's block ceiling with that of the level min(j + SVO_CEIL_PAIR_STEP, levels - 1)
   block holding it (primary casts and shadow rays check levels 0 and SVO_CEIL_PAIR_STEP of the table) */
#define SVO_CEIL_PAIR_STEP 1
/* the ceiling layout this library was built with: SVO_CEIL_K0 and SVO_CEIL_PAIR_STEP (either may be NULL) */
int svo_ceiling_layout(int32_t* k0, int32_t* pair_step);
/* The column-ceiling tables in HBM as the casts read them (inspection / tests): the int16 ceilings in
   svo_tree_ceilings' layout and their uint32 pairs (low: the block's ceiling, high: the ceiling of the level
   j + SVO_CEIL_PAIR_STEP block holding it, the coarsest level there is).  levels = 0 when the tree has none.
   Either buffer may be NULL. */
int svo_tree_device_ceilings(const svo_tree* t, int16_t* ceil, uint32_t* pairs, int64_t cap, int32_t* levels, int64_t* n);
/* The per-level quads in HBM (the shading pass's walk over every ceiling level): for every block of the finest
   level (4^SVO_CEIL_K0 columns, row-major [z][x]), the ceilings of the blocks of levels 0..3 holding it, int16 each,
   level j in bits 16j..16j+15 (a level the tree lacks: 0x7FFF).  quads may be NULL (count only); n = elements. */
int svo_tree_device_ceiling_quads(const svo_tree* t, uint64_t* quads, int64_t cap, int64_t* n);
/* The fine ceilings, one level below svo_tree_ceilings' finest: per aligned block of 4^(SVO_CEIL_K0 - 1) columns (one
   brick's footprint) the highest stored voxel row (-1: none), int16 row-major [z][x]; shift = log2 of the block's
   width.  The march before the traversal loop descends onto them.  A tree without ceiling levels has none (n = 0).
   2 bytes per 16 columns: 2 MB for a 4096-voxel world, 32 MB for a 16384-voxel one.  svo_tree_ceilings_fine computes
   them from the host tree; svo_tree_device_ceilings_fine reads the table in HBM.  out / fine may be NULL (count only). */
int svo_tree_ceilings_fine(const svo_tree* t, int16_t* out, int64_t cap, int32_t* shift, int64_t* n);
int svo_tree_device_ceilings_fine(const svo_tree* t, int16_t* fine, int64_t cap, int64_t* n);
/* The frame schedule of (hip_stream, kind: 2 shading; 0 / 1, primary and AO casts, keep none) over t (inspection /
   tests; SVO_CAST_NO_SCHEDULE): the dispatch order of the next frames of that geometry, by groups of SVO_SCHED_GROUP
   consecutive blocks (order[slot group] = frame group; n / SVO_SCHED_GROUP entries) and the block durations of the frame
   it was sorted from (100 MHz ticks, n entries); n = blocks (0: no schedule yet).  Either buffer may be NULL;
   synchronises hip_stream. */
int svo_tree_schedule(const svo_tree* t, void* hip_stream, int32_t kind, uint32_t* order, uint32_t* cost, int64_t cap, int64_t* n);
/* Checkpoint (the reference regenerates its world at every start, main.cpp:190): write the
   linearised tree (levels, view, palette, nodes, material runs; a checksum) to `path`, and read it back
   as a new tree (not uploaded).  Loading validates every child / material reference against the array
   sizes, so a damaged file fails with SVO_EIO instead of reaching a kernel. */
int svo_tree_save(const svo_tree* t, const char* path);
int svo_tree_load(const char* path, svo_tree** out);

/* ---------------------------------------------------------------------------- casting ------- */
/* Hit record per ray (caller-owned device buffers, 24 B / ray):
     pos_steps[4*i .. 4*i+3] = {x, y, z, stepsLeft}   (RayResult.pos / .steps)
     t[i]                    = deltaPos[axis] before its last increment (entry distance of pos)
     info[i]                 = bit 31 hit | bits 16-17 last axis (3 = no step) | bit 18 step < 0
                               on that axis | bits 0-15 material id (0 = none)
   RayResult.lastPos = pos - (axis step).  Frame rays: index = row * width + px, rows counted
   from the bottom (gl_FragCoord), restricted to the tile rows of this shard.
   Hemisphere AO (light_scattering.frag:133-236): for a hit, ao_samples rays
   start at the centre of lastPos, directions = svo_hemisphere's table with its pole (component 2)
   turned to the hit face's normal by a signed axis permutation (pole -> normal axis, components
   0/1 -> the next two axes cyclically), each cast with castRayFromCam semantics and ao_steps
   steps; ao[i] = number of them that hit. */
typedef struct {
    int32_t* pos_steps;
    float* t;
    uint32_t* info;
    uint8_t* ao;       /* per ray: AO rays that hit (0..ao_samples); required when ao_samples > 0 */
} svo_hits;

typedef struct {
    /* frame mode (ray_dirs == NULL): one primary ray per pixel, low_res.frag:264-288 */
    float origin[3];   /* cameraPos (also the origin of explicit rays when ray_origins == NULL) */
    float cam_dir[3];  /* normalised cameraDir */
    int32_t width, height;
    float ppx, ppy;    /* projPlaneSize uniform (main.cpp:94); see svo_proj_plane */
    int32_t tile_row_start, tile_row_step; /* shard: 8-pixel tile rows start, start+step, ... */
    /* explicit mode: n_rays rays, device float3 arrays */
    const float* ray_dirs;
    const float* ray_origins; /* optional */
    int32_t n_rays;
    int32_t steps;     /* DDA step budget per ray (castRayFromCam's `steps`) */
    int32_t flags;     /* SVO_CAST_* bits, 0 = default */
    int32_t ao_samples; /* hemisphere AO rays per primary hit (0 = off, <= 64; reference: 20) */
    int32_t ao_steps;   /* DDA budget of each AO ray (reference: 5, light_scattering.frag:231) */
    uint64_t* stats;   /* optional device u64[SVO_STATS_HEADER] accumulating per-launch counters when
                          flags & SVO_CAST_STATS: rays, lookups, node loads, cell skips,
                          skips that ran out of budget, brick voxel steps, plain voxel steps,
                          lane work units, wave-max work units x 64, crossings by box cell
                          size (4 slots), brick visits, wave-level loop iterations,
                          wave-level brick voxel steps, loop iterations that took no DDA
                          step and were ended by the progress guard (0 unless a count is wrong),
                          lookups started at
                          the root, lookups answered by the cached parent, wave-level
                          crossings, wave-level descent levels, lookups restarted from the
                          per-lane path, node loads of the AO plan's brick lookups;
                          then 2 stamps per block (svo_cast_blocks);
                          then, with SVO_CAST_STATS in frame mode, one word per
                          output pixel: lookups | brick steps << 32
                          (SVO_CAST_STATS or SVO_CAST_TIMELINE) */
    /* frame mode, several frames in one launch (the multi-GPU step: one launch per rank covers its
       tile rows of every frame): n_frames <= SVO_MAX_FRAMES (0 or 1: one frame at `origin`);
       frame_origins = host array of n_frames camera positions (origin is then ignored).  Records
       of frame f follow those of frame f-1: svo_cast_count / svo_cast_blocks count all frames. */
    int32_t n_frames;
    const float* frame_origins;
} svo_cast_desc;

#define SVO_MAX_FRAMES 16

/* svo_cast_desc.flags: take every DDA step one at a time (disables the exact closed-form crossing
   of empty regions; results are identical — for testing and A/B timing) */
#define SVO_CAST_ITERATIVE 1
/* svo_cast_desc.flags: accumulate traversal counters into svo_cast_desc.stats (diagnostics) */
#define SVO_CAST_STATS 2
/* svo_cast_desc.flags, scheduling (results identical): frames are dispatched top tile row first
   (longest rays first); this bit restores bottom-first order */
#define SVO_CAST_BOTTOM_FIRST 4
/* svo_cast_desc.flags: write per-block start/end stamps (100 MHz) to stats[SVO_STATS_HEADER + 2*block] only;
   stats must hold SVO_STATS_HEADER + 2 * svo_cast_blocks() [+ pixels with SVO_CAST_STATS] words */
#define SVO_STATS_HEADER 32
#define SVO_CAST_TIMELINE 32
/* (bits 16 and 1024 were round-2 dispatch experiments, XCD-contiguous bands and horizon-first row order:
   measured slower or equal, removed) */
/* svo_cast_desc.flags, AO (results identical): trace every AO ray through the tree instead of the
   per-face voxel plan (A/B reference path) */
#define SVO_CAST_AO_TRACE 128
/* svo_cast_desc.flags, scheduling (results identical): in frame mode each wavefront (one block)
   covers 16x4 pixels of its 8-pixel tile row; these bits select 8x8 or 32x2 instead.  A small launch (a
   strong-scaling shard: whole footprints would make fewer than 20480 wavefronts) casts its first-dispatched tile rows
   by half footprints, 32 pixels per wavefront; svo_cast_blocks counts those wavefronts too */
#define SVO_CAST_TILE_8X8 256
#define SVO_CAST_TILE_32X2 512
/* svo_cast_desc.flags (results identical): read nodes through 64-bit addresses even when the tree is
   small enough for 32-bit buffer offsets (trees of more than 2^28 nodes always use them) */
#define SVO_CAST_WIDE_ADDR 2048
/* svo_cast_desc.flags (results identical): the kernel instance picks itself by the origins — from
   integral or half-integral origins every ray's crossings are exact linear sums; other rays cross
   empty regions in exact segments.  SEGMENTS forces the segment-capable instance for any origin */
#define SVO_CAST_SEGMENTS 4096
/* svo_cast_desc.flags (results identical): frames whose rays all step with the same signs run an
   instance with those signs compiled in; this bit keeps the per-wave sign flags instead */
#define SVO_CAST_NO_OCTANT 16384
/* svo_cast_desc.flags (results identical): rays above the highest stored row of the column block they are in
   (primary casts: 16- and 64-column blocks; the shading pass: 64 and 256) cross the empty box above that row in
   one move, without a tree lookup (column ceilings, svo_tree_ceilings, computed at upload / sync); this bit walks
   the tree instead */
#define SVO_CAST_NO_CEILINGS 32768
/* svo_cast_desc.flags, scheduling (results identical): shaded frames (svo_shade_rays) of more than
   SVO_SCHED_MIN_BLOCKS blocks are dispatched longest block first, by the block durations a recent frame of the same
   geometry measured on the same stream (frame-to-frame coherence; a small sort kernel after every 4th frame orders the
   next ones, used while the camera stays within 0.5 deg / 1 voxel of the frame sorted); the first frame of a geometry
   runs in the default order.  This bit keeps the default order (and leaves the
   schedule untouched).  Primary casts always run in the default order (their longest waves are its first) */
#define SVO_CAST_NO_SCHEDULE 65536
#define SVO_SCHED_MIN_BLOCKS 4096
#define SVO_SCHED_GROUP 4 /* the schedule orders groups of this many consecutive blocks (frames of a multiple of it) */

/* number of rays a desc produces on this shard (= records written) */
int svo_cast_count(const svo_cast_desc* d, int64_t* n);
/* number of blocks (64-lane wavefronts) a cast of this desc launches */
int svo_cast_blocks(const svo_cast_desc* d, int64_t* n);
/* asynchronous on hip_stream */
int svo_cast_rays(const svo_tree* t, const svo_cast_desc* d, const svo_hits* out, void* hip_stream);
/* RAY_CASTER::castRayFromCam with explicit camera (synchronous, one ray on the GPU) */
int svo_cast_ray_from_cam(const svo_tree* t, const float pos[3], const float dir[3], int32_t steps, svo_ray_result* out,
                          svo_block* block);
/* Launches over t whose rays ended on the traversal's progress guard (an iteration that took no DDA step:
   only a wrong crossing count can cause it).  Such a ray's record has stepsLeft = -1 and no hit; the count
   should be 0 (shading launches count on t, the tree their shadow rays walk).  reset != 0 zeroes the counter.
   Synchronous: waits for the whole device (launches on any stream), then reads device memory. */
int svo_tree_guard_trips(const svo_tree* t, uint64_t* trips, int32_t reset);
/* the same pick ray, stream-ordered and without a host round trip: the result (svo_ray_result, 28 B) is
   written to d_result, device memory aligned to 16 bytes, on hip_stream (two small launches) — for the
   per-frame lookingAtBlock ray (main.cpp:81,89; svo_shade_desc.look_at_dev).  The block is not returned. */
int svo_cast_ray_from_cam_async(const svo_tree* t, const float pos[3], const float dir[3], int32_t steps, svo_ray_result* d_result,
                                void* hip_stream);
int svo_sync(void* hip_stream);

/* Wire formats of hit records for the exchange between GPUs (the tile-row gather):
   12 B (any desc)  int16 dx, dy, dz   pos - trunc(origin of the ray's frame, or of the explicit ray)
                    uint16 info16      hit << 15 | axis << 13 | (step < 0) << 12 | material id (12 bits)
                    float t
   8 B (compact)    u64: n_x | n_y << 15 | n_z << 30 | hit << 45 | axis << 46 | material id << 48, n_k = the DDA
                    steps the ray took on axis k.  Used for frame descs whose every camera position is integral
                    or half-integral: the receiver regenerates each pixel's ray and recovers the step signs,
                    the position, the steps left and t exactly (every crossing sum from such origins is exact).
   stepsLeft is not sent: every DDA step moves one axis by one voxel, so a hit leaves
   steps - |dx| - |dy| - |dz| and a miss 0.  Both need steps <= 32767 and at most 4096 palette entries
   (SVO_ERANGE otherwise).  svo_wire_bytes gives a desc's record size (8 or 12).  d describes the
   records (svo_cast_count of them, the frames / origins and tile rows they were cast from); wire and
   hits are device buffers; asynchronous. */
#define SVO_WIRE_BYTES 12 /* the larger of the two */
int svo_wire_bytes(const svo_tree* t, const svo_cast_desc* d, int32_t* bytes);
int svo_hits_pack(const svo_tree* t, const svo_cast_desc* d, const svo_hits* hits, void* wire, void* hip_stream);
int svo_hits_unpack(const svo_tree* t, const svo_cast_desc* d, const void* wire, const svo_hits* hits, void* hip_stream);
/* svo_cast_rays writing the wire record of each ray (svo_wire_bytes(d) bytes, record order) instead of its hit
   record — the cast and the pack in one pass; ao: the AO counts as svo_hits.ao (when d->ao_samples > 0) */
int svo_cast_wire(const svo_tree* t, const svo_cast_desc* d, void* wire, uint8_t* ao, void* hip_stream);
/* decode the wire records of the shard d describes (tile rows tile_row_start, +tile_row_step, ... of its
   n_frames frames) into whole frames: frames holds n_frames x width x height records in pixel order (the
   layout of an unsharded svo_cast_rays); only this shard's pixels are written.  ao: AO counts in record
   order (or NULL) */
int svo_wire_scatter(const svo_tree* t, const svo_cast_desc* d, const void* wire, const uint8_t* ao, const svo_hits* frames,
                     void* hip_stream);

/* ------------------------------------------------------------- multi-GPU frame exchange ----- */
/* frames sharded by interleaved 8-pixel tile rows (svo_cast_desc.tile_row_start = rank,
   tile_row_step = nranks), each frame's shards gathered over RCCL to the rank that displays it.  RCCL
   is bound at run time (librccl.so.1; the instance already in the process, e.g. torch's, if any). */
typedef struct svo_exchange svo_exchange;
#define SVO_NCCL_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: call on one rank and hand the bytes to every rank */
int svo_nccl_unique_id(void* out);
/* a communicator of nranks ranks (ncclCommInitRank; every rank calls it), this rank's GPU `device` */
int svo_exchange_create(int32_t nranks, int32_t rank, const void* unique_id, int32_t device, svo_exchange** out);
/* an exchange over a communicator the caller owns (an ncclComm_t of the same RCCL instance) */
int svo_exchange_wrap(void* nccl_comm, int32_t device, svo_exchange** out);
void svo_exchange_destroy(svo_exchange* x);
int svo_exchange_info(const svo_exchange* x, int32_t* rank, int32_t* nranks);
/* One step's exchange.  d: this rank's shard of n_frames frames (as cast into `mine`, records of frame f
   after those of frame f-1); frame f is displayed by rank f % nranks.  Packs `mine` into wire records
   (svo_hits_pack; AO counts alongside when d->ao_samples > 0), sends every frame's shard to its
   display rank and receives the shards of the frames this rank displays — one RCCL group of
   point-to-point transfers: a gather for one frame, an all-to-all for nranks frames — then unpacks them
   into frames_out: the whole frames (width x height records each, the layout of an unsharded
   svo_cast_rays) of frames rank, rank + nranks, ... in that order (unused on ranks that display none).
   This rank's own shards of its frames never travel.  Returns SVO_EINVAL when t lives on another device.
   Asynchronous on hip_stream; `mine` must not be overwritten before the stream passes this call. */
int svo_exchange_frames(svo_exchange* x, const svo_tree* t, const svo_cast_desc* d, const svo_hits* mine, const svo_hits* frames_out,
                        void* hip_stream);
/* the same exchange from wire records this rank cast itself (svo_cast_wire of d into `wire`, with `ao` when
   d->ao_samples > 0): no pack pass; the records of the frames this rank displays are decoded from `wire`
   in place (they never travel).  `wire` and `ao` must not be overwritten before the stream passes this call. */
int svo_exchange_wire(svo_exchange* x, const svo_tree* t, const svo_cast_desc* d, const void* wire, const uint8_t* ao,
                      const svo_hits* frames_out, void* hip_stream);

/* ---------------------------------------------------------------------------- shading ------- */
/* Shading pass: low_res.frag's colour model over castRayFromCam hits, one float4
   (r, g, b, 0) per ray in the order of the hit records:
     miss            -> genSkyBox (low_res.frag:157-168) of the final direction x finalColorMod
     hit             -> colour x calcLightIntensity (:242-252) x finalColorMod; unless reflected, 0.3 x
                        colour x finalColorMod when the face turns away from the sun or a shadow ray
                        (castRayFromCam semantics from the centre of lastPos towards sun_dir,
                        shadow_steps steps, liquid passes) hits (:361-391)
     look_at voxel   -> colour x 2 + 0.3 (:340-343)
   A block with flags & 7 == 3 reflects the ray while budget remains (:170-189, :319-331):
   the last crossing on the hit axis is undone, that axis's step and direction flip, the DDA
   continues; finalColorMod *= 0.94 per reflection.  A refractive block (flags & 7 == 5) while
   budget remains is passed with finalColorMod *= (0.94, 0.97, 1.0) for liquid, 0.95 otherwise
   (:214); the first one bends the ray (refractRay :196-240, n 1.0 -> 1.1, normal = hit axis x step,
   for liquid plus the shader's wobble sin((time + exact.x * 0.2 - exact.z * 0.1) * 10) * 0.2 on x
   and renormalised, :225-229; the shader's origin-based exact position) and deltaPos restarts from
   the current cell.  Liquid is seen only through a scene tree of SVO_VIEW_ALL (built from the same
   world or terrain as t); without one (scene == NULL) liquid passes unbent, as in castRayFromCam.
   Single precision in the shader's operation order; sin through double precision, rounded once. */
typedef struct {
    float sun_dir[3];      /* normalised sunDir (globals.cpp:23: normalize(2,1,4)) */
    int32_t look_at[3];    /* lookingAtBlock (main.cpp:81,89) */
    int32_t look_at_valid; /* 0: no highlight */
    int32_t shadow_steps;  /* 75 (low_res.frag:382) */
    const svo_tree* scene; /* SVO_VIEW_ALL tree the primary / reflected / refracted ray walks (NULL: t);
                              shadow rays walk t (liquid passes) */
    float time;            /* deltaTime uniform of the liquid wobble (low_res.frag:226) */
    const svo_ray_result* look_at_dev; /* device record (NULL: use look_at / look_at_valid): lookingAtBlock is its
                              pos, read by the kernel — e.g. written by svo_cast_ray_from_cam_async on the same
                              stream, so a frame needs no host round trip (main.cpp:81,89) */
} svo_shade_desc;

/* asynchronous on hip_stream; rgba: device float4 per ray; hits: optional hit records (may be NULL) */
int svo_shade_rays(const svo_tree* t, const svo_cast_desc* d, const svo_shade_desc* s, float* rgba, const svo_hits* hits,
                   void* hip_stream);

/* host helpers shared bit-for-bit with the device code */
int svo_proj_plane(int32_t width, int32_t height, float* ppx, float* ppy);
int svo_normalize(const float v[3], float out[3]);
int svo_pixel_dir(const float cam_dir[3], float ppx, float ppy, int32_t width, int32_t height, int32_t px, int32_t py,
                  float out[3]);
/* every pixel's direction, out[3 * (py * width + px) + a] */
int svo_pixel_dirs(const float cam_dir[3], float ppx, float ppy, int32_t width, int32_t height, float* out);
/* gen_hemisphare_distrib.py's table for n points (x, y, pole) as float: phi = acos(1-(i+.5)*.85/n),
   theta = pi*(1+sqrt 5)*(i+.5) */
int svo_hemisphere(int32_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* SVO_RT_H */
