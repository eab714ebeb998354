// svo_patch_shapes.hip — svo_tree_patch_shapes_gpu: a resident tree is changed, on the device, by an ordered list of solid
// shapes (boxes and balls, each with the id it stores; id 0 erases).  A voxel ends up with the id of the last shape that
// contains it; the cost follows the shapes' surfaces, never their volumes.  The descent is svo_patch_volume.hip's, with
// the box's class pyramid replaced by a closed form (svo_shape_cell.h cell_relation, asked per cell over the whole table):
//   * a cell no shape touches keeps its record and its subtree (below a K_SOLID region: a synthesised K_SOLID, below an
//     empty one nothing);
//   * a cell wholly inside the deciding shape is one K_SOLID record of that shape's id at whatever level it sits, or a
//     clear slot bit for id 0: nothing is read for it;
//   * a cell the deciding shape cuts is re-emitted one level down: a new child block at the tail.  A cut brick is
//     classified from its 64 composite voxels (shape_voxel, else the old tree's: svo_tree_descent.h) by k_brick_count /
//     k_brick_write's rules; one that stores no voxel clears its slot bit, so no K_BRICK record with mask 0 exists.  Cut
//     interior cells are not re-collapsed.
// Level-synchronous: one wavefront per cut cell, lane = child slot (voxel at the brick level), ballots for the masks,
// exclusive scans (hipCUB) for child-block and material-run offsets, a count pass and a write pass per level.  An item
// carries only what the tree held (svo_plan.h P_NODE / P_UNIFORM / P_EMPTY): every child asks cell_relation anew.  The
// table sits in HBM and is indexed by the loop counter alone, the same in every lane; it is not copied per lane.
// The descent starts at the anchor the host finds on its image (svo_plan.cpp patch_anchor over the union of the shapes'
// clipped bounding boxes), whose record is the only one rewritten in place.  A bounding box equal to the extent does not
// restart the arrays: they restart only when cell_relation calls the whole extent IN.  The superseded records are counted
// by a host walk (svo_plan.cpp shapes_superseded) that asks the same cell_relation about the same cells.  Everything is
// written to scratch first, and committed through svo_patch_commit.h as the other patches are.
// Every node and material index is widened to 64 bits before it addresses memory.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/svo_rt.h"
#include "svo_build_emit.h"
#include "svo_hip.h"
#include "svo_internal.h"
#include "svo_patch_commit.h"
#include "svo_plan.h"
#include "svo_shape_cell.h"
#include "svo_tree_descent.h"

using namespace svo;

static_assert(kShapeBox == SVO_SHAPE_BOX && kShapeBall == SVO_SHAPE_BALL, "svo_shape_cell.h's kinds are the ABI's");

namespace {

// a cut cell of one level's list: where its record goes (Region.node: an index into the scratch records; 0 is the
// anchor's), and what the tree held there (svo_plan.h P_NODE / P_UNIFORM / P_EMPTY: `old` is a node index or a material)
struct Item {
    Region r;
    uint32_t old, kind;
};

struct DevShapes {
    const ShapeRec* shapes;  // the table, in list order
    int32_t n;
    const Node* nodes;       // the resident tree (read only: the patch is written to scratch)
    const uint16_t* mats;
    int32_t levels;
    uint64_t nbase;          // scratch record s >= 1 becomes node nbase + s - 1 of the tree
};

// the composite: the last shape's id where a shape holds the voxel, the old tree's elsewhere (svo_tree_descent.h)
__device__ __forceinline__ uint32_t comp_voxel(const DevShapes& P, int32_t x, int32_t y, int32_t z) {
    uint32_t id;
    return shape_voxel(P.shapes, P.n, x, y, z, &id) ? id : old_voxel(P, (uint32_t)x, (uint32_t)y, (uint32_t)z);
}

// what a child slot of a cell becomes
enum : uint32_t { CH_NONE = 0u, CH_SOLID = 1u, CH_COPY = 2u, CH_NEXT = 3u };
struct Child {
    uint32_t what;
    uint32_t a;  // CH_SOLID: the material; CH_COPY: the old record's index; CH_NEXT: the next item's `old`
    uint32_t b;  // CH_NEXT: the next item's kind
};

// slot sl of item `it` (children cs = 4^k voxels wide); on = the old record of a P_NODE item
__device__ Child child_of(const DevShapes& P, const Item& it, const Node& on, uint32_t sl, int32_t cs, int k) {
    const int32_t x = it.r.x0 + (int32_t)(sl & 3u) * cs, y = it.r.y0 + (int32_t)((sl >> 2) & 3u) * cs, z = it.r.z0 + (int32_t)(sl >> 4) * cs;
    uint32_t id;
    const uint32_t rel = cell_relation(P.shapes, P.n, x, y, z, cs, &id);
    if (rel == SHAPE_IN) return id ? Child{CH_SOLID, id, 0u} : Child{CH_NONE, 0u, 0u};
    // what the child held
    uint32_t okind = it.kind, old = it.old;
    uint64_t om = it.kind == P_UNIFORM ? ~0ull : 0ull;  // (k == 1) the voxels the old child stored
    if (it.kind == P_NODE) {
        okind = P_EMPTY;
        if ((on.mask >> sl) & 1ull) {
            old = on.ref + (uint32_t)__popcll(on.mask & ((1ull << sl) - 1ull));
            if (rel == SHAPE_OUT) return Child{CH_COPY, old, 0u};
            const Node oc = P.nodes[(uint64_t)old];
            okind = P_NODE;
            om = oc.mask;
            if (node_kind(oc.info) == K_SOLID) {
                okind = P_UNIFORM;
                old = node_material(oc.info);
                om = ~0ull;
            }
        }
    }
    if (rel == SHAPE_OUT) return okind == P_UNIFORM ? Child{CH_SOLID, old, 0u} : Child{CH_NONE, 0u, 0u};
    if (k == 1) {  // a cut brick: absent unless a composite voxel is stored (a shape's id, else what om says the tree held)
        bool any = false;
        for (uint32_t v = 0; v < 64u && !any; v++) {
            uint32_t vid;
            const bool hit = shape_voxel(P.shapes, P.n, x + (int32_t)(v & 3u), y + (int32_t)((v >> 2) & 3u), z + (int32_t)(v >> 4), &vid);
            any = hit ? vid != 0u : (bool)((om >> v) & 1ull);
        }
        if (!any) return Child{CH_NONE, 0u, 0u};
    }
    return Child{CH_NEXT, old, okind};
}

__device__ __forceinline__ Node old_record(const DevShapes& P, const Item& it) {
    return it.kind == P_NODE ? P.nodes[(uint64_t)it.old] : Node{0ull, 0u, K_INTERIOR};
}

// one wavefront per item, lane = child slot: the children that exist and those that go on to the next level's list
__global__ void k_shapes_count(DevShapes P, const Item* cur, int64_t r0, int64_t n, int32_t cs, int k, uint32_t* nkid, uint32_t* nnext) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;  // whole waves exit together
    const Item it = cur[r];
    const Child c = child_of(P, it, old_record(P, it), sl, cs, k);
    const uint64_t kid = __ballot(c.what != CH_NONE), nx = __ballot(c.what == CH_NEXT);
    if (sl == 0) {
        nkid[r] = (uint32_t)__popcll(kid);
        nnext[r] = (uint32_t)__popcll(nx);
    }
}

// second pass: the item's INTERIOR record, its SOLID and copied children, the next level's items.  base: the scratch
// index of this level's first child record
__global__ void k_shapes_write(DevShapes P, const Item* cur, int64_t r0, int64_t n, int32_t cs, int k, const uint64_t* koff, const uint64_t* noff,
                               uint64_t base, Node* out, Item* next) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t sl = threadIdx.x & 63u;
    if (r >= n) return;
    const Item it = cur[r];
    const Child c = child_of(P, it, old_record(P, it), sl, cs, k);
    const uint64_t kid = __ballot(c.what != CH_NONE), nx = __ballot(c.what == CH_NEXT);
    const uint64_t below = (1ull << sl) - 1ull;
    const uint64_t kpos = base + koff[r] + (uint64_t)__popcll(kid & below);
    if (c.what == CH_NEXT) {
        const Region R{it.r.x0 + (int32_t)(sl & 3u) * cs, it.r.y0 + (int32_t)((sl >> 2) & 3u) * cs, it.r.z0 + (int32_t)(sl >> 4) * cs, (uint32_t)kpos};
        next[noff[r] + (uint64_t)__popcll(nx & below)] = Item{R, c.a, c.b};
    } else if (c.what == CH_SOLID) {
        out[kpos] = Node{~0ull, 0u, K_SOLID | (c.a << 16)};
    } else if (c.what == CH_COPY) {
        out[kpos] = P.nodes[(uint64_t)c.a];
    }
    if (sl == 0) out[it.r.node] = Node{kid, (uint32_t)(P.nbase + base + koff[r] - 1ull), K_INTERIOR};
}

// bricks, by k_brick_count / k_brick_write's rules over the composite voxels (every item stores at least one)
__global__ void k_shapes_brick_count(DevShapes P, const Item* cur, int64_t r0, int64_t n, uint32_t* nmat) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const Region R = cur[r].r;
    const uint32_t c = comp_voxel(P, R.x0 + (int32_t)(v & 3u), R.y0 + (int32_t)((v >> 2) & 3u), R.z0 + (int32_t)(v >> 4));
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    if (v == 0) nmat[r] = uni ? 0u : (uint32_t)__popcll(solid);
}

// mbase: the tree's material index of mats[0]
__global__ void k_shapes_brick_write(DevShapes P, const Item* cur, int64_t r0, int64_t n, const uint64_t* moff, uint64_t mbase, Node* out,
                                     uint16_t* mats) {
    const int64_t r = r0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t v = threadIdx.x & 63u;
    if (r >= n) return;
    const Region R = cur[r].r;
    const uint32_t c = comp_voxel(P, R.x0 + (int32_t)(v & 3u), R.y0 + (int32_t)((v >> 2) & 3u), R.z0 + (int32_t)(v >> 4));
    const uint64_t solid = __ballot(c != G_EMPTY);
    const bool uni = g_uniform(c, solid);
    const uint32_t first = (uint32_t)__shfl((int)c, (int)__builtin_ctzll(solid | (1ull << 63)));
    if (!uni && c != G_EMPTY) mats[moff[r] + (uint64_t)__popcll(solid & ((1ull << v) - 1ull))] = (uint16_t)c;
    if (v == 0) out[R.node] = uni ? Node{solid, 0u, K_BRICK | K_UNIFORM | (first << 16)} : Node{solid, (uint32_t)(mbase + moff[r]), K_BRICK};
}

}  // namespace

extern "C" int svo_tree_patch_shapes_gpu(svo_tree* t, const svo_shape* shapes, int32_t n) {
    const char* who = "svo_tree_patch_shapes_gpu";
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: NULL tree");
    if (n < 0) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: n must not be negative");
    if (n > 0 && !shapes) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_shapes_gpu: NULL shapes");
    if (n > kShapesMax) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: n must not exceed 1024");
    const int32_t L = t->levels;
    if (L < 2 || t->nodes.empty()) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: trees of fewer than 2 levels are not patched");
    if (t->palette.empty() || t->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_shapes_gpu: the palette must hold 1..65535 entries");
    ShapesPlan plan;
    int32_t bad = -1;
    int why = SHAPES_OK;
    try {
        why = shapes_plan(L, t->view, t->palette, shapes, n, &plan, &bad);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_shapes_gpu: out of memory");
    }
    if (why != SHAPES_OK) {
        const std::string at = std::string(who) + ": shape " + std::to_string(bad) + ": ";
        switch (why) {
            case SHAPES_KIND: SVO_FAIL(SVO_EINVAL, at + "unknown kind");
            case SHAPES_BOX_DIM: SVO_FAIL(SVO_EINVAL, at + "a box's dimensions must be positive");
            case SHAPES_BOX_EXTENT: SVO_FAIL(SVO_EINVAL, at + "a box must lie within the extent (no wrap)");
            case SHAPES_R2_NEG: SVO_FAIL(SVO_EINVAL, at + "r2 must not be negative");
            case SHAPES_CENTRE: SVO_FAIL(SVO_ERANGE, at + "a ball's centre must lie within 2^20 of the origin on every axis");
            case SHAPES_R2_BIG: SVO_FAIL(SVO_ERANGE, at + "r2 must not exceed 2^42");
            default: SVO_FAIL(SVO_ERANGE, at + "the id is not below the tree's palette size");
        }
    }
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_shapes_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_shapes_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    const int32_t ns = (int32_t)plan.table.size();
    if (ns == 0) return SVO_OK;  // no shape, or every one clipped away

    // the anchor, the restart and the superseded records: host work on the image, before the first HIP call
    uint32_t top_id = 0;
    const bool whole = cell_relation(plan.table.data(), ns, 0, 0, 0, 1 << (2 * L), &top_id) == SHAPE_IN;
    PatchAnchor anchor = patch_anchor(t->nodes.data(), L, plan.lo, plan.hi);
    anchor.whole = whole;  // (patch_anchor's own `whole`, a bounding box equal to the extent, only keeps the anchor at the root)

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // records and ceilings are rewritten in place below: every cast over the tree must be over first (svo_tree_sync's
    // contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    const uint64_t nbase = whole ? 1 : t->synced_nodes, mbase = whole ? 0 : t->synced_mats;
    uint64_t gnodes = 0, gmats = 0;
    if (!whole) shapes_superseded(t->nodes.data(), L, anchor, plan.table.data(), ns, &gnodes, &gmats);
    try {
        t->ceil_dirty.reserve(t->ceil_dirty.size() + plan.rects.size());
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_shapes_gpu: out of host memory");
    }

    Pool pool;
    ShapeRec* dshapes;
    int rc = pool.alloc(&dshapes, (size_t)ns);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dshapes, plan.table.data(), (size_t)ns * sizeof(ShapeRec), hipMemcpyHostToDevice), SVO_EDEVICE);
    const DevShapes P{dshapes, ns, reinterpret_cast<const Node*>(t->d_nodes), reinterpret_cast<const uint16_t*>(t->d_mats), L, nbase};

    // scratch records: [0] the anchor's, [1 ..) the appended tail; grown per level (capacity doubling, device copies)
    uint64_t cap = 1 << 12, used = 1, n_mats = 0;
    Node* out;
    rc = pool.alloc(&out, cap);
    if (rc) return rc;
    auto reserve = [&](uint64_t need) -> int {
        if (need <= cap) return SVO_OK;
        uint64_t nc = cap;
        while (nc < need) nc *= 2;
        Node* nn;
        int r2 = pool.alloc(&nn, nc);
        if (r2) return r2;
        HIP_TRY(hipMemcpy(nn, out, used * sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
        pool.release(out);
        (void)hipFree(out);
        out = nn;
        cap = nc;
        return SVO_OK;
    };
    uint16_t* mats = nullptr;
    std::vector<void*> tmp;
    struct TmpFree {
        std::vector<void*>& v;
        ~TmpFree() {
            for (void* x : v) (void)hipFree(x);
        }
    } tmp_free{tmp};

    const Item first{Region{anchor.o[0], anchor.o[1], anchor.o[2], 0u}, anchor.old, anchor.kind};
    int64_t ncur = 1;
    if (whole) {  // a root without children
        const Node root = top_id == 0 ? Node{0ull, 0u, K_INTERIOR} : Node{~0ull, 0u, K_SOLID | (top_id << 16)};
        HIP_TRY(hipMemcpy(out, &root, sizeof(Node), hipMemcpyHostToDevice), SVO_EDEVICE);
        ncur = 0;
    }
    Item* cur;
    rc = pool.alloc(&cur, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(cur, &first, sizeof(Item), hipMemcpyHostToDevice), SVO_EDEVICE);
    for (int d = anchor.depth; d < L && ncur > 0; d++) {
        const int32_t cs = 1 << (2 * (L - d - 1));
        if (d == L - 1) {
            uint32_t* nmat;
            uint64_t* moff;
            rc = pool.alloc(&nmat, ncur);
            if (!rc) rc = pool.alloc(&moff, ncur);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_shapes_brick_count, g, dim3(256), 0, nullptr, P, cur, r0, ncur, nmat);
            });
            if (rc) return rc;
            rc = scan(nmat, moff, ncur, &n_mats, tmp);
            if (rc) return rc;
            if (mbase + n_mats > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 material entries");
            rc = pool.alloc(&mats, n_mats + 1);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_shapes_brick_write, g, dim3(256), 0, nullptr, P, cur, r0, ncur, moff, mbase, out, mats);
            });
            if (rc) return rc;
            break;
        }
        uint32_t *nkid, *nnext;
        uint64_t *koff, *noff, nk = 0, nn = 0;
        rc = pool.alloc(&nkid, ncur);
        if (!rc) rc = pool.alloc(&nnext, ncur);
        if (!rc) rc = pool.alloc(&koff, ncur);
        if (!rc) rc = pool.alloc(&noff, ncur);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_shapes_count, g, dim3(256), 0, nullptr, P, cur, r0, ncur, cs, L - d - 1, nkid, nnext);
        });
        if (rc) return rc;
        rc = scan(nkid, koff, ncur, &nk, tmp);
        if (!rc) rc = scan(nnext, noff, ncur, &nn, tmp);
        if (rc) return rc;
        if (nbase + used - 1 + nk > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 nodes");
        rc = reserve(used + nk);
        if (rc) return rc;
        Item* next;
        rc = pool.alloc(&next, nn);
        if (rc) return rc;
        rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
            hipLaunchKernelGGL(k_shapes_write, g, dim3(256), 0, nullptr, P, cur, r0, ncur, cs, L - d - 1, koff, noff, used, out, next);
        });
        if (rc) return rc;
        used += nk;
        cur = next;
        ncur = (int64_t)nn;
    }
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock1 = std::chrono::steady_clock::now();

    // the totals are known and nothing of the tree has changed yet: room, then the tail, then the anchor's record
    rc = commit_patch(t, who, PatchTail{out, used - 1, mats, n_mats, anchor.node, nbase, mbase, whole});
    if (rc) return rc;
    if (whole) {
        t->garbage_nodes = t->garbage_mats = 0;
    } else {
        t->garbage_nodes += gnodes;
        t->garbage_mats += gmats;
    }
    const auto clock2 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(t->top_mu);
        t->top_valid = false;
    }
    t->dev_top_y = tree_top_y(t);
    for (const auto& r : plan.rects) t->ceil_dirty.push_back(r);
    rc = sync_ceilings(t);
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    t->patch_ms[0] = ms(clock0, clock1);
    t->patch_ms[1] = ms(clock1, clock2);
    t->patch_ms[2] = ms(clock2, std::chrono::steady_clock::now());
    return rc;
}
