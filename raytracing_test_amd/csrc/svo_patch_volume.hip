// svo_patch_volume.hip — svo_tree_patch_volume_gpu: the content of a resident tree inside a dense box of voxels in HBM is
// replaced by the box, on the device.  The result is the tree of the composite (the box inside, the old tree outside):
//   * a region the box does not meet keeps its record and its subtree;
//   * an aligned region wholly inside the box is emitted canonically from the box alone, through the class pyramid of
//     svo_build_volume_gpu over the box (svo_volume_pyramid.h; its level-1 pass reads the box once and checks the ids)
//     and the plain emitter's rules: EMPTY clears the slot bit, an id is a K_SOLID child, MIXED descends;
//   * a region the box cuts is re-emitted one level down: a new child block at the tail whose slots are the old child
//     record copied (outside the box; below a K_SOLID region a synthesised K_SOLID, below an empty one nothing), the
//     pyramid's answer (inside), or again a cut region.  A cut brick is classified from its 64 composite voxels (the box's
//     voxel after the view filter, else the old tree's) by k_brick_count / k_brick_write's rules; one that stores no voxel
//     clears its slot bit, so no K_BRICK record with mask 0 exists.  Cut interior regions are not re-collapsed.
// Level-synchronous like svo_build_emit.h: one wavefront per region, lane = child slot (voxel at the brick level), ballots
// for the masks, exclusive scans (hipCUB) for child-block and material-run offsets, a count pass and a write pass per level;
// one list of work items per level holds the cut regions (with what they held before) and the plain MIXED ones.  The
// descent starts at the anchor the host finds on its image (svo_plan.cpp patch_anchor), whose record is the only one
// rewritten in place.  Everything is written to scratch first: the totals are known, and every id checked, before the
// tree is touched, and the arrays are reallocated (emit_tree's slack rule) only when the tail would not fit
// (svo_patch_commit.h, shared with svo_patch_points.hip).
// Every node and material index is widened to 64 bits before it addresses memory: trees above 2^28 nodes take the same
// kernels.
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
#include "svo_tree_descent.h"
#include "svo_volume_pyramid.h"

using namespace svo;

namespace {

// a region of one level's list: where its record goes (Region.node: an index into the scratch records; 0 is the anchor's),
// and what it held (svo_plan.h P_*: `old` is a node index or a material)
struct Item {
    Region r;
    uint32_t old, kind;
};

struct DevPatch {
    DevVolume V;           // the box and its pyramid
    const Node* nodes;     // the resident tree (read only: the patch is written to scratch)
    const uint16_t* mats;
    int32_t levels;
    int32_t b0[3], b1[3];  // the box, [b0, b1)
    uint64_t nbase;        // scratch record s >= 1 becomes node nbase + s - 1 of the tree
};

enum : uint32_t { REL_OUT = 0u, REL_IN = 1u, REL_CUT = 2u };
__device__ __forceinline__ uint32_t relation(const DevPatch& P, int32_t x, int32_t y, int32_t z, int32_t cs) {
    const int32_t c[3] = {x, y, z};
    bool out = false, in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        out = out || c[a] + cs <= P.b0[a] || c[a] >= P.b1[a];
        in = in && c[a] >= P.b0[a] && c[a] + cs <= P.b1[a];
    }
    return out ? REL_OUT : (in ? REL_IN : REL_CUT);
}

// the composite: the box's voxel (after the view filter) inside the box, the old tree's outside (svo_tree_descent.h)
__device__ __forceinline__ uint32_t comp_voxel(const DevPatch& P, int32_t x, int32_t y, int32_t z) {
    const bool in = x >= P.b0[0] && x < P.b1[0] && y >= P.b0[1] && y < P.b1[1] && z >= P.b0[2] && z < P.b1[2];
    return in ? P.V.voxel(x, y, z) : old_voxel(P, (uint32_t)x, (uint32_t)y, (uint32_t)z);
}

// what a child slot of a region becomes
enum : uint32_t { CH_NONE = 0u, CH_SOLID = 1u, CH_COPY = 2u, CH_NEXT = 3u };
struct Child {
    uint32_t what;
    uint32_t a;  // CH_SOLID: the material; CH_COPY: the old record's index; CH_NEXT: the next item's `old`
    uint32_t b;  // CH_NEXT: the next item's kind
};

// slot sl of item `it` (children cs = 4^k voxels wide); on = the old record of a P_NODE item
__device__ Child child_of(const DevPatch& P, const Item& it, const Node& on, uint32_t sl, int32_t cs, int k) {
    const int32_t x = it.r.x0 + (int32_t)(sl & 3u) * cs, y = it.r.y0 + (int32_t)((sl >> 2) & 3u) * cs, z = it.r.z0 + (int32_t)(sl >> 4) * cs;
    const uint32_t rel = it.kind == P_PLAIN ? REL_IN : relation(P, x, y, z, cs);
    if (rel == REL_IN) {
        const uint32_t c = P.V.classify(x, y, z, cs, k);
        if (c == G_EMPTY) return Child{CH_NONE, 0u, 0u};
        if (c == G_MIXED) return Child{CH_NEXT, 0u, P_PLAIN};
        return Child{CH_SOLID, c, 0u};
    }
    // what the child held
    uint32_t okind = it.kind, old = it.old;
    if (it.kind == P_NODE) {
        okind = P_EMPTY;
        if ((on.mask >> sl) & 1ull) {
            old = on.ref + (uint32_t)__popcll(on.mask & ((1ull << sl) - 1ull));
            if (rel == REL_OUT) return Child{CH_COPY, old, 0u};
            const uint32_t info = P.nodes[(uint64_t)old].info;
            okind = P_NODE;
            if (node_kind(info) == K_SOLID) {
                okind = P_UNIFORM;
                old = node_material(info);
            }
        }
    }
    if (rel == REL_OUT) return okind == P_UNIFORM ? Child{CH_SOLID, old, 0u} : Child{CH_NONE, 0u, 0u};
    if (k == 1) {  // a cut brick: absent unless a composite voxel is stored
        bool any = false;
        for (uint32_t v = 0; v < 64u && !any; v++) any = comp_voxel(P, x + (int32_t)(v & 3u), y + (int32_t)((v >> 2) & 3u), z + (int32_t)(v >> 4)) != G_EMPTY;
        if (!any) return Child{CH_NONE, 0u, 0u};
    }
    return Child{CH_NEXT, old, okind};
}

__device__ __forceinline__ Node old_record(const DevPatch& P, const Item& it) {
    return it.kind == P_NODE ? P.nodes[(uint64_t)it.old] : Node{0ull, 0u, K_INTERIOR};
}

// one wavefront per item, lane = child slot: the children that exist and those that go on to the next level's list
__global__ void k_patch_count(DevPatch P, const Item* cur, int64_t r0, int64_t n, int32_t cs, int k, uint32_t* nkid, uint32_t* nnext) {
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
__global__ void k_patch_write(DevPatch P, const Item* cur, int64_t r0, int64_t n, int32_t cs, int k, const uint64_t* koff, const uint64_t* noff,
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
__global__ void k_patch_brick_count(DevPatch P, const Item* cur, int64_t r0, int64_t n, uint32_t* nmat) {
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
__global__ void k_patch_brick_write(DevPatch P, const Item* cur, int64_t r0, int64_t n, const uint64_t* moff, uint64_t mbase, Node* out,
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

extern "C" int svo_tree_garbage(const svo_tree* t, uint64_t* nodes, uint64_t* mats) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_garbage: NULL tree");
    if (nodes) *nodes = t->garbage_nodes;
    if (mats) *mats = t->garbage_mats;
    return SVO_OK;
}

extern "C" int svo_tree_patch_volume_gpu(svo_tree* t, const svo_volume_box* box) {
    const char* who = "svo_tree_patch_volume_gpu";
    if (!t || !box) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: NULL argument");
    if (!box->voxels) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: NULL voxels");
    if (box->nx < 1 || box->ny < 1 || box->nz < 1) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: dimensions must be positive");
    const int32_t L = t->levels;
    const int64_t E = (int64_t)1 << (2 * L);
    const int32_t dims[3] = {box->nx, box->ny, box->nz};
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        if (box->origin[a] < 0 || (int64_t)box->origin[a] + dims[a] > E)
            SVO_FAIL(SVO_EINVAL, "svo_tree_patch_volume_gpu: the box must lie within the extent (no wrap)");
        lo[a] = box->origin[a];
        hi[a] = box->origin[a] + dims[a];
    }
    if (t->device < 0 || !t->d_nodes) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_volume_gpu: tree not uploaded (svo_upload)");
    if (tree_unsynced(t)) SVO_FAIL(SVO_ESTATE, "svo_tree_patch_volume_gpu: the tree has host edits not yet synced (svo_tree_sync)");
    if (L < 2 || t->nodes.empty()) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: trees of fewer than 2 levels are not patched");
    if (t->palette.empty() || t->palette.size() > 65535) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: the palette must hold 1..65535 entries");

    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // the box may come from any stream, and records and ceilings are rewritten in place below: every cast over the tree
    // must be over first (svo_tree_sync's contract)
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock0 = std::chrono::steady_clock::now();

    // the box as a volume of the tree's own palette and view, and its class pyramid: ids are checked here
    std::vector<svo_block> blocks;
    std::vector<Material> pal;
    try {
        for (const Material& m : t->palette) blocks.push_back(to_block(m));
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "svo_tree_patch_volume_gpu: out of memory");
    }
    svo_volume_desc vd;
    memset(&vd, 0, sizeof(vd));
    vd.levels = L;
    vd.nx = box->nx;
    vd.ny = box->ny;
    vd.nz = box->nz;
    for (int a = 0; a < 3; a++) vd.origin[a] = box->origin[a];
    vd.voxels = box->voxels;
    vd.palette = blocks.data();
    vd.n_palette = (uint32_t)blocks.size();
    vd.view = t->view;
    vd.device = t->device;
    Pool pool;
    DevPatch P;
    memset(&P, 0, sizeof(P));
    bool all = false, bad = false;
    uint16_t top = 0;
    int rc = prepare(&vd, pool, P.V, pal, all);
    if (!rc) rc = build_pyramid(P.V, L, all, pool, &bad, &top);
    if (rc) return rc;
    if (bad) SVO_FAIL(SVO_ERANGE, "svo_tree_patch_volume_gpu: a voxel id is not below the tree's palette size");

    const PatchAnchor anchor = patch_anchor(t->nodes.data(), L, lo, hi);
    // a box that is the whole extent is a full build: the arrays restart behind the root and nothing is left superseded
    const uint64_t nbase = anchor.whole ? 1 : t->synced_nodes, mbase = anchor.whole ? 0 : t->synced_mats;
    uint64_t gnodes = 0, gmats = 0;
    if (!anchor.whole) patch_superseded(t->nodes.data(), L, anchor, lo, hi, &gnodes, &gmats);
    P.nodes = reinterpret_cast<const Node*>(t->d_nodes);
    P.mats = reinterpret_cast<const uint16_t*>(t->d_mats);
    P.levels = L;
    for (int a = 0; a < 3; a++) {
        P.b0[a] = lo[a];
        P.b1[a] = hi[a];
    }
    P.nbase = nbase;

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

    Item first{Region{anchor.o[0], anchor.o[1], anchor.o[2], 0u}, anchor.old, anchor.kind};
    int64_t ncur = 1;
    if (anchor.whole) {
        first = Item{Region{0, 0, 0, 0u}, 0u, P_PLAIN};
        if (top != C_MIXED) {  // a root without children
            const Node root = top == C_EMPTY ? Node{0ull, 0u, K_INTERIOR} : Node{~0ull, 0u, K_SOLID | ((uint32_t)top << 16)};
            HIP_TRY(hipMemcpy(out, &root, sizeof(Node), hipMemcpyHostToDevice), SVO_EDEVICE);
            ncur = 0;
        }
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
                hipLaunchKernelGGL(k_patch_brick_count, g, dim3(256), 0, nullptr, P, cur, r0, ncur, nmat);
            });
            if (rc) return rc;
            rc = scan(nmat, moff, ncur, &n_mats, tmp);
            if (rc) return rc;
            if (mbase + n_mats > 0xFFFFFFFFull) SVO_FAIL(SVO_ERANGE, std::string(who) + ": tree exceeds 2^32 material entries");
            rc = pool.alloc(&mats, n_mats + 1);
            if (rc) return rc;
            rc = for_region_chunks(ncur, [&](int64_t r0, dim3 g) {
                hipLaunchKernelGGL(k_patch_brick_write, g, dim3(256), 0, nullptr, P, cur, r0, ncur, moff, mbase, out, mats);
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
            hipLaunchKernelGGL(k_patch_count, g, dim3(256), 0, nullptr, P, cur, r0, ncur, cs, L - d - 1, nkid, nnext);
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
            hipLaunchKernelGGL(k_patch_write, g, dim3(256), 0, nullptr, P, cur, r0, ncur, cs, L - d - 1, koff, noff, used, out, next);
        });
        if (rc) return rc;
        used += nk;
        cur = next;
        ncur = (int64_t)nn;
    }
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    const auto clock1 = std::chrono::steady_clock::now();

    // the totals are known and nothing of the tree has changed yet: room, then the tail, then the anchor's record
    rc = commit_patch(t, who, PatchTail{out, used - 1, mats, n_mats, anchor.node, nbase, mbase, anchor.whole});
    if (rc) return rc;
    if (anchor.whole) {
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
    t->ceil_dirty.push_back({lo[0], lo[2], hi[0], hi[2]});
    rc = sync_ceilings(t);
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    t->patch_ms[0] = ms(clock0, clock1);
    t->patch_ms[1] = ms(clock1, clock2);
    t->patch_ms[2] = ms(clock2, std::chrono::steady_clock::now());
    return rc;
}

extern "C" int svo_tree_patch_times(const svo_tree* t, double ms[3]) {
    if (!t || !ms) SVO_FAIL(SVO_EINVAL, "svo_tree_patch_times: NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = t->patch_ms[i];
    return SVO_OK;
}
