// svo_patch_commit.h — how the device-side patches put their result into a resident tree (commit_cells of
// svo_patch_cells.h, the one descent of them all, calls it).  A patch is written to scratch first; once its totals are known the
// device arrays are grown when the tail would not fit (emit_tree's slack rule), the tail is appended, the anchor's one
// record is rewritten in place, and the tail and that record are copied back to the host image.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "svo_hip.h"
#include "svo_internal.h"

namespace {

using namespace svo;

// the device arrays grown to hold `need_n` nodes and `need_m` material entries (emit_tree's slack rule), the first `keep_n` /
// `keep_m` elements kept
inline int grow_device(svo_tree* t, const char* who, uint64_t need_n, uint64_t keep_n, uint64_t need_m, uint64_t keep_m) {
    if (need_n > t->dev_node_cap) {
        const uint64_t cap = std::min<uint64_t>(need_n + need_n / 8 + 65536, 1ull << 32);
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, cap * sizeof(Node)), SVO_ENOMEM);
        if (hipMemcpy(p, t->d_nodes, keep_n * sizeof(Node), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipFree(p);
            SVO_FAIL(SVO_EDEVICE, std::string(who) + ": device copy failed");
        }
        (void)hipFree(t->d_nodes);
        t->d_nodes = p;
        t->device_bytes += (cap - t->dev_node_cap) * sizeof(Node);
        t->dev_node_cap = cap;
    }
    if (need_m > t->dev_mat_cap) {
        const uint64_t cap = std::min<uint64_t>(need_m + need_m / 8 + 65536, 1ull << 32);
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, cap * sizeof(uint16_t)), SVO_ENOMEM);
        if (keep_m && hipMemcpy(p, t->d_mats, keep_m * sizeof(uint16_t), hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipFree(p);
            SVO_FAIL(SVO_EDEVICE, std::string(who) + ": device copy failed");
        }
        (void)hipFree(t->d_mats);
        t->d_mats = p;
        t->device_bytes += (cap - t->dev_mat_cap) * sizeof(uint16_t);
        t->dev_mat_cap = cap;
    }
    return SVO_OK;
}

// A finished patch in scratch (device memory): out[0] is the anchor's new record, out[1 .. add] the node tail, which becomes
// nodes nbase .. of the tree; mats[0 .. n_mats) the material tail at mbase.  whole: the arrays restart (nothing is kept).
struct PatchTail {
    const Node* out;
    uint64_t add;
    const uint16_t* mats;
    uint64_t n_mats;
    uint32_t anchor_node;
    uint64_t nbase, mbase;
    bool whole;
};

// Nothing of the tree has changed before the call; after an error before the first copy into the arrays it still has not.
inline int commit_patch(svo_tree* t, const char* who, const PatchTail& p) {
    const uint64_t total_n = p.nbase + p.add, total_m = p.mbase + p.n_mats;
    try {  // (the host vectors grow with the device arrays' slack: an exact reserve would copy the whole image at every patch)
        if (total_n > t->nodes.capacity()) t->nodes.reserve(total_n + total_n / 8 + 65536);
        if (total_m > t->mats.capacity()) t->mats.reserve(total_m + total_m / 8 + 65536);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, std::string(who) + ": out of host memory");
    }
    int rc = grow_device(t, who, total_n, p.whole ? 0 : p.nbase, total_m, p.mbase);
    if (rc) return rc;
    Node* dn = reinterpret_cast<Node*>(t->d_nodes);
    uint16_t* dm = reinterpret_cast<uint16_t*>(t->d_mats);
    if (p.add) HIP_TRY(hipMemcpy(dn + p.nbase, p.out + 1, p.add * sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    if (p.n_mats) HIP_TRY(hipMemcpy(dm + p.mbase, p.mats, p.n_mats * sizeof(uint16_t), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(dn + p.anchor_node, p.out, sizeof(Node), hipMemcpyDeviceToDevice), SVO_EDEVICE);
    // the host image stays the mirror of HBM
    t->nodes.resize(total_n);
    t->mats.resize(total_m);
    if (p.add) HIP_TRY(hipMemcpy(t->nodes.data() + p.nbase, dn + p.nbase, p.add * sizeof(Node), hipMemcpyDeviceToHost), SVO_EDEVICE);
    if (p.n_mats) HIP_TRY(hipMemcpy(t->mats.data() + p.mbase, dm + p.mbase, p.n_mats * sizeof(uint16_t), hipMemcpyDeviceToHost), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(t->nodes.data() + p.anchor_node, dn + p.anchor_node, sizeof(Node), hipMemcpyDeviceToHost), SVO_EDEVICE);
    t->synced_nodes = total_n;
    t->synced_mats = total_m;
    t->volume_patched = true;
    return SVO_OK;
}

}  // namespace
