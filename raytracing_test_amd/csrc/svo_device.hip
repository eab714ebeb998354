// svo_device.hip — a tree's residency in HBM (the updateSsboData analogue, src/voxel_data/voxel_allocator.hpp:38-91):
// upload, adoption of device-built arrays, the sync after edits, release.  HIP API calls only, no kernels; what moves
// is worked out by svo_plan.cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "svo_hip.h"
#include "svo_plan.h"

using namespace svo;

void svo::tree_release_device(svo_tree* t) {
    if (!t || t->device < 0) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(t->device);
    if (t->d_nodes) (void)hipFree(t->d_nodes);
    if (t->d_mats) (void)hipFree(t->d_mats);
    if (t->d_pal) (void)hipFree(t->d_pal);
    if (t->d_pick) (void)hipFree(t->d_pick);
    if (t->d_ao_plan) (void)hipFree(t->d_ao_plan);
    if (t->d_ceil) (void)hipFree(t->d_ceil);
    if (t->d_ceilp) (void)hipFree(t->d_ceilp);
    if (t->d_ceilq) (void)hipFree(t->d_ceilq);
    if (t->d_ceilf) (void)hipFree(t->d_ceilf);
    t->d_ceil = t->d_ceilp = t->d_ceilq = t->d_ceilf = nullptr;
    for (auto& e : t->scheds)
        if (e.d_buf) (void)hipFree(e.d_buf);
    t->scheds.clear();
    t->ceil_levels = 0;
    t->ceil_dev_n = 0;
    t->d_ao_plan = nullptr;
    t->ao_plan_steps = -1;
    (void)hipSetDevice(prev);
    t->d_nodes = t->d_mats = t->d_pick = t->d_pal = nullptr;
    t->dev_node_cap = t->dev_mat_cap = t->dev_pal_n = 0;
    t->device = -1;
    t->device_bytes = 0;
}

extern "C" void svo_tree_destroy(svo_tree* t) {
    if (!t) return;
    tree_release_device(t);
    delete t;
}

// the column ceilings of the host image (tree_ceilings), their pairs and quads, replacing the device copies (the device
// buffers are kept when their size is unchanged)
static int upload_ceilings(svo_tree* t) {
    int32_t n = 0;
    try {
        n = ceil_tables_build(t);
    } catch (const std::bad_alloc&) {
        t->ceil_host.clear();
        t->ceilp_host.clear();
        t->ceilq_host.clear();
        t->ceil_fine_host.clear();
        n = -1;
    }
    t->ceil_dirty.clear();
    // (the fine table's size follows from the levels, as the others': one test covers the four)
    if (n <= 0 || (int64_t)t->ceil_host.size() != t->ceil_dev_n) {
        if (t->d_ceil) (void)hipFree(t->d_ceil);
        if (t->d_ceilp) (void)hipFree(t->d_ceilp);
        if (t->d_ceilq) (void)hipFree(t->d_ceilq);
        if (t->d_ceilf) (void)hipFree(t->d_ceilf);
        t->d_ceil = t->d_ceilp = t->d_ceilq = t->d_ceilf = nullptr;
        t->ceil_dev_n = 0;
    }
    t->ceil_levels = 0;
    if (n < 0) SVO_FAIL(SVO_ENOMEM, "column ceilings: out of host memory");
    if (n == 0) return SVO_OK;
    const size_t m = t->ceil_host.size();
    if (!t->d_ceil) {
        HIP_TRY(hipMalloc(&t->d_ceil, m * sizeof(int16_t)), SVO_ENOMEM);
        HIP_TRY(hipMalloc(&t->d_ceilp, m * sizeof(uint32_t)), SVO_ENOMEM);
        HIP_TRY(hipMalloc(&t->d_ceilq, t->ceilq_host.size() * sizeof(uint64_t)), SVO_ENOMEM);
        HIP_TRY(hipMalloc(&t->d_ceilf, t->ceil_fine_host.size() * sizeof(int16_t)), SVO_ENOMEM);
        t->ceil_dev_n = (int64_t)m;
    }
    HIP_TRY(hipMemcpy(t->d_ceilf, t->ceil_fine_host.data(), t->ceil_fine_host.size() * sizeof(int16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(t->d_ceil, t->ceil_host.data(), m * sizeof(int16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(t->d_ceilp, t->ceilp_host.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    HIP_TRY(hipMemcpy(t->d_ceilq, t->ceilq_host.data(), t->ceilq_host.size() * sizeof(uint64_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    t->ceil_levels = n;
    return SVO_OK;
}

// after edits: only the columns svo_tree_update touched are recomputed (tree walks restricted to them), and only the
// rows of the tables that changed travel, into the device buffers already there
int svo::sync_ceilings(svo_tree* t) {
    if (t->ceil_dirty.empty()) return SVO_OK;
    if (t->ceil_levels == 0 || !t->d_ceil) {
        t->ceil_dirty.clear();
        return SVO_OK;
    }
    const int32_t n = t->ceil_levels;
    std::vector<std::array<int64_t, 4>> rects;
    rects.swap(t->ceil_dirty);
    CeilRows rows;
    try {
        ceil_tables_update_all(t, n, rects, &rows);
    } catch (const std::bad_alloc&) {
        SVO_FAIL(SVO_ENOMEM, "column ceilings: out of host memory");
    }
    {
        const int64_t w = (int64_t)1 << (2 * (t->levels - kCeilK0));
        for (const auto& q : rows.quads) {
            const int64_t lo = q.first * w, cnt = (q.second - q.first) * w;
            HIP_TRY(hipMemcpy(reinterpret_cast<uint64_t*>(t->d_ceilq) + lo, t->ceilq_host.data() + lo, cnt * sizeof(uint64_t),
                              hipMemcpyHostToDevice), SVO_EDEVICE);
        }
    }
    for (const auto& z : rows.level[0]) {
        const CeilFineSpan f = ceil_fine_span(t, z);
        HIP_TRY(hipMemcpy(reinterpret_cast<int16_t*>(t->d_ceilf) + f.first, t->ceil_fine_host.data() + f.first, f.count * sizeof(int16_t),
                          hipMemcpyHostToDevice), SVO_EDEVICE);
    }
    for (int32_t j = 0; j < n; j++) {
        const int64_t w = (int64_t)1 << (2 * (t->levels - kCeilK0 - j));
        for (const auto& z : rows.level[j]) {
            const int64_t lo = t->ceil_off[j] + z.first * w, cnt = (z.second - z.first) * w;
            HIP_TRY(hipMemcpy(reinterpret_cast<int16_t*>(t->d_ceil) + lo, t->ceil_host.data() + lo, cnt * sizeof(int16_t),
                              hipMemcpyHostToDevice), SVO_EDEVICE);
            HIP_TRY(hipMemcpy(reinterpret_cast<uint32_t*>(t->d_ceilp) + lo, t->ceilp_host.data() + lo, cnt * sizeof(uint32_t),
                              hipMemcpyHostToDevice), SVO_EDEVICE);
        }
    }
    return SVO_OK;
}

static int upload_palette(svo_tree* t) {
    // palette colours (u64[n]) then flags (u32[n]) for the shading pass
    const size_t np = std::max<size_t>(t->palette.size(), 1);
    std::vector<uint8_t> pal(np * 12, 0);
    for (size_t i = 0; i < t->palette.size(); i++) {
        memcpy(&pal[i * 8], &t->palette[i].color, 8);
        memcpy(&pal[np * 8 + i * 4], &t->palette[i].flags, 4);
    }
    if (t->d_pal) (void)hipFree(t->d_pal);
    t->d_pal = nullptr;
    HIP_TRY(hipMalloc(&t->d_pal, pal.size()), SVO_ENOMEM);
    HIP_TRY(hipMemcpy(t->d_pal, pal.data(), pal.size(), hipMemcpyHostToDevice), SVO_EDEVICE);
    t->dev_pal_n = np;
    t->palette_dirty = false;
    return SVO_OK;
}

// the rest of a tree's residency once d_nodes / d_mats (node_cap / mat_cap elements) hold its image on the current device
static int finish_residency(svo_tree* t, int32_t device, uint64_t node_cap, uint64_t mat_cap) {
    const size_t wb = kSideBytes;
    HIP_TRY(hipMalloc(&t->d_pick, wb), SVO_ENOMEM);
    HIP_TRY(hipMemset(t->d_pick, 0, wb), SVO_EDEVICE);
    int rc = upload_palette(t);
    if (rc) return rc;
    t->device = device;
    t->device_bytes = node_cap * sizeof(Node) + mat_cap * sizeof(uint16_t) + wb + t->dev_pal_n * 12;
    t->dev_node_cap = node_cap;
    t->dev_mat_cap = mat_cap;
    t->synced_nodes = t->nodes.size();
    t->dev_top_y = tree_top_y(t);
    t->synced_mats = t->mats.size();
    t->dirty_nodes.clear();
    t->full_upload = false;
    return upload_ceilings(t);
}

extern "C" int svo_upload(svo_tree* t, int32_t device) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_upload: NULL tree");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev), SVO_EDEVICE);
    if (device < 0 || device >= ndev) SVO_FAIL(SVO_EDEVICE, "svo_upload: no such HIP device");
    tree_release_device(t);
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    // capacity for appended edit blocks (svo_tree_update / svo_tree_sync) without reallocation
    // (node and material indices are 32-bit: no room beyond 2^32 elements)
    const uint64_t ncap = std::min<uint64_t>(t->nodes.size() + t->nodes.size() / 8 + 65536, 1ull << 32);
    const uint64_t mcap = std::min<uint64_t>(t->mats.size() + t->mats.size() / 8 + 65536, 1ull << 32);
    const size_t nb = ncap * sizeof(Node), mb = mcap * sizeof(uint16_t);
    HIP_TRY(hipMalloc(&t->d_nodes, nb), SVO_ENOMEM);
    HIP_TRY(hipMalloc(&t->d_mats, mb), SVO_ENOMEM);
    HIP_TRY(hipMemcpy(t->d_nodes, t->nodes.data(), t->nodes.size() * sizeof(Node), hipMemcpyHostToDevice), SVO_EDEVICE);
    if (!t->mats.empty()) HIP_TRY(hipMemcpy(t->d_mats, t->mats.data(), t->mats.size() * sizeof(uint16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    return finish_residency(t, device, ncap, mcap);
}

int svo::adopt_device(svo_tree* t, int32_t device, void* d_nodes, uint64_t node_cap, void* d_mats, uint64_t mat_cap) {
    tree_release_device(t);
    HIP_TRY(hipSetDevice(device), SVO_EDEVICE);
    t->d_nodes = d_nodes;
    t->d_mats = d_mats;
    return finish_residency(t, device, node_cap, mat_cap);
}

// updateSsboData after edits (voxel_allocator.hpp:38-78): only the appended tail and the records
// rewritten in place travel; a rebuilt or outgrown tree is uploaded whole
extern "C" int svo_tree_sync(svo_tree* t) {
    if (!t) SVO_FAIL(SVO_EINVAL, "svo_tree_sync: NULL tree");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, "svo_tree_sync: tree not uploaded (svo_upload)");
    if (t->full_upload || t->nodes.size() > t->dev_node_cap || t->mats.size() > t->dev_mat_cap) return svo_upload(t, t->device);
    if (!tree_unsynced(t)) return SVO_OK;  // nothing changed since the last upload / sync
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    // the records, ceilings and palette below are rewritten in place: every cast over the tree must be over first, on any
    // stream (null-stream copies do not wait for non-blocking streams; a frame reading lowered ceilings against old nodes
    // could skip blocks still stored).  As the reference's updateSsboData, this runs between frames.
    HIP_TRY(hipDeviceSynchronize(), SVO_EDEVICE);
    Node* dn = reinterpret_cast<Node*>(t->d_nodes);
    if (t->nodes.size() > t->synced_nodes)
        HIP_TRY(hipMemcpy(dn + t->synced_nodes, t->nodes.data() + t->synced_nodes, (t->nodes.size() - t->synced_nodes) * sizeof(Node),
                          hipMemcpyHostToDevice), SVO_EDEVICE);
    if (t->mats.size() > t->synced_mats)
        HIP_TRY(hipMemcpy(reinterpret_cast<uint16_t*>(t->d_mats) + t->synced_mats, t->mats.data() + t->synced_mats,
                          (t->mats.size() - t->synced_mats) * sizeof(uint16_t), hipMemcpyHostToDevice), SVO_EDEVICE);
    for (const auto& r : dirty_runs(t->dirty_nodes))  // runs of consecutive rewritten records
        HIP_TRY(hipMemcpy(dn + r.first, t->nodes.data() + r.first, (size_t)(r.second - r.first + 1) * sizeof(Node), hipMemcpyHostToDevice),
                SVO_EDEVICE);
    if (t->palette_dirty) {
        int rc = upload_palette(t);
        if (rc) return rc;
    }
    t->dirty_nodes.clear();
    t->synced_nodes = t->nodes.size();
    t->dev_top_y = tree_top_y(t);
    t->synced_mats = t->mats.size();
    return sync_ceilings(t);
}
