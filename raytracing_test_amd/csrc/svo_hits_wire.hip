// svo_hits_wire.hip — the hit records' wire format (svo_wire.h) outside the cast kernel: the pack / unpack kernels and
// the svo_wire_* / svo_hits_* entry points of include/svo_rt.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "svo_hip.h"
#include "svo_wire.h"

using namespace svo;

// ================================================================================================
// wire records of the tile-row gather (svo_wire.h: 8 B compact, 12 B general)
// ================================================================================================
// 8-B records for frame descs from integral / half-integral camera positions (every crossing sum exact)
int32_t svo::wire_bytes_for(const svo_tree* t, const svo_cast_desc* d) {
    if (d->ray_dirs || d->steps > 32767 || t->palette.size() > 4096) return 12;
    const int32_t nf = d->n_frames > 1 ? d->n_frames : 1;
    for (int32_t f = 0; f < nf; f++)
        for (int k = 0; k < 3; k++) {
            const float o = nf > 1 ? d->frame_origins[3 * f + k] : d->origin[k];
            if (!(2.0f * o == __builtin_truncf(2.0f * o) && __builtin_fabsf(o) < 1073741824.0f)) return 12;
        }
    return 8;
}

int svo::wire_params(const svo_tree* t, const svo_cast_desc* d, const char* fn, WireParams& Q) {
    if (!t || !d) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": NULL argument");
    if (t->device < 0) SVO_FAIL(SVO_ESTATE, std::string(fn) + ": tree not uploaded (svo_upload)");
    if (d->steps < 0 || d->steps > 32767) SVO_FAIL(SVO_ERANGE, std::string(fn) + ": the wire formats need steps <= 32767");
    if (t->palette.size() > 4096) SVO_FAIL(SVO_ERANGE, std::string(fn) + ": the wire formats need at most 4096 materials");
    memset(&Q, 0, sizeof(Q));
    int64_t n = 0;
    int rc = svo_cast_count(d, &n);
    if (rc) return rc;
    if (n >= ((int64_t)1 << 32) - 256) SVO_FAIL(SVO_ERANGE, std::string(fn) + ": too many records for one launch");
    Q.n = n;
    Q.steps = d->steps;
    Q.explicit_mode = d->ray_dirs != nullptr;
    Q.compact = wire_bytes_for(t, d) == 8;
    const int32_t nf = (!Q.explicit_mode && d->n_frames > 1) ? d->n_frames : 1;
    Q.frame_records = std::max<int64_t>(1, n / nf);
    for (int32_t f = 0; f < nf; f++)
        for (int k = 0; k < 3; k++) Q.frame_org[3 * f + k] = nf > 1 ? d->frame_origins[3 * f + k] : d->origin[k];
    Q.rorg = Q.explicit_mode ? d->ray_origins : nullptr;
    if (!Q.explicit_mode) {
        raygen_init(Q.rg, d->cam_dir, d->ppx, d->ppy, d->width, d->height);
        Q.width = d->width;
        Q.tile_row_start = d->tile_row_start;
        Q.tile_row_step = d->tile_row_step;
        Q.frame_pixels = (int64_t)d->width * d->height;
    }
    return SVO_OK;
}

namespace {

__global__ __launch_bounds__(256) void k_hits_pack(const WireParams Q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.n) return;
    float o[3];
    wire_origin(Q, i, o);
    const int4 ps = reinterpret_cast<const int4*>(Q.pos)[i];
    wire_put(Q.wire, Q.compact != 0, i, o, ps.x, ps.y, ps.z, Q.t[i], Q.info[i]);
}

__global__ __launch_bounds__(256) void k_hits_unpack(const WireParams Q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.n) return;
    wire_get(Q, i);
}

int hits_check(const svo_hits* h, const char* fn) {
    if (!h || !h->pos_steps || !h->t || !h->info) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": NULL hit buffer");
    return SVO_OK;
}

}  // namespace

extern "C" int svo_wire_bytes(const svo_tree* t, const svo_cast_desc* d, int32_t* bytes) {
    if (!t || !d || !bytes) SVO_FAIL(SVO_EINVAL, "svo_wire_bytes: NULL argument");
    *bytes = wire_bytes_for(t, d);
    return SVO_OK;
}

extern "C" int svo_hits_pack(const svo_tree* t, const svo_cast_desc* d, const svo_hits* hits, void* wire, void* stream) {
    WireParams Q;
    int rc = wire_params(t, d, "svo_hits_pack", Q);
    if (!rc) rc = hits_check(hits, "svo_hits_pack");
    if (rc) return rc;
    if (!wire) SVO_FAIL(SVO_EINVAL, "svo_hits_pack: NULL wire buffer");
    Q.pos = hits->pos_steps;
    Q.t = hits->t;
    Q.info = hits->info;
    Q.wire = reinterpret_cast<uint32_t*>(wire);
    if (Q.n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    hipLaunchKernelGGL(k_hits_pack, dim3((uint32_t)((Q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return SVO_OK;
}

// unpack into record order (scatter = 0) or into the whole frames at pixel positions (scatter = 1)
static int wire_decode(const svo_tree* t, const svo_cast_desc* d, const void* wire, const uint8_t* ao, const svo_hits* hits, void* stream,
                       int32_t scatter, const char* fn) {
    WireParams Q;
    int rc = wire_params(t, d, fn, Q);
    if (!rc) rc = hits_check(hits, fn);
    if (rc) return rc;
    if (!wire) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": NULL wire buffer");
    if (scatter && Q.explicit_mode) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": explicit rays have no pixels to scatter to");
    if (ao && !hits->ao) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": AO counts without an ao buffer");
    Q.wire = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(wire));
    Q.pos = hits->pos_steps;
    Q.t = hits->t;
    Q.info = hits->info;
    Q.ao_in = ao;
    Q.ao_out = ao ? hits->ao : nullptr;
    Q.scatter = scatter;
    if (Q.n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(t->device), SVO_EDEVICE);
    hipLaunchKernelGGL(k_hits_unpack, dim3((uint32_t)((Q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError(), SVO_EDEVICE);
    return SVO_OK;
}

extern "C" int svo_hits_unpack(const svo_tree* t, const svo_cast_desc* d, const void* wire, const svo_hits* hits, void* stream) {
    return wire_decode(t, d, wire, nullptr, hits, stream, 0, "svo_hits_unpack");
}

extern "C" int svo_wire_scatter(const svo_tree* t, const svo_cast_desc* d, const void* wire, const uint8_t* ao, const svo_hits* frames,
                                void* stream) {
    return wire_decode(t, d, wire, ao, frames, stream, 1, "svo_wire_scatter");
}
