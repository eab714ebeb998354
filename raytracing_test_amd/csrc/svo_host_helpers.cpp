// svo_host_helpers.cpp — the kernels' ray generation, hemisphere table and noise as host calls, for callers and
// tests that need the very numbers the device computes.
#include <math.h>

#include "svo_noise.h"
#include "svo_world.h"

using namespace svo;

// ================================================================================================
// Host helpers (the same code the kernel runs)
// ================================================================================================
extern "C" int svo_proj_plane(int32_t width, int32_t height, float* ppx, float* ppy) {
    if (width <= 0 || height <= 0 || !ppx || !ppy) SVO_FAIL(SVO_EINVAL, "svo_proj_plane: bad argument");
    // main.cpp:94: glm::tan(glm::radians(45.0)) in double, then the float uniforms
    const double t = tan(45.0 * 0.01745329251994329576923690768489);
    *ppx = (float)t;
    *ppy = (float)(t * (double)(float)height / (double)width);
    return SVO_OK;
}

extern "C" int svo_normalize(const float v[3], float o[3]) {
    if (!v || !o) SVO_FAIL(SVO_EINVAL, "svo_normalize: NULL argument");
    normalize3(v, o);
    return SVO_OK;
}

extern "C" int svo_pixel_dir(const float cam[3], float ppx, float ppy, int32_t w, int32_t h, int32_t px, int32_t py, float o[3]) {
    if (!cam || !o || w <= 0 || h <= 0) SVO_FAIL(SVO_EINVAL, "svo_pixel_dir: bad argument");
    RayGen g;
    raygen_init(g, cam, ppx, ppy, w, h);
    raygen_pixel(g, px, py, o);
    return SVO_OK;
}

extern "C" int svo_pixel_dirs(const float cam[3], float ppx, float ppy, int32_t w, int32_t h, float* out) {
    if (!cam || !out || w <= 0 || h <= 0) SVO_FAIL(SVO_EINVAL, "svo_pixel_dirs: bad argument");
    RayGen g;
    raygen_init(g, cam, ppx, ppy, w, h);
    parallel_for(h, 0, [&](int64_t b, int64_t e) {
        for (int64_t py = b; py < e; py++)
            for (int32_t px = 0; px < w; px++) raygen_pixel(g, px, (int32_t)py, out + 3 * ((size_t)py * w + px));
    });
    return SVO_OK;
}

extern "C" int svo_hemisphere(int32_t n, float* out) {
    if (n < 0 || n > 64 || (!out && n > 0)) SVO_FAIL(SVO_EINVAL, "svo_hemisphere: n must be in [0, 64]");
    hemisphere_table(n, out);
    return SVO_OK;
}

extern "C" int svo_noise2(int64_t seed, const double* x, const double* y, int64_t n, double* out) {
    if ((!x || !y || !out) && n > 0) SVO_FAIL(SVO_EINVAL, "svo_noise2: NULL argument");
    Simplex2 s;
    simplex2_seed(s, seed);
    for (int64_t i = 0; i < n; i++) out[i] = simplex2_eval(s.perm, x[i], y[i]);
    return SVO_OK;
}
