// svo_bounce.h — what the shading pass's bouncing rays carry: the DDA state a straight trace hands on (RayState), the
// direction, count and tint of the bounces (Bounce) and the refracted direction (refract_dir).  Used by trace() in
// svo_trace.h (T_REFLECT, T_XS_*) and by svo_shade.h.
#pragma once

#include "svo_cast_params.h"

// A shading ray's DDA state on entering the first block it hits (the cell, crossing values, budget and last step axis):
// the straight trace before any bounce hands it to the reflection / refraction trace, which resumes from it (trace: T_XS_SAVE / T_XS_RESUME)
struct RayState {
    double T[3];
    int32_t r[3];
    int32_t steps;
    uint32_t axis;
};

// Reflections and refractions of the shading pass (reflectRay / refractRay, low_res.frag:170-240):
// direction after them, reflection count, finalColorMod (a vec3: liquid tints per channel), and
// whether the ray was bent (kBent, a bit of the reflection count's word: 28 B per lane in LDS, which with the launch's own
// path depth lets the shading instances run 7 waves per SIMD).
constexpr int32_t kBent = 1 << 30;
struct Bounce {
    float d[3];
    int32_t n;  // reflections | kBent
    float m[3];
};

// refractRay(vec3, vec3, float, float) (low_res.frag:196-209), n1 = 1.0, n2 = 1.1; dot as
// ((x + y) + z), no fused operations (-ffp-contract=off)
__device__ __forceinline__ void refract_dir(float d[3], const float nin[3]) {
    const float r = 1.0f / 1.1f;
    float n[3] = {nin[0], nin[1], nin[2]};
    float c1 = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    if (c1 < 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = -n[k];
        c1 = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    }
    const float c2 = svo::sqrt_rn(1.0f - r * r * (1.0f - c1 * c1));
    const float kf = r * c1 - c2;
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = r * d[k] + kf * n[k];
}
