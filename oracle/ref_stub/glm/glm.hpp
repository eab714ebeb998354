/* Stand-in for <glm/glm.hpp>, holding only what the reference's core translation units use (globals.cpp,
 * ray_caster.cpp and the headers they include): vec3 / dvec3 / ivec3, converting construction between them,
 * component-wise - and *, scalar *, trunc, abs and normalize.
 *
 * The arithmetic is plain IEEE, one operation per component in the component's own type, with no fused or reordered
 * operations: that is what GLM's scalar (non-SIMD) code path computes for these operators.  normalize is
 * v * (1 / sqrt(dot(v, v))) with the dot product summed x, y, z in order, as GLM's inversesqrt form does.
 *
 * This header is the one thing between the pins of oracle/REFERENCE_PINS.md and "the reference as shipped": every
 * other line that ref_core runs for a lookup, a put or a cast is compiled from the reference's own files.  Of the code
 * the pins exercise, only castRayFromCam's `trunc(cameraPos)`, the vec3 -> dvec3 / ivec3 -> dvec3 conversions, and
 * `absDelta - (exact - dvec3(round)) * delta` go through it (ray_caster.cpp:59-66). */
#ifndef REF_STUB_GLM_HPP
#define REF_STUB_GLM_HPP

#include <cmath>

namespace glm {

template <class T>
struct tvec3 {
    T x, y, z;

    tvec3() : x(), y(), z() {}
    template <class A, class B, class C>
    tvec3(A a, B b, C c) : x(static_cast<T>(a)), y(static_cast<T>(b)), z(static_cast<T>(c)) {}
    template <class U>
    tvec3(const tvec3<U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
};

typedef tvec3<float> vec3;
typedef tvec3<double> dvec3;
typedef tvec3<int> ivec3;

template <class T>
inline tvec3<T> operator-(const tvec3<T>& a, const tvec3<T>& b) { return tvec3<T>(a.x - b.x, a.y - b.y, a.z - b.z); }
template <class T>
inline tvec3<T> operator*(const tvec3<T>& a, const tvec3<T>& b) { return tvec3<T>(a.x * b.x, a.y * b.y, a.z * b.z); }
template <class T>
inline tvec3<T> operator*(const tvec3<T>& a, T s) { return tvec3<T>(a.x * s, a.y * s, a.z * s); }
template <class T>
inline tvec3<T> operator*(T s, const tvec3<T>& a) { return tvec3<T>(s * a.x, s * a.y, s * a.z); }

/* scalar abs as a template, like GLM's (so that ray_caster.cpp's unqualified abs(double) resolves to it and not to the C
 * library's abs(int)), with GLM's own form x >= 0 ? x : -x: it differs from fabs only at -0.0, i.e. for an infinite
 * direction component, which the pins do not use */
template <class T>
inline T abs(T v) { return v >= static_cast<T>(0) ? v : -v; }
template <class T>
inline tvec3<T> abs(const tvec3<T>& v) { return tvec3<T>(abs(v.x), abs(v.y), abs(v.z)); }

template <class T>
inline tvec3<T> trunc(const tvec3<T>& v) { return tvec3<T>(std::trunc(v.x), std::trunc(v.y), std::trunc(v.z)); }

template <class T>
inline T dot(const tvec3<T>& a, const tvec3<T>& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <class T>
inline tvec3<T> normalize(const tvec3<T>& v) { return v * (static_cast<T>(1) / std::sqrt(dot(v, v))); }

}  // namespace glm

#endif
