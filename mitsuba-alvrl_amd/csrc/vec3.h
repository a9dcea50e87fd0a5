// vec3.h -- the 3-vector and the triangle test that every side shares: the
// host tracer and the device tracer (through transport.h) and the BVH queries
// of bvh_device.hpp, which the gather, the refinement and the strict R build
// compile under their own flags.  It has no transcendental function and
// includes nothing but the C headers, so a translation unit built with FMA
// contraction can take it without reaching detmath.h.  Each expression keeps
// its association; plain C++17 under g++, __host__ __device__ under hipcc.
#ifndef ALVRL_VEC3_H
#define ALVRL_VEC3_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define TP_M __host__ __device__
#else
#define TP_M
#endif
#define TP_FN static inline TP_M

namespace alvrl {
namespace transport {

struct V3 { float x, y, z; };

TP_FN V3 v3(float x, float y, float z) { return V3{x, y, z}; }
TP_FN V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
TP_FN V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
TP_FN V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
TP_FN V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
TP_FN float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TP_FN float length(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
TP_FN V3 normalize(V3 a) { const float r = 1.0f / length(a); return a * r; }
TP_FN V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// TriangleT::rayIntersect (triangle.h:109-145): t of the hit, or false.
TP_FN bool tri_intersect(const float* tri, V3 o, V3 d, float* u, float* v, float* t)
{
    const V3 p0 = v3(tri[0], tri[1], tri[2]), p1 = v3(tri[3], tri[4], tri[5]), p2 = v3(tri[6], tri[7], tri[8]);
    const V3 edge1 = p1 - p0, edge2 = p2 - p0;
    const V3 pvec = cross(d, edge2);
    const float det = dot(edge1, pvec);
    if (det == 0) return false;
    const float inv_det = 1.0f / det;
    const V3 tvec = o - p0;
    *u = dot(tvec, pvec) * inv_det;
    if (*u < 0.0f || *u > 1.0f) return false;
    const V3 qvec = cross(tvec, edge1);
    *v = dot(d, qvec) * inv_det;
    if (*v >= 0.0f && *u + *v <= 1.0f) {   // inverted comparison (catches NaNs)
        *t = dot(edge2, qvec) * inv_det;
        return true;
    }
    return false;
}

}  // namespace transport
}  // namespace alvrl

#endif
