// dev_meshlight.hpp -- the emissive triangles of a mesh as lights of traceMIS (TRC_FLAG_MESH_LIGHTS, tracer_abi.h): the light set's
// rule, the sampler of a point on a light triangle through a one-level alias table, and the per-triangle area pdf.  An extension
// beyond the reference, whose traceMIS samples squareList[5] / [6] only (Render.metal:320-324).  The tables are built by
// trc_meshlight.hip; tests/meshlight_ref restates every function here on the CPU (the same bits).
#pragma once

#include "dev_vec.hpp"

namespace trcdev {

// The tables of one scene.  alias: n_lights entries {accept threshold, alias} over the light triangles in triangle order (the entry
// format of dev_envlight.hpp: a 32-bit draw below the threshold keeps the entry); tri: light k -> its triangle; pdfA: per TRIANGLE,
// the area density weight / (total * area) the sampler gives a point on it, 0 for a triangle that is not a light.
struct MeshLight {
    const uint2* alias;
    const uint32_t* tri;
    const float* pdfA;
    uint32_t n_lights;
    float p_mesh;             // probability of picking the mesh in the light pick: 1/2 with square lights, 1 without, 0 without a light
                              // triangle (and under knob mesh_light_pick = 0, which keeps n_lights and pdfA)
    uint32_t squares;         // the scene has squareList[5] and [6]
};

// area of a triangle, binary32, in this order: e1 = v1 - v0, e2 = v2 - v0, c = cross(e1, e2), A = sqrt(c.x c.x + c.y c.y + c.z c.z) / 2
TRC_DEV float mesh_tri_area(F3 v0, F3 v1, F3 v2) {
    const F3 c = cross(v1 - v0, v2 - v0);
    return sqrt_cr(dot(c, c)) / 2.0f;
}
TRC_DEV F3 mesh_tri_normal(F3 v0, F3 v1, F3 v2) { return normalize(cross(v1 - v0, v2 - v0)); }      // the geometric normal, unit length
// the weight of a triangle as a light (float64: the product of two binary32 values is exact and cannot leave the range), 0 when it is none:
// an emitter material (type_is_emitter), y = luminance of its albedo finite and > 0, area finite and > 0
TRC_DEV double mesh_light_weight(bool type_is_emitter, float y, float area) {
    const bool lit = type_is_emitter && y > 0.0f && y <= FLT_MAX && area > 0.0f && area <= FLT_MAX;
    return lit ? (double)y * (double)area : 0.0;
}
TRC_DEV void mesh_tri_load(const uint32_t* tripos /* blob + off_tripos */, uint32_t t, F3& v0, F3& v1, F3& v2) {
    const float4* p = reinterpret_cast<const float4*>(tripos) + 3 * (size_t)t;
    const float4 a = p[0], b = p[1], c = p[2];
    v0 = f3(a.x, a.y, a.z); v1 = f3(b.x, b.y, b.z); v2 = f3(c.x, c.y, c.z);
}

struct MeshSample { uint32_t tri; F3 p, n; float pdfA; };
// One sample, seen from `pos`: r0 / r1 pick the light (multiply-shift index, alias decision), f0 / f1 in [0, 1] the point: s = sqrt(f0),
// b0 = 1 - s, b1 = f1 s, p = (v0 b0 + v1 b1) + v2 ((1 - b0) - b1).  n = the geometric normal on pos's side (square_sample's copysignf).
// Requires n_lights > 0.
TRC_DEV void mesh_light_sample(const MeshLight& L, const uint32_t* tripos, uint32_t r0, uint32_t r1, float f0, float f1, F3 pos, MeshSample& ms) {
    uint32_t k = (uint32_t)(((uint64_t)r0 * L.n_lights) >> 32);
    const uint2 a = L.alias[k];
    if (r1 >= a.x) k = a.y;
    const uint32_t t = L.tri[k];
    F3 v0, v1, v2;
    mesh_tri_load(tripos, t, v0, v1, v2);
    const float s = sqrt_cr(f0), b0 = 1.0f - s, b1 = f1 * s;
    const F3 p = (v0 * b0 + v1 * b1) + v2 * ((1.0f - b0) - b1);
    const F3 n = mesh_tri_normal(v0, v1, v2);
    const F3 w = normalize(pos - p);
    ms.tri = t;
    ms.p = p;
    ms.n = n * copysignf(1.0f, dot(w, n));
    ms.pdfA = L.pdfA[t];
}

}  // namespace trcdev
