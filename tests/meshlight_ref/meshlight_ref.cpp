// meshlight_ref.cpp -- CPU restatement of the mesh's emissive triangles as lights (TRC_FLAG_MESH_LIGHTS, include/tracer_abi.h): the
// light set, the weights, Vose's alias table in its stated order, pdfA and the sampler of tracer_amd/csrc/dev_meshlight.hpp and
// trc_meshlight.hip, written again from the statement (the same bits as the kernels').  Built into the oracle library (oracle/Makefile), where the oracle's traceMISLight and meshlight_loader.py find it, with
// -ffp-contract=off.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "trc_detmath.h"

namespace {
const int kMatDiffuse = 0;      // TRC_MAT_DIFFUSE: the emitter

uint32_t threshold(double q) { return q >= 1.0 ? 0xFFFFFFFFu : (q <= 0.0 ? 0u : (uint32_t)(q * 4294967296.0)); }

void vose(const double* w, uint32_t n, double sum, uint32_t* out /* 2 n */) {
    std::vector<double> q(n);
    for (uint32_t i = 0; i < n; ++i) q[i] = sum > 0.0 ? (w[i] * (double)n) / sum : 1.0;
    std::vector<uint32_t> small, large;
    for (uint32_t i = 0; i < n; ++i) (q[i] < 1.0 ? small : large).push_back(i);
    while (!small.empty() && !large.empty()) {
        const uint32_t l = small.back(); small.pop_back();
        const uint32_t g = large.back(); large.pop_back();
        out[2 * l] = threshold(q[l]); out[2 * l + 1] = g;
        q[g] = (q[g] + q[l]) - 1.0;
        (q[g] < 1.0 ? small : large).push_back(g);
    }
    while (!large.empty()) { const uint32_t g = large.back(); large.pop_back(); out[2 * g] = 0xFFFFFFFFu; out[2 * g + 1] = g; }
    while (!small.empty()) { const uint32_t l = small.back(); small.pop_back(); out[2 * l] = 0xFFFFFFFFu; out[2 * l + 1] = l; }
}

struct V3 { float x, y, z; };
V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 crs(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float dt(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 nrm(V3 a) { const float inv = 1.0f / sqrtf(dt(a, a)); return V3{a.x * inv, a.y * inv, a.z * inv}; }
V3 vert(const float* tri_v, uint32_t t, int k) { const float* p = tri_v + 9 * (size_t)t + 3 * k; return V3{p[0], p[1], p[2]}; }
float area(const float* tri_v, uint32_t t) {
    const V3 v0 = vert(tri_v, t, 0), c = crs(sub(vert(tri_v, t, 1), v0), sub(vert(tri_v, t, 2), v0));
    return sqrtf(dt(c, c)) / 2.0f;
}
}  // namespace

extern "C" {
// tri_v: 9 floats per triangle (v0, v1, v2 as uploaded); tri_mat: material index per triangle; mat_type / mat_albedo: the material table.
// Out: alias (2 per light), tri (per light), pdfA (per triangle), total, n_lights; alias and tri have room for n_tri lights.
void meshlight_ref_tables(const float* tri_v, uint32_t n_tri, const uint32_t* tri_mat, const int32_t* mat_type, const float* mat_albedo, uint32_t n_mat,
                          uint32_t* alias, uint32_t* tri, float* pdfA, double* total, uint32_t* n_lights) {
    std::vector<double> w(n_tri), wl;
    uint32_t n = 0;
    for (uint32_t t = 0; t < n_tri; ++t) {
        w[t] = 0.0;
        const uint32_t m = tri_mat[t];
        if (m >= n_mat) continue;
        const float* a = mat_albedo + 3 * (size_t)m;
        const float y = 0.212671f * a[0] + 0.715160f * a[1] + 0.072169f * a[2];
        const float A = area(tri_v, t);
        if (mat_type[m] == kMatDiffuse && y > 0.0f && y <= FLT_MAX && A > 0.0f && A <= FLT_MAX) w[t] = (double)y * (double)A;
        if (w[t] > 0.0) { tri[n++] = t; wl.push_back(w[t]); }
    }
    double sum = 0.0;
    for (uint32_t k = 0; k < n; ++k) sum += wl[k];
    vose(wl.data(), n, sum, alias);
    for (uint32_t t = 0; t < n_tri; ++t) pdfA[t] = w[t] > 0.0 ? (float)(w[t] / (sum * (double)area(tri_v, t))) : 0.0f;
    *total = sum;
    *n_lights = n;
}

// draws: 4 words per item (2 integer draws, 2 float bit patterns), pos: 3 floats per item -> tri_out, out 7 floats (point, normal, pdfA)
void meshlight_ref_sample(const float* tri_v, const uint32_t* alias, const uint32_t* tri, const float* pdfA, uint32_t n_lights,
                          const uint32_t* draws, const float* pos, size_t n, uint32_t* tri_out, float* out) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t* d = draws + 4 * i;
        uint32_t k = (uint32_t)(((uint64_t)d[0] * n_lights) >> 32);
        if (d[1] >= alias[2 * k]) k = alias[2 * k + 1];
        const uint32_t t = tri[k];
        float f0, f1;
        std::memcpy(&f0, d + 2, 4); std::memcpy(&f1, d + 3, 4);
        const V3 v0 = vert(tri_v, t, 0), v1 = vert(tri_v, t, 1), v2 = vert(tri_v, t, 2);
        const float s = sqrtf(f0), b0 = 1.0f - s, b1 = f1 * s, b2 = (1.0f - b0) - b1;
        const V3 p{(v0.x * b0 + v1.x * b1) + v2.x * b2, (v0.y * b0 + v1.y * b1) + v2.y * b2, (v0.z * b0 + v1.z * b1) + v2.z * b2};
        const V3 g = nrm(crs(sub(v1, v0), sub(v2, v0)));
        const V3 w = nrm(sub(V3{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, p));
        const float sg = copysignf(1.0f, dt(w, g));
        tri_out[i] = t;
        float* o = out + 7 * i;
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = g.x * sg; o[4] = g.y * sg; o[5] = g.z * sg; o[6] = pdfA[t];
    }
}
}  // extern "C"
