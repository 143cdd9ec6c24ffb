/*
 * pin_api.h -- the unit entry points that exist twice (TEST INFRASTRUCTURE): as orc_* in liboracle.so, over the oracle's
 * restatement (oracle.cpp), and as ref_* in _ref/libmetal_ref.so, over the reference's own shader headers compiled on the
 * host (ref_metal_entry.cpp + metal_shim/).  PIN_API(P) declares one family, so the two cannot differ in a signature.
 * tests/test_reference_pin.py compares their outputs bit for bit.
 *
 * All are batches: plain C, arrays in and out, no global state, item i of every array belongs to call i.  Where an
 * array of primitives is passed with a count (n_prim), call i uses primitive i % n_prim.  Outputs the callee does not
 * write keep the 0 they start with (the oracle's B-3 convention), except where the reference itself works on an
 * uninitialised local (Cube::hit_test; see the table at the top of tests/test_reference_pin.py).
 * Where oracle.h already has a one-item function of the name, the batch carries the suffix _n.
 */
#ifndef ORACLE_PIN_API_H
#define ORACLE_PIN_API_H

#include "tracer_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a ray as the primitive tests see it: direction taken as it is (Ray::Ray would normalise it), range_t = (x, y) */
typedef struct pin_ray { float origin[3]; float direction[3]; float range[2]; } pin_ray;            /* 32 B */
/* what a hit_test leaves: its return value, range_t.y after the call, and HitRecord (HitRecord.hh:9-24) */
typedef struct pin_rec {
    int32_t  accepted;
    float    range_y;
    float    t;
    float    p[3], gn[3], sn[3];
    float    uv[2];
    uint32_t material;
    float    PDF;
    int32_t  f;
} pin_rec;                                                                                           /* 68 B */

#define PIN_API(P)                                                                                                              \
    /* 1.0 - u - v as the library's compiler reads it (Triangle.hh:68): two float subtractions in MSL */                       \
    float P##_literal_probe(float u, float v);                                                                                  \
    /* Sphere.hh:33-78, Square.hh:60-113, Cube.hh:17-47, Triangle.hh:31-85 (tri: 3 vertices per triangle) */                  \
    void P##_sphere_hit(const trc_Sphere* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out);                    \
    void P##_square_hit(const trc_Square* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out);                    \
    void P##_cube_hit(const trc_Cube* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out);                        \
    void P##_triangle_hit(const trc_TriangleVertex* tri, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out);           \
    /* AABB.hh:73-90, 92-112 (t starts at range.y, as Scene::hit passes it), 114-209 (writes t, p, gn, uv only) */            \
    void P##_aabb_hit(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, int32_t* out);                         \
    void P##_aabb_hit_t_n(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, int32_t* out, float* t_out);       \
    void P##_aabb_hit_record(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out);                  \
    /* Scene::hit, Render.hh:135-252; rays as orc_trace_rays takes them (Ray::Ray normalises); range_y is unused (0) */        \
    void P##_scene_hit(const trc_scene* scene, const trc_ray* rays, size_t n, int any_hit, pin_rec* out);                       \
    /* Square.hh:40-58 -> p[3] n[3] areaPDF material(as bits); Triangle.hh:87-128 -> p[3] n[3] areaPDF; area */                \
    void P##_square_sample(const trc_Square* prim, size_t n_prim, const float* u2, const float* pos3, size_t n, float* out8);   \
    void P##_triangle_sample(const trc_TriangleVertex* tri, size_t n_prim, const float* u2, size_t n, float* out7);             \
    void P##_triangle_area(const trc_TriangleVertex* tri, size_t n, float* out);                                                \
    /* Math.hh */                                                                                                               \
    void  P##_offset_ray_n(const float* p3, const float* n3, size_t n, float* out3);                                            \
    void  P##_next_float_up(const float* x, size_t n, float* out);                                                              \
    void  P##_next_float_down(const float* x, size_t n, float* out);                                                            \
    void  P##_erf_n(const float* x, size_t n, float* out);                                                                      \
    void  P##_erfinv_n(const float* x, size_t n, float* out);                                                                   \
    float P##_gamma(int n);                                                                                                     \
    /* Sampling.hh, HitRecord.hh:45-79 */                                                                                       \
    void P##_cosine_sample_hemisphere_n(const float* u2, size_t n, float* out3);                                                \
    void P##_concentric_sample_disk(const float* u2, size_t n, float* out2);                                                    \
    void P##_uniform_sample_triangle(const float* u2, size_t n, float* out2);                                                   \
    void P##_power_heuristic_n(int nf, const float* fPdf, int ng, const float* gPdf, size_t n, float* out);                     \
    void P##_coordinate_system(const float* a3, size_t n, float* out6);                                                         \
    void P##_spherical_direction(const float* sin_cos_phi3, const float* xyz9, size_t n, float* out3);                          \
    void P##_phase_hg_n(const float* cosTheta, const float* g, size_t n, float* out);                                           \
    void P##_hg_sample_n(const float* g, const float* wo3, const float* uu2, size_t n, float* out4 /* wi[3] p */);              \
    /* BXDF.metal:3-34, BXDF.hh:24-41 (Refract -> ok wi[3]) */                                                                 \
    void P##_fr_dielectric_n(const float* cosi, const float* eta, size_t n, float* out);                                        \
    void P##_fr_conductor_n(const float* cosi, const float* eta3, const float* k3, size_t n, float* out3);                      \
    void P##_reflect(const float* wo3, const float* n3, size_t n, float* out3);                                                 \
    void P##_refract(const float* wo3, const float* n3, const float* eta, size_t n, float* out4);                               \
    /* Material.hh:77-146 -> f[3] pdf; pdf; wi[3] f[3] pdf */                                                                  \
    void P##_material_f_n(const trc_Material* m, const float* wo3, const float* wi3, const float* uv2, const float* uu2,        \
                          size_t n, float* out4);                                                                               \
    void P##_material_pdf_n(const trc_Material* m, const float* wo3, const float* wi3, const float* uu2, size_t n, float* out); \
    void P##_material_s_f_n(const trc_Material* m, const float* wo3, const float* uv2, const float* uu2, size_t n, float* out7);\
    /* MicrofacetBXDF.h:137-434, dist 0 Beckmann(ax, ay), 1 TrowbridgeReitz(ax, ay) ->                                          \
     * D(wh) G(wo, wh) G1(wo) PDF(wo, wh) sample_wh(wo, uu)[3] Lambda(wo) (Beckmann's Lambda is private there: 0) */           \
    void P##_microfacet(int dist, float ax, float ay, const float* wo3, const float* wh3, const float* uu2, size_t n, float* out8);

#ifdef __cplusplus
}
#endif
#endif
