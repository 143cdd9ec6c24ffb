// ref_metal_entry.cpp -- C entry points (pin_api.h, family ref_*) over the reference's OWN shader headers, TEST INFRASTRUCTURE.
//
// The headers are #included from $(REF)/RT_Metal/Metal where they lie (oracle/Makefile); no line of them is in this
// repository.  <metal_stdlib> resolves to metal_shim/metal_stdlib, our host stand-in.  The result, _ref/libmetal_ref.so, is
// what tests/test_reference_pin.py holds liboracle.so to, bit for bit, and what tests/golden/make_reference_pin.py records.
// Must be built with g++ -fsingle-precision-constant (an unsuffixed literal is a float in MSL): ref_literal_probe shows it.
#include "pin_api.h"          // before the stand-in: `device`, `thread`, `constant` are ordinary words until then

#include <stddef.h>

#include "Render.hh"          // the reference's: Scene::hit and, through it, every header below Render.metal
#include "BXDF.metal"         // the reference's: FrDielectric, FrConductor

#undef constant
#undef thread
#undef device
#undef threadgroup

// Texture.hh:37-38 names noise() (Noise.metal) in a branch that no material of the ABI reaches through these entry points
float noise(float3) { metal::trc_shim_not_callable(); }

// ---------------------------------------------------------------- layouts: SURVEY Appendix A, executable
#define SAME_SIZE(R, T) static_assert(sizeof(R) == sizeof(T) && alignof(R) <= 16, "size of " #R " is not " #T "'s")
#define SAME_OFF(R, T, m) static_assert(offsetof(R, m) == offsetof(T, m), "offset of " #R "::" #m)
static_assert(sizeof(float2) == 8 && alignof(float2) == 8 && sizeof(float3) == 16 && alignof(float3) == 16, "float2 / float3");
static_assert(sizeof(float4) == 16 && alignof(float4) == 16 && sizeof(float4x4) == 64 && alignof(float4x4) == 16, "float4 / float4x4");
static_assert(sizeof(packed_float3) == 12 && alignof(packed_float3) == 4 && sizeof(packed_float2) == 8 && alignof(packed_float2) == 4, "packed");
static_assert(sizeof(uint3) == 16 && sizeof(int3) == 16 && sizeof(uint2) == 8, "integer vectors");
SAME_SIZE(AABB, trc_AABB); SAME_OFF(AABB, trc_AABB, mini); SAME_OFF(AABB, trc_AABB, maxi);
SAME_SIZE(BVH, trc_BVH); SAME_OFF(BVH, trc_BVH, parent); SAME_OFF(BVH, trc_BVH, left); SAME_OFF(BVH, trc_BVH, right);
SAME_OFF(BVH, trc_BVH, axis); SAME_OFF(BVH, trc_BVH, pType); SAME_OFF(BVH, trc_BVH, pIndex); SAME_OFF(BVH, trc_BVH, bBOX);
SAME_SIZE(Sphere, trc_Sphere); SAME_OFF(Sphere, trc_Sphere, radius); SAME_OFF(Sphere, trc_Sphere, center);
SAME_OFF(Sphere, trc_Sphere, model_matrix); SAME_OFF(Sphere, trc_Sphere, normal_matrix); SAME_OFF(Sphere, trc_Sphere, inverse_matrix);
SAME_OFF(Sphere, trc_Sphere, material); SAME_OFF(Sphere, trc_Sphere, boundingBOX);
SAME_SIZE(Square, trc_Square); SAME_OFF(Square, trc_Square, axis_i); SAME_OFF(Square, trc_Square, axis_j);
SAME_OFF(Square, trc_Square, range_i); SAME_OFF(Square, trc_Square, range_j); SAME_OFF(Square, trc_Square, axis_k);
SAME_OFF(Square, trc_Square, value_k); SAME_OFF(Square, trc_Square, model_matrix); SAME_OFF(Square, trc_Square, normal_matrix);
SAME_OFF(Square, trc_Square, inverse_matrix); SAME_OFF(Square, trc_Square, material); SAME_OFF(Square, trc_Square, boundingBOX);
SAME_SIZE(Cube, trc_Cube); SAME_OFF(Cube, trc_Cube, model_matrix); SAME_OFF(Cube, trc_Cube, normal_matrix);
SAME_OFF(Cube, trc_Cube, inverse_matrix); SAME_OFF(Cube, trc_Cube, box); SAME_OFF(Cube, trc_Cube, material);
SAME_SIZE(TriangleVertex, trc_TriangleVertex); SAME_OFF(TriangleVertex, trc_TriangleVertex, v);
SAME_OFF(TriangleVertex, trc_TriangleVertex, n); SAME_OFF(TriangleVertex, trc_TriangleVertex, uv);
SAME_SIZE(TextureInfo, trc_TextureInfo); SAME_OFF(TextureInfo, trc_TextureInfo, type);
SAME_OFF(TextureInfo, trc_TextureInfo, textureIndex); SAME_OFF(TextureInfo, trc_TextureInfo, albedo);
SAME_SIZE(Material, trc_Material); SAME_OFF(Material, trc_Material, type); SAME_OFF(Material, trc_Material, medium);
SAME_OFF(Material, trc_Material, specular); SAME_OFF(Material, trc_Material, eta); SAME_OFF(Material, trc_Material, roughness);
SAME_OFF(Material, trc_Material, textureInfo);
SAME_SIZE(Camera, trc_Camera); SAME_OFF(Camera, trc_Camera, lookFrom); SAME_OFF(Camera, trc_Camera, lookAt); SAME_OFF(Camera, trc_Camera, viewUp);
SAME_OFF(Camera, trc_Camera, vfov); SAME_OFF(Camera, trc_Camera, aspect); SAME_OFF(Camera, trc_Camera, aperture);
SAME_OFF(Camera, trc_Camera, lenRadius); SAME_OFF(Camera, trc_Camera, focus_dist); SAME_OFF(Camera, trc_Camera, u);
SAME_OFF(Camera, trc_Camera, v); SAME_OFF(Camera, trc_Camera, w); SAME_OFF(Camera, trc_Camera, vertical);
SAME_OFF(Camera, trc_Camera, horizontal); SAME_OFF(Camera, trc_Camera, cornerLowLeft);
SAME_SIZE(GridDensityInfo, trc_GridDensityInfo);
static_assert((int)PrimitiveType::Sphere == TRC_PRIM_SPHERE && (int)PrimitiveType::Square == TRC_PRIM_SQUARE &&
              (int)PrimitiveType::Cube == TRC_PRIM_CUBE && (int)PrimitiveType::Triangle == TRC_PRIM_TRIANGLE &&
              (int)PrimitiveType::BVH == TRC_PRIM_BVH, "PrimitiveType ordinals");
static_assert((int)MaterialType::Lambert == TRC_MAT_LAMBERT && (int)MaterialType::Plastic == TRC_MAT_PLASTIC &&
              (int)MaterialType::Metal == TRC_MAT_METAL && (int)MaterialType::Glass == TRC_MAT_GLASS &&
              (int)MaterialType::_NIL_ == TRC_MAT_NIL, "MaterialType ordinals");
static_assert((int)TextureType::Constant == TRC_TEX_CONSTANT && (int)TextureType::Checker == TRC_TEX_CHECKER &&
              (int)TextureType::Noise == TRC_TEX_NOISE && (int)TextureType::Image == TRC_TEX_IMAGE, "TextureType ordinals");

namespace {

inline float3 f3(const float* p) { return float3(p[0], p[1], p[2]); }
inline float2 f2(const float* p) { return float2(p[0], p[1]); }
inline void put3(float* o, float3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
inline void put2(float* o, float2 v) { o[0] = v.x; o[1] = v.y; }

// every field the caller of a hit_test owns starts at 0 (the oracle's B-3 convention)
inline void zero(HitRecord& r) {
    r.t = 0; r.p = float3(0); r.f = false; r.gn = float3(0); r.sn = float3(0); r.uv = float2(0); r.material = 0; r.PDF = 0;
}
inline Ray raw_ray(const pin_ray& in) {     // direction as given: Ray::Ray would normalise it
    Ray r;
    r.origin = f3(in.origin);
    r.direction = f3(in.direction);
    return r;
}
inline void put_rec(pin_rec& o, bool accepted, float range_y, const HitRecord& r) {
    o.accepted = accepted ? 1 : 0;
    o.range_y = range_y;
    o.t = r.t;
    put3(o.p, r.p); put3(o.gn, r.gn); put3(o.sn, r.sn); put2(o.uv, r.uv);
    o.material = r.material;
    o.PDF = r.PDF;
    o.f = r.f ? 1 : 0;
}

template <typename Prim, typename Abi>
void prim_hit(const Abi* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) {
    const Prim* list = reinterpret_cast<const Prim*>(prim);
    for (size_t i = 0; i < n; ++i) {
        Ray ray = raw_ray(rays[i]);
        float2 range_t = f2(rays[i].range);
        HitRecord rec;
        zero(rec);
        bool ok = list[i % n_prim].hit_test(ray, range_t, rec);
        put_rec(out[i], ok, range_t.y, rec);
    }
}

}  // namespace

extern "C" {

PIN_API(ref)

float ref_literal_probe(float u, float v) { float w = 1.0 - u - v; return w; }

void ref_sphere_hit(const trc_Sphere* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) { prim_hit<Sphere>(prim, n_prim, rays, n, out); }
void ref_square_hit(const trc_Square* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) { prim_hit<Square>(prim, n_prim, rays, n, out); }
void ref_cube_hit(const trc_Cube* prim, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) { prim_hit<Cube>(prim, n_prim, rays, n, out); }
void ref_triangle_hit(const trc_TriangleVertex* tri, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) {
    const TriangleVertex* tv = reinterpret_cast<const TriangleVertex*>(tri);
    for (size_t i = 0; i < n; ++i) {
        Ray ray = raw_ray(rays[i]);
        float2 range_t = f2(rays[i].range);
        HitRecord rec;
        zero(rec);
        uint3 abc(0, 1, 2);
        Triangle t(tv + 3 * (i % n_prim), abc);
        bool ok = t.hit_test(ray, range_t, rec);
        put_rec(out[i], ok, range_t.y, rec);
    }
}

void ref_aabb_hit(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, int32_t* out) {
    const AABB* b = reinterpret_cast<const AABB*>(box);
    for (size_t i = 0; i < n; ++i) {
        Ray ray = raw_ray(rays[i]);
        float2 range_t = f2(rays[i].range);
        out[i] = b[i % n_prim].hit(ray, range_t) ? 1 : 0;
    }
}
void ref_aabb_hit_t_n(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, int32_t* out, float* t_out) {
    const AABB* b = reinterpret_cast<const AABB*>(box);
    for (size_t i = 0; i < n; ++i) {
        Ray ray = raw_ray(rays[i]);
        float2 range_t = f2(rays[i].range);
        float t = range_t.y;
        out[i] = b[i % n_prim].hit_t(ray, range_t, t) ? 1 : 0;
        t_out[i] = t;
    }
}
void ref_aabb_hit_record(const trc_AABB* box, size_t n_prim, const pin_ray* rays, size_t n, pin_rec* out) {
    const AABB* b = reinterpret_cast<const AABB*>(box);
    for (size_t i = 0; i < n; ++i) {
        Ray ray = raw_ray(rays[i]);
        float2 range_t = f2(rays[i].range);
        HitRecord rec;
        zero(rec);
        bool ok = b[i % n_prim].hit(ray, range_t, rec);
        put_rec(out[i], ok, range_t.y, rec);
    }
}

void ref_scene_hit(const trc_scene* scene, const trc_ray* rays, size_t n, int any_hit, pin_rec* out) {
    Primitive prims;
    prims.sphereList = reinterpret_cast<const Sphere*>(scene->sphereList);
    prims.squareList = reinterpret_cast<const Square*>(scene->squareList);
    prims.cubeList = reinterpret_cast<const Cube*>(scene->cubeList);
    prims.triList = reinterpret_cast<const TriangleVertex*>(scene->triList);
    prims.idxList = scene->idxList;
    prims.bvhList = reinterpret_cast<const BVH*>(scene->bvhList);
    Scene sc{prims};
    for (size_t i = 0; i < n; ++i) {
        Ray ray(f3(rays[i].origin), f3(rays[i].direction));
        HitRecord rec;
        zero(rec);
        bool ok = sc.hit(ray, rec, rays[i].tmax, any_hit != 0);
        put_rec(out[i], ok, 0.0f, rec);
    }
}

void ref_square_sample(const trc_Square* prim, size_t n_prim, const float* u2, const float* pos3, size_t n, float* out8) {
    const Square* list = reinterpret_cast<const Square*>(prim);
    for (size_t i = 0; i < n; ++i) {
        LightSampleRecord lsr;
        lsr.p = float3(0); lsr.n = float3(0); lsr.areaPDF = 0; lsr.material = 0;
        float2 u = f2(u2 + 2 * i);
        float3 pos = f3(pos3 + 3 * i);
        list[i % n_prim].sample(u, pos, lsr);
        put3(out8 + 8 * i, lsr.p); put3(out8 + 8 * i + 3, lsr.n);
        out8[8 * i + 6] = lsr.areaPDF;
        out8[8 * i + 7] = as_type<float>(lsr.material);
    }
}
void ref_triangle_sample(const trc_TriangleVertex* tri, size_t n_prim, const float* u2, size_t n, float* out7) {
    const TriangleVertex* tv = reinterpret_cast<const TriangleVertex*>(tri);
    for (size_t i = 0; i < n; ++i) {
        LightSampleRecord lsr;
        lsr.p = float3(0); lsr.n = float3(0); lsr.areaPDF = 0; lsr.material = 0;
        uint3 abc(0, 1, 2);
        Triangle t(tv + 3 * (i % n_prim), abc);
        float2 uu = f2(u2 + 2 * i);
        t.sample(uu, lsr);
        put3(out7 + 7 * i, lsr.p); put3(out7 + 7 * i + 3, lsr.n);
        out7[7 * i + 6] = lsr.areaPDF;
    }
}
void ref_triangle_area(const trc_TriangleVertex* tri, size_t n, float* out) {
    const TriangleVertex* tv = reinterpret_cast<const TriangleVertex*>(tri);
    for (size_t i = 0; i < n; ++i) {
        uint3 abc(0, 1, 2);
        Triangle t(tv + 3 * i, abc);
        out[i] = t.area();
    }
}

void ref_offset_ray_n(const float* p3, const float* n3, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) put3(out3 + 3 * i, offset_ray(f3(p3 + 3 * i), f3(n3 + 3 * i)));
}
void ref_next_float_up(const float* x, size_t n, float* out) { for (size_t i = 0; i < n; ++i) out[i] = NextFloatUp(x[i]); }
void ref_next_float_down(const float* x, size_t n, float* out) { for (size_t i = 0; i < n; ++i) out[i] = NextFloatDown(x[i]); }
void ref_erf_n(const float* x, size_t n, float* out) { for (size_t i = 0; i < n; ++i) out[i] = Erf(x[i]); }
void ref_erfinv_n(const float* x, size_t n, float* out) { for (size_t i = 0; i < n; ++i) out[i] = ErfInv(x[i]); }
float ref_gamma(int n) { return gamma(n); }

void ref_cosine_sample_hemisphere_n(const float* u2, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) { float2 u = f2(u2 + 2 * i); put3(out3 + 3 * i, CosineSampleHemisphere(u)); }
}
void ref_concentric_sample_disk(const float* u2, size_t n, float* out2) {
    for (size_t i = 0; i < n; ++i) { float2 u = f2(u2 + 2 * i); put2(out2 + 2 * i, ConcentricSampleDisk(u)); }
}
void ref_uniform_sample_triangle(const float* u2, size_t n, float* out2) {
    for (size_t i = 0; i < n; ++i) { float2 u = f2(u2 + 2 * i); put2(out2 + 2 * i, UniformSampleTriangle(u)); }
}
void ref_power_heuristic_n(int nf, const float* fPdf, int ng, const float* gPdf, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = PowerHeuristic(nf, fPdf[i], ng, gPdf[i]);
}
void ref_coordinate_system(const float* a3, size_t n, float* out6) {
    for (size_t i = 0; i < n; ++i) {
        float3 a = f3(a3 + 3 * i), b(0), c(0);
        CoordinateSystem(a, b, c);
        put3(out6 + 6 * i, b); put3(out6 + 6 * i + 3, c);
    }
}
void ref_spherical_direction(const float* scp, const float* xyz9, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) {
        float3 x = f3(xyz9 + 9 * i), y = f3(xyz9 + 9 * i + 3), z = f3(xyz9 + 9 * i + 6);
        put3(out3 + 3 * i, SphericalDirection(scp[3 * i], scp[3 * i + 1], scp[3 * i + 2], x, y, z));
    }
}
void ref_phase_hg_n(const float* cosTheta, const float* g, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = PhaseHG(cosTheta[i], g[i]);
}
void ref_hg_sample_n(const float* g, const float* wo3, const float* uu2, size_t n, float* out4) {
    for (size_t i = 0; i < n; ++i) {
        HenyeyGreenstein hg(g[i]);
        float3 wo = f3(wo3 + 3 * i), wi(0);
        float2 uu = f2(uu2 + 2 * i);
        out4[4 * i + 3] = hg.Sample_p(wo, wi, uu);
        put3(out4 + 4 * i, wi);
    }
}

void ref_fr_dielectric_n(const float* cosi, const float* eta, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = FrDielectric(cosi[i], eta[i]).x;
}
void ref_fr_conductor_n(const float* cosi, const float* eta3, const float* k3, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) { float3 e = f3(eta3 + 3 * i), k = f3(k3 + 3 * i); put3(out3 + 3 * i, FrConductor(cosi[i], e, k)); }
}
void ref_reflect(const float* wo3, const float* n3, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) { float3 wo = f3(wo3 + 3 * i), nn = f3(n3 + 3 * i); put3(out3 + 3 * i, Reflect(wo, nn)); }
}
void ref_refract(const float* wo3, const float* n3, const float* eta, size_t n, float* out4) {
    for (size_t i = 0; i < n; ++i) {
        float3 wo = f3(wo3 + 3 * i), nn = f3(n3 + 3 * i), wi(0);
        out4[4 * i] = Refract(wo, nn, eta[i], wi) ? 1.0f : 0.0f;
        put3(out4 + 4 * i + 1, wi);
    }
}

void ref_material_f_n(const trc_Material* m, const float* wo3, const float* wi3, const float* uv2, const float* uu2, size_t n, float* out4) {
    const Material* mat = reinterpret_cast<const Material*>(m);
    for (size_t i = 0; i < n; ++i) {
        float3 wo = f3(wo3 + 3 * i), wi = f3(wi3 + 3 * i);
        float2 uv = f2(uv2 + 2 * i), uu = f2(uu2 + 2 * i);
        float pdf = 0;
        put3(out4 + 4 * i, mat->F(wo, wi, uv, pdf, uu));
        out4[4 * i + 3] = pdf;
    }
}
void ref_material_pdf_n(const trc_Material* m, const float* wo3, const float* wi3, const float* uu2, size_t n, float* out) {
    const Material* mat = reinterpret_cast<const Material*>(m);
    for (size_t i = 0; i < n; ++i) {
        float3 wo = f3(wo3 + 3 * i), wi = f3(wi3 + 3 * i);
        float2 uu = f2(uu2 + 2 * i);
        out[i] = mat->PDF(wo, wi, uu);
    }
}
void ref_material_s_f_n(const trc_Material* m, const float* wo3, const float* uv2, const float* uu2, size_t n, float* out7) {
    const Material* mat = reinterpret_cast<const Material*>(m);
    for (size_t i = 0; i < n; ++i) {
        float3 wo = f3(wo3 + 3 * i), wi(0);
        float2 uv = f2(uv2 + 2 * i), uu = f2(uu2 + 2 * i);
        float pdf = 0;
        float3 f = mat->S_F(wo, wi, uv, uu, pdf);
        put3(out7 + 7 * i, wi); put3(out7 + 7 * i + 3, f);
        out7[7 * i + 6] = pdf;
    }
}

void ref_microfacet(int dist, float ax, float ay, const float* wo3, const float* wh3, const float* uu2, size_t n, float* out8) {
    Beckmann bk(ax, ay);
    TrowbridgeReitz tr(ax, ay);
    for (size_t i = 0; i < n; ++i) {
        float3 wo = f3(wo3 + 3 * i), wh = f3(wh3 + 3 * i);
        float2 uu = f2(uu2 + 2 * i);
        float* o = out8 + 8 * i;
        if (dist == 0) {
            o[0] = bk.D(wh); o[1] = bk.G(wo, wh); o[2] = bk.G1(wo); o[3] = bk.PDF(wo, wh);
            put3(o + 4, bk.sample_wh(wo, uu));
            o[7] = 0.0f;
        } else {
            o[0] = tr.D(wh); o[1] = tr.G(wo, wh); o[2] = tr.G1(wo); o[3] = tr.PDF(wo, wh);
            put3(o + 4, tr.sample_wh(wo, uu));
            o[7] = tr.Lambda(wo);
        }
    }
}

}  // extern "C"
