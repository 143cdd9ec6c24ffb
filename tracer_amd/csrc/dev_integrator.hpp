// dev_integrator.hpp -- camera ray, tracePath / traceMIS and the per-pixel accumulation loop.
//
// Reference (RT_Metal/Metal/): Random.metal:3-26, RandomSampler.hh:6-46, Camera.hh:59-69,
// Render.metal:277-409 (traceMIS), :411-492 (tracePath), :495-558 (kernelPathTracing).
#pragma once

#include "dev_bsdf.hpp"
#include "dev_envlight.hpp"
#include "dev_intersect.hpp"
#include "dev_meshlight.hpp"
#include "trc_sobol.h"

#include <type_traits>

// traceVolume: steps of the GridDensity medium's delta tracker a lane takes per iteration of the render loop before the other lanes
// get their next Scene::hit (dev_integrator.hpp grid_sample); 0 = the whole tracker at once
#ifndef TRC_TRACK_SLICE
#define TRC_TRACK_SLICE 20
#endif

namespace trcdev {

// ---------------------------------------------------------------- PCG32 (Random.metal:3-26)
struct Pcg { uint64_t state, inc; };
TRC_DEV uint32_t pcg_next(Pcg& r) {
    uint64_t old = r.state;
    r.state = old * 6364136223846793005ULL + r.inc;
    uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((0u - rot) & 31));
}
// randomF: ldexp(float(u32), -32); float(u32) rounds to nearest-even so 1.0f is reachable (B-4)
TRC_DEV float pcg_float(Pcg& r) { return ldexpf((float)pcg_next(r), -32); }

// Work counters of a lane (rays, shaded hits): a register, or -- in the kernels that park per-pixel state in LDS
// (trc_render_kernels.hpp: PARK) -- a word of the lane's LDS column bumped by one ds_add_u32, which costs no register at all.
struct LdsCount { uint32_t* p; };
TRC_DEV void bump(uint32_t& c) { c++; }
TRC_DEV void bump(LdsCount& c) { (void)__hip_atomic_fetch_add(c.p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// image textures (trc_upload_textures): one pool of RGB float texels, rows bottom-up, and per image {first texel, w, h, 0};
// n = images uploaded.  Read only by the TEX instantiations (hit_color<true>).
struct TexTable { const float* texels; const uint4* desc; uint32_t n; };
struct Shade {            // what the integrators need from the material table
    const uint32_t* mats; // kMaterialDwords per material: type, texType, albedo.rgb, specular, medium, textureIndex
};
TRC_DEV int mat_type(const Shade& sh, uint32_t m) { return (int)sh.mats[m * kMaterialDwords]; }
TRC_DEV int mat_tex(const Shade& sh, uint32_t m) { return (int)sh.mats[m * kMaterialDwords + 1]; }
TRC_DEV bool mat_specular(const Shade& sh, uint32_t m) { return sh.mats[m * kMaterialDwords + 5] != 0u; }
TRC_DEV int mat_medium(const Shade& sh, uint32_t m) { return (int)sh.mats[m * kMaterialDwords + 6]; }
TRC_DEV F3 mat_albedo(const Shade& sh, uint32_t m) {
    const uint32_t* p = sh.mats + m * kMaterialDwords;
    return f3(__uint_as_float(p[2]), __uint_as_float(p[3]), __uint_as_float(p[4]));
}
// bilinear, clamp-to-edge lookup of level 0 of an RGB float image whose row 0 is at v = 0 (the reference's textureSampler,
// Common.hh:11): texHDR through env_radiance and the image textures through hit_color<true>
struct RgbImage { const float* rgb; uint32_t w, h; };        // 3*w*h floats, row 0 at v = 0
TRC_DEV F3 bilinear_rgb(const RgbImage& em, float u, float v) {
    const float x = u * (float)em.w - 0.5f, y = v * (float)em.h - 0.5f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float fx = x - fx0, fy = y - fy0;
    auto clampi = [](float f, uint32_t n) { return f < 0.0f ? 0u : (f > (float)(n - 1) ? n - 1 : (uint32_t)f); };
    const uint32_t x0 = clampi(fx0, em.w), x1 = clampi(fx0 + 1.0f, em.w);
    const uint32_t y0 = clampi(fy0, em.h), y1 = clampi(fy0 + 1.0f, em.h);
    auto texel = [&](uint32_t xx, uint32_t yy) { const float* t = em.rgb + 3 * ((size_t)yy * em.w + xx); return f3(t[0], t[1], t[2]); };
    const F3 top = (1 - fx) * texel(x0, y0) + fx * texel(x1, y0);
    const F3 bot = (1 - fx) * texel(x0, y1) + fx * texel(x1, y1);
    return (1 - fy) * top + fy * bot;
}
// sample.rgb of image `index` at uv (TextureInfo::value, Texture.hh:29-35); a non-finite component is looked up as 0, and a finite
// one is clamped to [-1, 2] (u * w must stay finite; the clamp-to-edge result of any |u| beyond that is the edge texel's anyway)
TRC_DEV F3 image_sample(const TexTable& tt, uint32_t index, F2 uv) {
    const uint4 d = tt.desc[index];
    const float u = (is_nan(uv.x) || is_inf(uv.x)) ? 0.0f : fminf(fmaxf(uv.x, -1.0f), 2.0f);
    const float v = (is_nan(uv.y) || is_inf(uv.y)) ? 0.0f : fminf(fmaxf(uv.y, -1.0f), 2.0f);
    return bilinear_rgb(RgbImage{tt.texels + 3 * (size_t)d.x, d.y, d.z}, u, v);
}

// texture colour of a hit; the sphere's uv (atan2 + asin, Sphere.hh:19-31) is only materialised here,
// and only when a texture consumes it -- same value as computing it inside hit_test
// ... and so is a square's (two divisions of rec.p's in-plane coordinates, Square.hh; square_uv)
// TEX: an Image material whose textureIndex names an uploaded image takes that image's sample, not scaled by albedo
// (Texture.hh:33-34); any other Image material resolves to its albedo as without TEX (the reference's nullptr branch)
template <bool TEX = false>
TRC_DEV F3 hit_color(const SceneRef& S, const Shade& sh, const HitRec& rec, const TexTable* tt = nullptr) {
    const int tex = mat_tex(sh, rec.material);
    F2 uv = rec.uv;
    uint32_t index = 0;
    bool image = false;
    if (TEX) {
        index = sh.mats[rec.material * kMaterialDwords + 7];
        image = tex == kTexImage && index < tt->n;
    }
    if (tex == kTexChecker || image) {
        const uint32_t type = rec.tag >> kTagIndexBits;
        if (type == 0u) uv = sphere_uv(rec.gn);
        else if (type == 1u) uv = square_uv(S, rec.tag & kTagIndexMask, rec.p);
    }
    if (TEX && image) return image_sample(*tt, index, uv);
    return texture_value(tex, mat_albedo(sh, rec.material), uv);
}

TRC_DEV float rgb_to_y(F3 rgb) { return 0.212671f * rgb.x + 0.715160f * rgb.y + 0.072169f * rgb.z; }   // Spectrum.hh:186-190

// Camera.hh:59-69 + RandomSampler.hh:40-46 (sampleUnitInDisk returns a point ON the unit circle, B-2)
TRC_DEV Ray cast_ray(const DCamera& cam, float s, float t, Pcg& rng) {
    float px, py;
    do {
        float a = pcg_float(rng);
        float b = pcg_float(rng);
        px = 2.0f * a - 1.0f;
        py = 2.0f * b - 1.0f;
    } while (px * px + py * py >= 1.0f);
    float inv = rsqrt_cr(px * px + py * py);
    float rdx = cam.lenRadius * (px * inv), rdy = cam.lenRadius * (py * inv);
    F3 offset = f3(cam.u[0], cam.u[1], cam.u[2]) * rdx + f3(cam.v[0], cam.v[1], cam.v[2]) * rdy;
    F3 origin = f3(cam.lookFrom[0], cam.lookFrom[1], cam.lookFrom[2]) + offset;
    F3 sample = f3(cam.cornerLowLeft[0], cam.cornerLowLeft[1], cam.cornerLowLeft[2]) +
                f3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]) * s +
                f3(cam.vertical[0], cam.vertical[1], cam.vertical[2]) * t;
    return make_ray(origin, sample - origin);
}

// texHDR (Render.hh:25,42-48) as an equirectangular RGB float image; null -> constant radiance `ambient`
typedef RgbImage EnvMap;         // (the lookup reads it through this struct: the env-mapped kernels keep their code)
TRC_DEV F3 env_radiance(const EnvMap& em, F3 ambient, F3 direction) {
    if (!em.rgb) return ambient;
    const F3 v = normalize(direction);
    const float u = dm_atan2f(v.z, v.x) * 0.1591f + 0.5f;        // SampleSphericalMap
    const float w = dm_asinf(v.y) * 0.3183f + 0.5f;
    return bilinear_rgb(em, u, w);
}

struct PathCtx {
    SceneRef S;
    F3 root_min, root_max;
    Shade sh;
    F3 ambient;
    EnvMap env;
    uint32_t* stack;
    uint32_t* lvstack;
    uint32_t max_depth;
    // traceVolume: density grid of the GridDensity medium (PackageEnv ids 3/4, Render.hh:30-31); null when absent
    const float* density;
    trc_GridDensityInfo dinfo;
    const uint8_t* occupancy;     // 1 byte per 4x4x4 brick of the grid: 0 = every cell a lookup inside could touch is zero
    // TRC_FLAG_SOBOL: tables of include/trc_sobol.h (null otherwise)
    const uint32_t* sobol32;      // [40][52] generator matrices
    const uint64_t* sobol_vdc;    // [52] VdCSobolMatrices[m - 1], then [52] VdCSobolMatricesInv[m - 1]
    uint32_t sobol_m, sobol_res;  // log2Resolution, resolution (SobolSampler.hh:56-58)
    uint32_t sobol_xy[2];         // thread_pos within its view
};
// ... of the TEX instantiations (image textures): a struct of its own, so that the others' context keeps its layout
struct PathCtxTex : PathCtx { TexTable tex; };
// The light of a traceMIS launch besides the two squares: none, the environment map (TRC_FLAG_ENV_LIGHT, dev_envlight.hpp) or the mesh's
// emissive triangles (TRC_FLAG_MESH_LIGHTS, dev_meshlight.hpp) -- one choice, never two -- and the sampling tables that go with it
enum class Light { None, Env, Mesh };
template <Light LIGHT>
using LightTables = typename std::conditional<LIGHT == Light::Env, EnvLight, typename std::conditional<LIGHT == Light::Mesh, MeshLight, void>::type>::type;
TRC_DEV float light_p(const EnvLight& L) { return L.p_env; }        // the probability that the light pick takes this light
TRC_DEV float light_p(const MeshLight& L) { return L.p_mesh; }
// ... and the context of a (TEX, LIGHT) instantiation: the light's tables come last, behind the image table of TEX
template <bool TEX> using PathCtxBase = typename std::conditional<TEX, PathCtxTex, PathCtx>::type;
template <bool TEX, Light LIGHT = Light::None> struct PathCtxOf : PathCtxBase<TEX> { LightTables<LIGHT> light; };
template <bool TEX> struct PathCtxOf<TEX, Light::None> : PathCtxBase<TEX> {};
template <bool TEX> TRC_DEV const TexTable* ctx_tex(const PathCtx& cx) {
    if constexpr (TEX) return &static_cast<const PathCtxTex&>(cx).tex; else return nullptr;
}
template <bool TEX, Light LIGHT> TRC_DEV const LightTables<LIGHT>* ctx_light(const PathCtx& cx) {
    if constexpr (LIGHT != Light::None) return &static_cast<const PathCtxOf<TEX, LIGHT>&>(cx).light; else return nullptr;
}
// TRC_FLAG_MATERIAL_PARAMS (PARAMS instantiations: trc_render_params.hpp): the table of trc_material_params, three float4 per material,
// behind the context of the (TEX, LIGHT) instantiation -- a struct of its own again, so that every other context keeps its layout
template <bool TEX, Light LIGHT = Light::None> struct PathCtxParams : PathCtxOf<TEX, LIGHT> { const float4* mparams; };
template <bool TEX, Light LIGHT, bool PARAMS> TRC_DEV const float4* ctx_mparams(const PathCtx& cx) {
    if constexpr (PARAMS) return static_cast<const PathCtxParams<TEX, LIGHT>&>(cx).mparams; else return nullptr;
}
// Material::S_F / Material::F of a hit: the literals' lobes, or under PARAMS the lobes of entry rec.material of the table (dev_bsdf.hpp)
template <bool STATS, bool TEX, Light LIGHT, bool PARAMS>
TRC_DEV F3 hit_S_F(const PathCtx& cx, int mtype, uint32_t material, F3 color, F3 wo, F3& wi, F2 uu, float& pdf, TravCounters& cnt) {
    if constexpr (PARAMS) return material_S_F_params(mtype, color, ctx_mparams<TEX, LIGHT, true>(cx), material, wo, wi, uu, pdf);
    else return material_S_F<STATS>(mtype, color, wo, wi, uu, pdf, cnt);
}
template <bool TEX, Light LIGHT, bool PARAMS>
TRC_DEV F3 hit_F(const PathCtx& cx, int mtype, uint32_t material, F3 color, F3 wo, F3 wi, F2 uu, float& pdf) {
    if constexpr (PARAMS) return material_F_params(mtype, color, ctx_mparams<TEX, LIGHT, true>(cx), material, wo, wi, uu, pdf);
    else return material_F(mtype, color, wo, wi, uu, pdf);
}

// ---------------------------------------------------------------- path state machine
// The reference runs, per pixel and per frame, castRay -> tracePath/traceMIS (a bounce loop around
// Scene::hit).  Executed literally on a 64-wide wavefront, every lane waits for the longest path of the
// wave in every sample (measured: 14.6 % VALU lane utilisation).  Here each lane is a small state
// machine that performs ONE Scene::hit per iteration of a single flat loop and immediately starts its
// next sample when a path ends (path regeneration), so lanes stay busy until their pixel's samples
// are exhausted.  Per-path arithmetic and RNG consumption are exactly the reference's.
struct PathState {
    Ray ray;
    HitRec rec;
    F3 ratio, color;
    F3 scat_attenuation;     // traceMIS: BxRecord carried from the BSDF sample to the next hit (:364-365,395-401)
    float scat_bxPDF;
    int depth_left;          // bounce rays the do-while may still trace (Render.metal:406,489)
    bool primary;            // the ray in flight is the camera ray
    int medium;              // traceVolume: Ray::medium (Ray.hh:18) of the ray in flight
    bool from_bsdf;          // traceVolume: the ray in flight left the BSDF-sampling branch (Render.metal:255-271 applies)
    bool tracking;           // traceVolume, TRC_TRACK_SLICE: the delta tracker of the GridDensity medium is part-way (grid_sample_slice)
    float trk_t;
    int trk_step;
    uint64_t sobol_index;    // TRC_FLAG_SOBOL: mSobolIndex of this sample and the next dimension (SobolSampler.hh:37-41)
    uint32_t sobol_dim;
    bool env_mis;            // Light::Env: the map's light sample shares the escape of the ray in flight (a cosine lobe, light_nee)
                             // Light::Mesh: ... the mesh's light sample shares the emitter hit of the ray in flight
};

// ---------------------------------------------------------------- pbrt::SobolSampler (SobolSampler.hh:26-167)
// SobolIntervalToIndex, :126-148
TRC_DEV uint64_t sobol_interval_to_index(const PathCtx& cx, uint64_t sampleIndex) {
    const uint32_t m = cx.sobol_m;
    if (m == 0) return 0;
    uint64_t index = sampleIndex << (m << 1);
    uint64_t delta = 0;
    for (int c = 0; sampleIndex; sampleIndex >>= 1, ++c)
        if (sampleIndex & 1) delta ^= cx.sobol_vdc[c];
    uint64_t b = (((uint64_t)cx.sobol_xy[0] << m) | cx.sobol_xy[1]) ^ delta;
    for (int c = 0; b; b >>= 1, ++c)
        if (b & 1) index ^= cx.sobol_vdc[TRC_SOBOL_MATRIX_SIZE + c];
    return index;
}
// SampleDimension, :152-163 over SobolSampleFloat, :150-160 (the column walk stops at 52 columns: indices stay
// below 2^52, see oracle/oracle.cpp SobolSampleFloat)
TRC_DEV float sobol_dimension(const PathCtx& cx, uint64_t index, uint32_t dimension) {
    if (dimension >= TRC_SOBOL_DIMS) return 0;
    uint32_t v = 0;
    const uint32_t* col = cx.sobol32 + dimension * TRC_SOBOL_MATRIX_SIZE;
    for (; index != 0; index >>= 1, ++col)
        if (index & 1) v ^= *col;
    float s = fminf((float)v * 2.3283064365386963e-10f, 1.0f - FLT_EPSILON);
    if (dimension <= 1) {
        s = s * (float)cx.sobol_res + 0.0f;
        s = fminf(fmaxf(s - (float)(dimension == 0 ? cx.sobol_xy[0] : cx.sobol_xy[1]), 0.0f), 1.0f - FLT_EPSILON);
    }
    return s;
}
// XSampler::sample2D(): RandomSampler.hh:19-24 or SobolSampler.hh:67-72
template <bool SOBOL>
TRC_DEV F2 sample_2d(const PathCtx& cx, PathState& ps, Pcg& rng) {
    F2 uu;
    if (SOBOL) {
        uu.x = sobol_dimension(cx, ps.sobol_index, ps.sobol_dim++);
        uu.y = sobol_dimension(cx, ps.sobol_index, ps.sobol_dim++);
    } else {
        uu.x = pcg_float(rng);
        uu.y = pcg_float(rng);
    }
    return uu;
}

TRC_DEV void path_begin(PathState& ps, const Ray& camera_ray, uint32_t max_depth) {
    ps.ray = camera_ray;
    hit_init(ps.rec);
    ps.ratio = f3(1.0f);
    ps.color = f3(0.0f);
    ps.scat_attenuation = f3(0.0f);
    ps.scat_bxPDF = 1.0f;
    ps.depth_left = (int)max_depth;
    ps.primary = true;
    ps.medium = TRC_MEDIUM_NIL;
    ps.from_bsdf = false;
    ps.tracking = false; ps.trk_t = 0.0f; ps.trk_step = 0;
}

// What happens between two Scene::hit calls of tracePath (Render.metal:432-489).  Returns true when the
// path is finished; `result` is then the sample's radiance.
template <bool STATS, bool SOBOL = false, bool TEX = false, class COUNT = uint32_t, bool PARAMS = false>
TRC_DEV bool path_step(const PathCtx& cx, PathState& ps, bool hitted, Pcg& rng, TravCounters& cnt, COUNT& n_shaded, F3& result) {
    if (!ps.primary) {                                               // } while ((--depth) > 0), :489
        if (--ps.depth_left <= 0) { result = ps.color; return true; }
    }
    ps.primary = false;
    if (!hitted) { result = ps.color + ps.ratio * env_radiance(cx.env, cx.ambient, ps.ray.d); return true; }        // :434-439
    HitRec& rec = ps.rec;
    const int mtype = mat_type(cx.sh, rec.material);
    if (mtype == kMatDiffuse) {                                      // emitter, :441-445
        F3 le = mat_albedo(cx.sh, rec.material);
        float w = dot(-ps.ray.d, -rec.gn);
        result = ps.ratio * le * fabsf(w);
        return true;
    }
    const F2 uu = sample_2d<SOBOL>(cx, ps, rng);                     // sample2D, :447
    const F3 hit_origin = rec.p;
    F3 _origin = offset_ray(rec.p, rec.sn);
    F3 nx, ny;
    coordinate_system(rec.sn, nx, ny);
    F3 minus_d = -ps.ray.d;
    F3 wo = f3(dot(nx, minus_d), dot(ny, minus_d), dot(rec.sn, minus_d));   // wts * (-dir)
    F3 wi = f3(0);
    float bxPDF = 0;                                                 // uninitialised in the reference (B-3)
    bump(n_shaded);
    prof<STATS>(cnt, kProfShade);
    F3 attenuation = hit_S_F<STATS, TEX, Light::None, PARAMS>(cx, mtype, rec.material, hit_color<TEX>(cx.S, cx.sh, rec, ctx_tex<TEX>(cx)), wo, wi, uu, bxPDF, cnt);
    if (bxPDF <= 0) { result = ps.color; return true; }
    F3 wiw = (nx * wi.x + ny * wi.y) + rec.sn * wi.z;                // stw * wi
    if (wi.z < 0) ps.ray = make_ray(offset_ray(hit_origin, -rec.sn), wiw);   // transmission
    else ps.ray = make_ray(_origin, wiw);
    ps.ratio = ps.ratio * div_shared(attenuation, fmaxf(FLT_EPSILON, bxPDF));
    {   // Russian roulette on luminance, :479-485
        float p = rgb_to_y(ps.ratio);
        if (pcg_float(rng) > p) { result = ps.color; return true; }
        ps.ratio = ps.ratio * rcp1(p);
    }
    return false;
}

// ---------------------------------------------------------------- participating media (traceVolume)
TRC_DEV float phase_hg(float cosTheta, float g) {                    // HitRecord.hh:45-49
    float gg = g * g;
    float denom = 1 + gg + 2 * g * cosTheta;
    return (0.25f / kPi) * (1 - gg) / (denom * sqrt_cr(denom));
}
TRC_DEV void hg_sample_p(float g, F3 wo, F3& wi, F2 uu) {            // HitRecord.hh:58-77 (the returned pdf is unused)
    float cosTheta;
    if (fabsf(g) < 1e-3f) cosTheta = 1 - 2 * uu.x;
    else {
        float gg = g * g;
        float sqrTerm = (1 - gg) / (1 + g - 2 * g * uu.x);
        cosTheta = -(1 + gg - sqrTerm * sqrTerm) / (2 * g);
    }
    float sinTheta = sqrt_cr(fmaxf(0.0f, 1 - cosTheta * cosTheta));
    float phi = 2 * kPi * uu.y;
    F3 v1, v2;
    coordinate_system(wo, v1, v2);
    float sp, cp;
    dm_sincosf(phi, &sp, &cp);
    wi = (sinTheta * cp * v1 + sinTheta * sp * v2) + cosTheta * wo;  // SphericalDirection, Sampling.hh:40-43
}
struct MediumHit { F3 p; float phaseG; bool sampled; };
// HomogeneousMedium(0.02, 0.08, 0.5).Sample, Medium.hh:38-74 / Render.metal:118-119
TRC_DEV F3 homogeneous_sample(const Ray& ray, const HitRec& rec, MediumHit& mi, Pcg& rng) {
    const F3 sigma_a = f3(0.02f), sigma_s = f3(0.08f), sigma_t = sigma_s + sigma_a;
    const int nSamples = 3;
    int channel = (int)(pcg_float(rng) * nSamples);
    if (channel > nSamples - 1) channel = nSamples - 1;
    float dist = -dm_logf(1 - pcg_float(rng)) / comp(sigma_t, (uint32_t)channel);
    float t = fminf(dist, rec.t);
    const bool sampledMedium = t < rec.t;
    const float tt = fminf(t, FLT_MAX);
    F3 Tr = f3(dm_expf(-sigma_t.x * tt), dm_expf(-sigma_t.y * tt), dm_expf(-sigma_t.z * tt));
    F3 density = Tr, result = Tr;
    if (sampledMedium) {
        mi.p = point_at(ray, t);
        mi.phaseG = 0.5f;
        mi.sampled = true;
        density = density * sigma_t;
        result = result * sigma_s;
    }
    float pdf = dot(f3(1.0f), density);
    if (0.0f >= pdf) pdf = 1.0f; else pdf = pdf / nSamples;
    return result / pdf;
}
// GridDensityMedium::D / Density / Sample, Medium.hh:111-199
TRC_DEV float grid_D(const trc_GridDensityInfo& info, const float* density, int x, int y, int z) {
    const int nx = (int)info.nx, ny = (int)info.ny, nz = (int)info.nz;
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return 0;
    return density[((size_t)z * ny + y) * nx + x];
}
TRC_DEV float lerp_f(float t, float s1, float s2) { return (1 - t) * s1 + t * s2; }          // Sampling.hh:13-16
TRC_DEV int grid_to_int(float f) { return !(f > -2.0e9f) ? -2000000000 : (f > 2.0e9f ? 2000000000 : (int)f); }
TRC_DEV float grid_density(const trc_GridDensityInfo& info, const float* density, F3 p) {
    const float nx = (float)info.nx, ny = (float)info.ny, nz = (float)info.nz;
    const F3 ps = f3(p.x * nx - 0.5f, p.y * ny - 0.5f, p.z * nz - 0.5f);
    const int ix = grid_to_int(floorf(ps.x)), iy = grid_to_int(floorf(ps.y)), iz = grid_to_int(floorf(ps.z));
    const F3 d = f3(ps.x - (float)ix, ps.y - (float)iy, ps.z - (float)iz);
    // the 8 corners: GridDensityMedium::D returns 0 outside the grid (Medium.hh:111-127), six compares per corner; a lookup
    // whose cell and its +1 neighbours all lie inside -- every lookup but those in the outermost layer -- needs one range test
    float c000, c100, c010, c110, c001, c101, c011, c111;
    const int gx = (int)info.nx, gy = (int)info.ny, gz = (int)info.nz;
    if (ix >= 0 && iy >= 0 && iz >= 0 && ix + 1 < gx && iy + 1 < gy && iz + 1 < gz) {
        const float* b = density + ((size_t)iz * gy + iy) * gx + ix;
        const size_t row = (size_t)gx, slab = (size_t)gx * gy;
        c000 = b[0]; c100 = b[1]; c010 = b[row]; c110 = b[row + 1];
        c001 = b[slab]; c101 = b[slab + 1]; c011 = b[slab + row]; c111 = b[slab + row + 1];
    } else {
        c000 = grid_D(info, density, ix, iy, iz); c100 = grid_D(info, density, ix + 1, iy, iz);
        c010 = grid_D(info, density, ix, iy + 1, iz); c110 = grid_D(info, density, ix + 1, iy + 1, iz);
        c001 = grid_D(info, density, ix, iy, iz + 1); c101 = grid_D(info, density, ix + 1, iy, iz + 1);
        c011 = grid_D(info, density, ix, iy + 1, iz + 1); c111 = grid_D(info, density, ix + 1, iy + 1, iz + 1);
    }
    float d00 = lerp_f(d.x, c000, c100);
    float d10 = lerp_f(d.x, c010, c110);
    float d01 = lerp_f(d.x, c001, c101);
    float d11 = lerp_f(d.x, c011, c111);
    float d0 = lerp_f(d.y, d00, d10);
    float d1 = lerp_f(d.y, d01, d11);
    return lerp_f(d.z, d0, d1);
}
constexpr int kGridSampleMaxSteps = 1 << 16;      // same bound as oracle/oracle.cpp (the reference loop is unbounded)
// The tracker in SLICES of at most `budget` steps (budget < 0: to the end): t and the step count live in the path state, a slice that
// runs out returns kTrackMore and the lane comes back for the next one WITHOUT a Scene::hit in between (trc_render_kernels.hpp) --
// the lanes that are not in the cloud go on with their paths instead of waiting for ~100 steps of somebody else's.  The lane's own
// sequence of operations (and its RNG stream) is the unsliced loop's.
constexpr float kTrackMore = -1.0f;
TRC_DEV float grid_sample(const PathCtx& cx, const HitRec& rec, MediumHit& mi, Pcg& rng, float& t, int& step, int budget) {
    if (!cx.density) return 1.0f;
    const trc_GridDensityInfo& info = cx.dinfo;
    const float tMax = rec.vol_t;
    for (; step < kGridSampleMaxSteps; ++step) {
        if (budget == 0) return kTrackMore;
        --budget;
        t -= dm_logf(1 - pcg_float(rng)) * info.invMaxDensity / info.sigma_t;
        if (t >= tMax) break;
        const F3 p = rec.vol_o + rec.vol_d * t;
        // empty-space shortcut: a lookup whose 2x2x2 footprint lies in an all-zero brick interpolates zeros to +0 (a
        // majorant-only "null collision"), so the 8 gathers and 7 lerps are skipped; the random number is still drawn.
        // (Round 6 also skipped the LOOKUP for the steps a ray certainly stays inside an empty brick -- exit distance worked out
        // once per brick: profiles/r06/exp_empty_runs.patch.  Same bits, +1.6 .. +4.8 %: the brick byte is an L1 hit, the extra
        // divergent branch and the exit arithmetic are not free.  Removed.)
        float dens = 0.0f;
        {
            const int ix = grid_to_int(floorf(p.x * (float)info.nx - 0.5f)), iy = grid_to_int(floorf(p.y * (float)info.ny - 0.5f)),
                      iz = grid_to_int(floorf(p.z * (float)info.nz - 0.5f));
            bool occupied = true;
            if (cx.occupancy) {
                const int bx = (ix + 1) >> 2, by = (iy + 1) >> 2, bz = (iz + 1) >> 2;
                const int nbx = ((int)info.nx + 4) >> 2, nby = ((int)info.ny + 4) >> 2, nbz = ((int)info.nz + 4) >> 2;
                occupied = (ix >= -1 && iy >= -1 && iz >= -1 && bx < nbx && by < nby && bz < nbz) ? cx.occupancy[((size_t)bz * nby + by) * nbx + bx] != 0 : false;
            }
            if (occupied) dens = grid_density(info, cx.density, p);
        }
        if (dens * info.invMaxDensity > pcg_float(rng)) {
            F3 world = p;
            if (rec.vol_cube != kTagNone) {                        // hitRecord.modelMatrix * float4(p, 1)
                const uint32_t* cb = cx.S.small_base + cx.S.off_cubes + rec.vol_cube * kCubeDwords;
                const float4 m0 = ld4(cb + 12), m1 = ld4(cb + 16), m2 = ld4(cb + 20);
                const F3 mc0 = f3(m0.x, m0.y, m0.z), mc1 = f3(m0.w, m1.x, m1.y), mc2 = f3(m1.z, m1.w, m2.x), mc3 = f3(m2.y, m2.z, m2.w);
                world = ((mc0 * p.x + mc1 * p.y) + mc2 * p.z) + mc3;
            }
            mi.p = world;
            mi.phaseG = info.g;
            mi.sampled = true;
            return info.sigma_s / info.sigma_t;
        }
    }
    return 1.0f;
}

// Same for traceMIS (Render.metal:298-406) and, with VOLUME, traceVolume (Render.metal:78-275 = traceMIS + the
// medium block :114-158).  Lights are literally squareList[5] and [6] (:320-324, B-12).
// The shadow ray (any-hit Scene::hit) is traced here, inside the step.
// The light sample of a traceMIS vertex with a light besides the squares (mis_step<.., LIGHT>; L = its tables, p = light_p(L)): the light
// pick, then that light's or a square's sample, its shadow ray and its MIS-weighted contribution; leaves the shading frame, -wo and the
// hit's colour for the BSDF sample.  The pick's one draw takes the light below p, else square 5 below p + (1 - p) / 2 and square 6 above;
// a square's sample is the reference's (:320-356) with its contribution divided by 1 - p.
// Light::Env: the map's sample draws six more numbers; its shadow ray is an any-hit walk to infinity from where a BSDF ray of the same
// direction would start (_origin: only directions above the surface are taken).
// Light::Mesh: the mesh's sample (dev_meshlight.hpp) draws four more numbers; its shadow ray is the any-hit walk to the sample's distance,
// as a square's.  Radiance keeps the reference's Le * cos convention.
template <Light LIGHT, bool ALL_LDS, bool STATS, bool HYB, bool TEX, class COUNT, bool PARAMS = false>
TRC_DEV void light_nee(const PathCtx& cx, PathState& ps, Pcg& rng, TravCounters& cnt, COUNT& n_rays, COUNT& n_shaded, const F2 uu,
                       const F3 _origin, const int mtype, F3& nx, F3& ny, F3& minus_d, F3& base_color) {
    const HitRec& rec = ps.rec;
    const LightTables<LIGHT>& L = *ctx_light<TEX, LIGHT>(cx);
    const float pick = pcg_float(rng);
    // 0: no light sample; 1: a square; 2: the light -- drawn only when it is picked, and only where the BSDF sample is a cosine lobe: a
    // Lambert vertex, or the Lambert lobe a Plastic vertex picks with uu.x < 1/2 (the same uu picks the same lobe in material_F and
    // material_S_F; that lobe's F and pdf are the value and density it samples with).  The other lobes (Beckmann, Metal, Glass) report
    // per-lobe pdfs with the reference's lobe-pick conventions, not the density the light's strategy would have to be weighed against:
    // there a pick of the light takes no sample and the BSDF ray that reaches it keeps weight 1.  The map besides only where the BSDF
    // ray's escape would count (mis_step's depth cutoff).
    ps.env_mis = mtype == kMatLambert || (mtype == kMatPlastic && uu.x < 0.5f);
    int kind;
    if constexpr (LIGHT == Light::Env) kind = pick < light_p(L) ? (ps.depth_left > 1 && ps.env_mis ? 2 : 0) : (L.squares ? 1 : 0);
    else kind = pick < light_p(L) ? (ps.env_mis ? 2 : 0) : (L.squares ? 1 : 0);
    coordinate_system(rec.sn, nx, ny);
    Ray _ray = make_ray(_origin, f3(0.0f, 0.0f, 1.0f));
    float _dis = FLT_MAX;
    F3 light_term = f3(0.0f);
    float liPDF = 0.0f;
    if (kind == 1) {
        LightSample lsr;
        square_sample(cx.S, pick < light_p(L) + (1.0f - light_p(L)) * 0.5f ? 5 : 6, uu, _origin, lsr);
        const F3 _dir = lsr.p - _origin;
        const F3 _nor = normalize(_dir);
        _dis = length(_dir);
        _ray = make_ray(_origin, _nor);
        const float cosOnLight = fabsf(dot(lsr.n, -_nor));
        light_term = mat_albedo(cx.sh, lsr.material) * cosOnLight;
        liPDF = (_dis * _dis) * lsr.areaPDF / cosOnLight;
    } else if (kind == 2) {
        // only where the BSDF strategy has support -- the cosine lobe samples wi.z > 0 and reports pdf 0 unless wo.z > 0 -- does the
        // light's sample carry weight: below the surface Lambert::F = wi.z / pi is negative, and nothing on the BSDF side covers it
        if constexpr (LIGHT == Light::Env) {
            const uint32_t r0 = pcg_next(rng), r1 = pcg_next(rng), r2 = pcg_next(rng), r3 = pcg_next(rng);
            const float f0 = pcg_float(rng), f1 = pcg_float(rng);
            float pdf;
            const F3 dir = env_light_sample(L, r0, r1, r2, r3, f0, f1, pdf);
            const float wi_z = dot(rec.sn, dir), wo_z = -dot(rec.sn, ps.ray.d);
            liPDF = (wi_z > 0.0f && wo_z > 0.0f) ? light_p(L) * pdf : 0.0f;
            if (liPDF > 0.0f) {
                _ray = make_ray(_origin, dir);               // where the BSDF ray of this direction starts (wi.z > 0)
                light_term = env_radiance(cx.env, cx.ambient, _ray.d);
            }
        } else {
            const uint32_t r0 = pcg_next(rng), r1 = pcg_next(rng);
            const float f0 = pcg_float(rng), f1 = pcg_float(rng);
            MeshSample ms;
            mesh_light_sample(L, cx.S.blob + cx.S.off_tripos, r0, r1, f0, f1, _origin, ms);
            const F3 _dir = offset_ray(ms.p, ms.n) - _origin;
            const F3 _nor = normalize(_dir);
            const float dist = length(_dir);
            const float cosL = fabsf(dot(ms.n, -_nor));
            const float wi_z = dot(rec.sn, _nor), wo_z = -dot(rec.sn, ps.ray.d);
            liPDF = (wi_z > 0.0f && wo_z > 0.0f) ? light_p(L) * ms.pdfA * (dist * dist) / cosL : 0.0f;
            if (!(liPDF > 0.0f && liPDF <= FLT_MAX)) liPDF = 0.0f;          // (a grazing or coincident sample: cosL or dist 0)
            if (liPDF > 0.0f) {
                _dis = dist;
                _ray = make_ray(_origin, _nor);
                // the material of triangle ms.tri, as the hit test reads it (dev_intersect.hpp: TRC_TRIANGLE_MATERIALS)
                const uint32_t material = TRC_TRIANGLE_MATERIALS ? ld1_global(cx.S.blob + cx.S.off_triattr + (size_t)ms.tri * kTriAttrDwords + 15u) : 19u;
                light_term = mat_albedo(cx.sh, material) * cosL;
            }
        }
    }
    bool blocked = true;
    if (kind == 1 || (kind == 2 && liPDF > 0.0f)) {              // (a square's sample walks whatever its pdf, as the reference's does)
        bump(n_rays);
        if (STATS) {
            HitRec shr;
            hit_init(shr);
            blocked = scene_hit<ALL_LDS, STATS, true, false, false, HYB>(cx.S, cx.root_min, cx.root_max, _ray, shr, _dis, cx.stack, cx.lvstack, cnt);
        } else {
            blocked = scene_occluded<ALL_LDS, false, HYB>(cx.S, cx.root_min, cx.root_max, _ray, _dis, cx.stack, cx.S.stack_cap);
        }
    }
    minus_d = -ps.ray.d;
    base_color = hit_color<TEX>(cx.S, cx.sh, rec, ctx_tex<TEX>(cx));
    if (!blocked) {
        const F3 wo = f3(dot(nx, minus_d), dot(ny, minus_d), dot(rec.sn, minus_d));
        const F3 wi = f3(dot(nx, _ray.d), dot(ny, _ray.d), dot(rec.sn, _ray.d));
        float bxPDF = 0;
        bump(n_shaded);
        F3 weight = hit_F<TEX, LIGHT, PARAMS>(cx, mtype, rec.material, base_color, wo, wi, uu, bxPDF) * light_term;
        if (kind == 1) ps.color = ps.color + ps.ratio * (weight * power_heuristic(1, liPDF, 1, bxPDF)) / (liPDF * (1.0f - light_p(L)));
        else ps.color = ps.color + ps.ratio * (weight * env_mis_weight(liPDF, bxPDF)) / liPDF;
    }
}

// LIGHT = Light::Env (TRC_FLAG_ENV_LIGHT, traceMIS only): the environment map is a light too (dev_envlight.hpp; light_nee).  A square's
// contribution is divided by 1 - p_env (the reference's expectation, its missing 1/2 included); the map is sampled only at a vertex whose
// BSDF ray would be counted if it escaped, and an escaping BSDF ray is weighted against it.
// With p_env = 0 (a black map) every operation and draw is the flag-off kernel's.
// LIGHT = Light::Mesh (TRC_FLAG_MESH_LIGHTS, traceMIS only): the mesh's emissive triangles are lights too (light_nee).  A BSDF-sampled hit
// on a TRIANGLE emitter is then ps.color + ps.ratio * (albedo * cosOnLight) * w, cosOnLight = |dot(geometric normal, -d)| and
// w = env_mis_weight(scat_bxPDF, p_mesh * pdfA[triangle] * dist^2 / cosOnLight) where the previous vertex took its BSDF sample from a
// cosine lobe, else 1: the estimator of the integrand the mesh's light sample estimates -- without the reference's second
// scat_attenuation / scat_bxPDF factor, and without rec.PDF, which only a square writes (tracer_abi.h).  A square emitter hit keeps the
// reference's formula.  Without a light triangle (p_mesh = 0, no tables) every operation and draw is the flag-off kernel's.
template <bool ALL_LDS, bool STATS, bool VOLUME = false, bool SOBOL = false, bool HYB = false, bool TEX = false, Light LIGHT = Light::None, class COUNT = uint32_t,
          bool PARAMS = false>
TRC_DEV bool mis_step(const PathCtx& cx, PathState& ps, bool hitted, Pcg& rng, TravCounters& cnt, COUNT& n_rays,
                      COUNT& n_shaded, F3& result) {
    HitRec& rec = ps.rec;
    const bool resume = VOLUME && TRC_TRACK_SLICE > 0 && ps.tracking;      // back for the next slice of the delta tracker: nothing below was left undone
    if (!resume) {
    if (!ps.primary) {
        if ((!VOLUME || ps.from_bsdf) && hitted && mat_type(cx.sh, rec.material) == kMatDiffuse) {   // MIS-weighted emitter hit, :390-404
            F3 Li = mat_albedo(cx.sh, rec.material);
            if constexpr (LIGHT == Light::Mesh) {
                const MeshLight& L = *ctx_light<TEX, LIGHT>(cx);
                if (L.n_lights != 0u && (rec.tag >> kTagIndexBits) == kTagTriangle) {      // a triangle emitter, and a mesh strategy exists
                    const uint32_t t = rec.tag & kTagIndexMask;
                    F3 v0, v1, v2;
                    mesh_tri_load(cx.S.blob + cx.S.off_tripos, t, v0, v1, v2);
                    const float cosL = fabsf(dot(mesh_tri_normal(v0, v1, v2), -ps.ray.d));
                    const F3 d = rec.p - ps.ray.o;
                    float w = 1.0f;
                    if (ps.env_mis) {
                        const float lightPDF = L.p_mesh * L.pdfA[t] * dot(d, d) / cosL;
                        if (lightPDF > 0.0f && lightPDF <= FLT_MAX) w = env_mis_weight(ps.scat_bxPDF, lightPDF);
                    }
                    result = ps.color + ps.ratio * (Li * cosL) * w;
                    return true;
                }
            }
            float cosOnLight = dot(-ps.ray.d, rec.sn);
            F3 weight = ps.scat_attenuation * Li * cosOnLight;
            F3 d = rec.p - ps.ray.o;
            float dist2 = dot(d, d);
            float lightPDF = rec.PDF * dist2 / cosOnLight;
            bool shared = true;                                  // (without square lights no light strategy shares the hit: weight 1)
            if constexpr (LIGHT == Light::Env) shared = ctx_light<TEX, LIGHT>(cx)->squares;
            if (shared) weight = weight * power_heuristic(1, ps.scat_bxPDF, 1, lightPDF);
            result = ps.color + ps.ratio * weight / ps.scat_bxPDF;
            return true;
        }
        if (--ps.depth_left <= 0) { result = ps.color; return true; }   // } while ((--depth) > 0), :406
    }
    if constexpr (LIGHT == Light::Env) {
        if (!hitted) {                                               // a BSDF-sampled ray that escapes, against the map's own strategy
            const EnvLight& L = *ctx_light<TEX, LIGHT>(cx);
            F3 le = env_radiance(cx.env, cx.ambient, ps.ray.d);
            if (!ps.primary && ps.env_mis) {
                const float pe = L.p_env * env_light_pdf(L, ps.ray.d);
                if (pe > 0.0f) le = le * env_mis_weight(ps.scat_bxPDF, pe);
            }
            ps.primary = false;
            result = ps.color + ps.ratio * le;
            return true;
        }
    }
    ps.primary = false;
    if (!hitted) { result = ps.color + ps.ratio * env_radiance(cx.env, cx.ambient, ps.ray.d); return true; }
    }
    const int mtype = mat_type(cx.sh, rec.material);
    if (!resume && mtype == kMatDiffuse) {
        F3 le = mat_albedo(cx.sh, rec.material);
        float w = dot(-ps.ray.d, -rec.gn);
        result = ps.ratio * le * fabsf(w);
        return true;
    }
    if (VOLUME) {                                                    // Render.metal:114-158
        MediumHit mi;
        mi.p = f3(0); mi.phaseG = 0; mi.sampled = false;
        if (!resume && ps.medium == TRC_MEDIUM_HOMOGENEOUS) ps.ratio = ps.ratio * homogeneous_sample(ps.ray, rec, mi, rng);
        else if (ps.medium == TRC_MEDIUM_GRIDDENSITY) {
            if (!resume) { ps.trk_t = 0.0f; ps.trk_step = 0; }
            const float beam = grid_sample(cx, rec, mi, rng, ps.trk_t, ps.trk_step, TRC_TRACK_SLICE > 0 ? TRC_TRACK_SLICE : -1);
            if (TRC_TRACK_SLICE > 0) {
                ps.tracking = beam == kTrackMore;
                if (ps.tracking) return false;
            }
            ps.ratio = ps.ratio * f3(beam);
        }
        if (mi.sampled) {                                            // scatter inside the medium
            F2 u2; u2.x = pcg_float(rng); u2.y = pcg_float(rng);
            F3 wi;
            hg_sample_p(mi.phaseG, -ps.ray.d, wi, u2);
            ps.ray = make_ray(mi.p, wi);
            ps.medium = mat_medium(cx.sh, rec.material);
            ps.from_bsdf = false;
            return false;                                            // need_test, then `continue`
        }
        if (mtype == kMatNil) {                                      // medium boundary without a surface
            if (dot(ps.ray.d, rec.gn) < 0) {
                ps.ray = make_ray(offset_ray(rec.p, -rec.gn), ps.ray.d);
                ps.medium = mat_medium(cx.sh, rec.material);
            } else {
                ps.ray = make_ray(offset_ray(rec.p, rec.gn), ps.ray.d);
                ps.medium = TRC_MEDIUM_NIL;
            }
            ps.from_bsdf = false;
            return false;
        }
        ps.from_bsdf = true;
    }
    LightSample lsr;
    const F2 uu = sample_2d<SOBOL>(cx, ps, rng);                     // :314
    const F3 hit_origin = rec.p;
    F3 _origin = offset_ray(rec.p, rec.sn);
    F3 nx, ny, minus_d, base_color;
    if constexpr (LIGHT != Light::None) {
        light_nee<LIGHT, ALL_LDS, STATS, HYB, TEX, COUNT, PARAMS>(cx, ps, rng, cnt, n_rays, n_shaded, uu, _origin, mtype, nx, ny, minus_d, base_color);
    } else {
    if (pcg_float(rng) < 0.5f) square_sample(cx.S, 5, uu, _origin, lsr);
    else square_sample(cx.S, 6, uu, _origin, lsr);
    F3 _dir = lsr.p - _origin;
    F3 _nor = normalize(_dir);
    coordinate_system(rec.sn, nx, ny);
    const float _tr = 1.0f;
    const float _dis = length(_dir);
    const Ray _ray = make_ray(_origin, _nor);
    // what the light sample contributes if the shadow ray gets through, reduced to four values BEFORE the walk (the same expressions
    // on the same operands, :345-352): the sample itself (point, normal, material, area pdf) does not have to survive the walk
    float cosOnLight = fabsf(dot(lsr.n, -_nor));
    F3 light_term = mat_albedo(cx.sh, lsr.material) * cosOnLight;
    float liPDF = (_dis * _dis) * lsr.areaPDF / cosOnLight;
    TRC_PIN(light_term.x); TRC_PIN(light_term.y); TRC_PIN(light_term.z); TRC_PIN(liPDF);
    bump(n_rays);
    bool blocked;
    if (STATS) {                                  // the reference's walk (the exact counters are defined on it)
        HitRec shr;
        hit_init(shr);
        blocked = scene_hit<ALL_LDS, STATS, true, false, false, HYB>(cx.S, cx.root_min, cx.root_max, _ray, shr, _dis, cx.stack, cx.lvstack, cnt);
    } else {                                                          // any-hit: the answer does not depend on the order (dev_intersect.hpp)
        blocked = scene_occluded<ALL_LDS, false, HYB>(cx.S, cx.root_min, cx.root_max, _ray, _dis, cx.stack, cx.S.stack_cap);
    }
    minus_d = -ps.ray.d;
    base_color = hit_color<TEX>(cx.S, cx.sh, rec, ctx_tex<TEX>(cx));
    if (!blocked) {                                                  // light sampling, :339-356
        F3 wo = f3(dot(nx, minus_d), dot(ny, minus_d), dot(rec.sn, minus_d));
        F3 wi = f3(dot(nx, _ray.d), dot(ny, _ray.d), dot(rec.sn, _ray.d));
        float bxPDF = 0;
        bump(n_shaded);
        F3 weight = hit_F<TEX, LIGHT, PARAMS>(cx, mtype, rec.material, base_color, wo, wi, uu, bxPDF);
        weight = weight * light_term;
        weight = weight * power_heuristic(1, liPDF, 1, bxPDF);
        ps.color = ps.color + _tr * ps.ratio * weight / liPDF;
    }
    }
    // BXDF sampling, :358-378
    F3 wi = f3(0);
    float bxPDF = 0;
    F3 wo = f3(dot(nx, minus_d), dot(ny, minus_d), dot(rec.sn, minus_d));
    bump(n_shaded);
    ps.scat_attenuation = hit_S_F<false, TEX, LIGHT, PARAMS>(cx, mtype, rec.material, base_color, wo, wi, uu, bxPDF, cnt);
    ps.scat_bxPDF = bxPDF;
    if (bxPDF <= 0) { result = ps.color; return true; }
    F3 wiw = (nx * wi.x + ny * wi.y) + rec.sn * wi.z;
    if (wi.z < 0) {
        ps.ray = make_ray(offset_ray(hit_origin, -rec.sn), wiw);
        if (VOLUME) ps.medium = (dot(wiw, rec.gn) < 0) ? mat_medium(cx.sh, rec.material) : (int)TRC_MEDIUM_NIL;   // :236-243
    } else {
        ps.ray = make_ray(_origin, wiw);
    }
    ps.ratio = ps.ratio * (ps.scat_attenuation / ps.scat_bxPDF);
    {
        float p = rgb_to_y(ps.ratio);
        if (pcg_float(rng) > p) { result = ps.color; return true; }
        ps.ratio = ps.ratio * rcp1(p);
    }
    return false;
}

}  // namespace trcdev
