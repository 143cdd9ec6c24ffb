// material_params_ref.cpp -- scalar CPU restatement of Material::S_F and Material::F (RT_Metal/Metal/Material.hh:77-146 over
// MicrofacetBXDF.h, BXDF.hh, BXDF.metal, MatteBXDF.hh, Sampling.hh, Math.hh) with the lobe parameters the reference writes as literals
// handed in per call: the definition TRC_FLAG_MATERIAL_PARAMS is tested against (include/tracer_abi.h: trc_material_params).
// binary32, one rounding per operation in the order written, no contraction (-ffp-contract=off), transcendental functions from
// include/trc_detmath.h.  Written class by class as the reference states them -- not as the kernels organise them by lobe.
// Its authority comes from what exists: at the default parameters it equals the oracle's Material_S_F / Material_F bit for bit, at any
// roughness its distributions equal orc_microfacet, at any index its Fresnel terms equal orc_fr_dielectric_n / orc_fr_conductor_n
// (tests/test_material_params_ref.py).  Built by tests/material_params_ref/material_params_loader.py.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "trc_detmath.h"

namespace {

const float PI_F = 3.14159265358979323846f;

struct V2 { float x, y; };
struct V3 { float x, y, z; };
inline V3 v3(float x, float y, float z) { return V3{x, y, z}; }
inline V3 v3(float s) { return V3{s, s, s}; }
inline V3 v3a(const float* f) { return V3{f[0], f[1], f[2]}; }
inline V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline V3 operator/(V3 a, V3 b) { return v3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
inline V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
inline V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
inline V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float length(V3 a) { return sqrtf(dot(a, a)); }
inline V3 normalize(V3 a) { float inv = 1.0f / length(a); return a * inv; }
inline float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
inline void put3(float* o, V3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// ---------------------------------------------------------------- Math.hh:118-167
float ErfInv(float x) {
    float w, p;
    x = clampf(x, -.99999f, .99999f);
    w = -dm_logf((1 - x) * (1 + x));
    if (w < 5) {
        w = w - 2.5f;
        p = 2.81022636e-08f;
        p = 3.43273939e-07f + p * w;
        p = -3.5233877e-06f + p * w;
        p = -4.39150654e-06f + p * w;
        p = 0.00021858087f + p * w;
        p = -0.00125372503f + p * w;
        p = -0.00417768164f + p * w;
        p = 0.246640727f + p * w;
        p = 1.50140941f + p * w;
    } else {
        w = sqrtf(w) - 3;
        p = -0.000200214257f;
        p = 0.000100950558f + p * w;
        p = 0.00134934322f + p * w;
        p = -0.00367342844f + p * w;
        p = 0.00573950773f + p * w;
        p = -0.0076224613f + p * w;
        p = 0.00943887047f + p * w;
        p = 1.00167406f + p * w;
        p = 2.83297682f + p * w;
    }
    return p * x;
}
float Erf(float x) {
    float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f;
    float p = 0.3275911f;
    int sign = 1;
    if (x < 0) sign = -1;
    x = fabsf(x);
    float t = 1 / (1 + p * x);
    float y = 1 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * dm_expf(-x * x);
    return sign * y;
}

// ---------------------------------------------------------------- Sampling.hh
V2 ConcentricSampleDisk(V2 u) {
    V2 uOffset = V2{2.f * u.x - 1, 2.f * u.y - 1};
    if (uOffset.x == 0 && uOffset.y == 0) return V2{0, 0};
    const float PiOver2 = PI_F / 2.0f, PiOver4 = PI_F / 4.0f;
    float theta, r;
    if (fabsf(uOffset.x) > fabsf(uOffset.y)) {
        r = uOffset.x;
        theta = PiOver4 * (uOffset.y / uOffset.x);
    } else {
        r = uOffset.y;
        theta = PiOver2 - PiOver4 * (uOffset.x / uOffset.y);
    }
    return V2{r * dm_cosf(theta), r * dm_sinf(theta)};
}
V3 CosineSampleHemisphere(V2 u) {
    V2 d = ConcentricSampleDisk(u);
    float z = sqrtf(fmaxf(0.0f, 1.0f - d.x * d.x - d.y * d.y));
    return v3(d.x, d.y, z);
}
float CosTheta(V3 w) { return w.z; }
float Cos2Theta(V3 w) { return w.z * w.z; }
float AbsCosTheta(V3 w) { return fabsf(w.z); }
float Sin2Theta(V3 w) { return fmaxf(0.0f, 1.0f - Cos2Theta(w)); }
float SinTheta(V3 w) { return sqrtf(Sin2Theta(w)); }
float TanTheta(V3 vec) {
    float temp = 1 - vec.z * vec.z;
    if (temp <= 0.0f || vec.z == 0.0f) return 0.0f;
    return sqrtf(temp) / vec.z;
}
float Tan2Theta(V3 vec) {
    float zz = vec.z * vec.z;
    float temp = 1 - zz;
    if (temp <= 0.0f || zz == 0.0f) return 0.0f;
    return temp / zz;
}
float CosPhi(V3 w) { float s = SinTheta(w); return (s == 0) ? 1 : clampf(w.x / s, -1.0f, 1.0f); }
float SinPhi(V3 w) { float s = SinTheta(w); return (s == 0) ? 0 : clampf(w.y / s, -1.0f, 1.0f); }
float Cos2Phi(V3 w) { float r = CosPhi(w); return r * r; }
float Sin2Phi(V3 w) { float r = SinPhi(w); return r * r; }
float Sqr(float v) { return v * v; }
V3 Faceforward(V3 n, V3 v) { return (dot(n, v) < 0.f) ? -n : n; }

// ---------------------------------------------------------------- BXDF.hh / BXDF.metal
V3 Reflect(V3 wo, V3 n) { return -wo + 2 * dot(wo, n) * n; }
bool Refract(V3 wo, V3 n, float eta, V3& wi) {
    float cosThetaI = wo.z;
    float sin2ThetaI = fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI);
    float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return false;
    float cosThetaT = sqrtf(1 - sin2ThetaT);
    wi = eta * -wo + (eta * cosThetaI - cosThetaT) * n;
    return true;
}
float FrDielectric(float cosi, float eta) {
    cosi = clampf(cosi, -1.0f, 1.0f);
    bool entering = cosi > 0.f;
    if (!entering) { eta = 1 / eta; cosi = -cosi; }
    float sin2Theta_i = 1 - cosi * cosi;
    float sin2Theta_t = sin2Theta_i / Sqr(eta);
    if (sin2Theta_t >= 1) return 1.f;
    float cosTheta_t = sqrtf(fmaxf(0.0f, 1 - sin2Theta_t));
    float r_parl = (eta * cosi - cosTheta_t) / (eta * cosi + cosTheta_t);
    float r_perp = (cosi - eta * cosTheta_t) / (cosi + eta * cosTheta_t);
    return (r_parl * r_parl + r_perp * r_perp) / 2;
}
V3 FrConductor(float cosi, V3 eta, V3 k) {
    V3 tmp = (eta * eta + k * k) * cosi * cosi;
    V3 Rparl2 = (tmp - (2.f * eta * cosi) + v3(1)) / (tmp + (2.f * eta * cosi) + v3(1));
    V3 tmp_f = eta * eta + k * k;
    V3 Rperp2 = (tmp_f - (2.f * eta * cosi) + v3(cosi * cosi)) / (tmp_f + (2.f * eta * cosi) + v3(cosi * cosi));
    return 0.5f * (Rparl2 + Rperp2);
}
struct FresnelConductor {
    V3 eta, k;
    V3 Evaluate(float cosThetaI) const { return FrConductor(fabsf(cosThetaI), eta, k); }
};
struct FresnelDielectric {
    float eta;
    V3 Evaluate(float cosThetaI) const { return v3(FrDielectric(cosThetaI, eta)); }
};

// ---------------------------------------------------------------- MatteBXDF.hh:6-22
struct Lambertian {
    float F(V3, V3 wi) const { return wi.z / PI_F; }
    float PDF(V3 wo, V3 wi) const { return wo.z * wi.z > 0 ? fabsf(wi.z) / PI_F : 0; }
    float S_F(V3 wo, V3& wi, V2 uu, float& pdf) const {
        wi = CosineSampleHemisphere(uu);
        pdf = PDF(wo, wi);
        return wi.z / PI_F;
    }
};

// ---------------------------------------------------------------- MicrofacetBXDF.h:137-290
struct Beckmann {
    float alphax, alphay;
    Beckmann(float ax, float ay) : alphax(fmaxf(0.001f, ax)), alphay(fmaxf(0.001f, ay)) {}
    float Lambda(V3 w) const {
        float absTanTheta = fabsf(TanTheta(w));
        if (std::isinf(absTanTheta)) return 0.;
        float alpha = sqrtf(Cos2Phi(w) * alphax * alphax + Sin2Phi(w) * alphay * alphay);
        float a = 1 / (alpha * absTanTheta);
        if (a >= 1.6f) return 0;
        return (1 - 1.259f * a + 0.396f * a * a) / (3.535f * a + 2.181f * a * a);
    }
    float D(V3 wh) const {
        float tan2Theta = Tan2Theta(wh);
        if (std::isinf(tan2Theta)) return 0.;
        float cos4Theta = Cos2Theta(wh) * Cos2Theta(wh);
        return dm_expf(-tan2Theta * (Cos2Phi(wh) / (alphax * alphax) + Sin2Phi(wh) / (alphay * alphay))) /
               (PI_F * alphax * alphay * cos4Theta);
    }
    float G1(V3 w) const { return 1 / (1 + Lambda(w)); }
    float G(V3 wo, V3 wi) const { return 1 / (1 + Lambda(wo) + Lambda(wi)); }
    float PDF(V3 wo, V3 wh) const { return D(wh) * G1(wo) * fabsf(dot(wo, wh)) / AbsCosTheta(wo); }
    static void Sample11(float cosThetaI, float U1, float U2, float* slope_x, float* slope_y) {
        if (cosThetaI > .9999f) {
            float r = sqrtf(-dm_logf(1.0f - U1));
            float sinPhi = dm_sinf(2 * PI_F * U2);
            float cosPhi = dm_cosf(2 * PI_F * U2);
            *slope_x = r * cosPhi;
            *slope_y = r * sinPhi;
            return;
        }
        float sinThetaI = sqrtf(fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI));
        float tanThetaI = sinThetaI / cosThetaI;
        float cotThetaI = 1 / tanThetaI;
        float a = -1, c = Erf(cotThetaI);
        float sample_x = fmaxf(U1, 1e-6f);
        float thetaI = dm_acosf(cosThetaI);
        float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
        float b = c - (1 + c) * dm_powf(1 - sample_x, fit);
        const float SQRT_PI_INV = 1.f / sqrtf(PI_F);
        float normalization = 1 / (1 + c + SQRT_PI_INV * tanThetaI * dm_expf(-cotThetaI * cotThetaI));
        int it = 0;
        while (++it < 10) {
            if (!(b >= a && b <= c)) b = 0.5f * (a + c);
            float invErf = ErfInv(b);
            float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_expf(-invErf * invErf)) - sample_x;
            float derivative = normalization * (1 - invErf * tanThetaI);
            if (fabsf(value) < 1e-5f) break;
            if (value > 0) c = b; else a = b;
            b -= value / derivative;
        }
        *slope_x = ErfInv(b);
        *slope_y = ErfInv(2.0f * fmaxf(U2, 1e-6f) - 1.0f);
    }
    V3 sample_wh(V3 wo, V2 u) const {
        bool flip = wo.z < 0;
        V3 wi = flip ? -wo : wo;
        V3 wiStretched = normalize(v3(alphax * wi.x, alphay * wi.y, wi.z));
        float slope_x, slope_y;
        Sample11(CosTheta(wiStretched), u.x, u.y, &slope_x, &slope_y);
        float tmp = CosPhi(wiStretched) * slope_x - SinPhi(wiStretched) * slope_y;
        slope_y = SinPhi(wiStretched) * slope_x + CosPhi(wiStretched) * slope_y;
        slope_x = tmp;
        slope_x = alphax * slope_x;
        slope_y = alphay * slope_y;
        V3 wh = normalize(v3(-slope_x, -slope_y, 1.f));
        if (flip) wh = -wh;
        return wh;
    }
};

// ---------------------------------------------------------------- MicrofacetBXDF.h:292-434
struct TrowbridgeReitz {
    float alpha_x, alpha_y;
    TrowbridgeReitz(float ax, float ay) : alpha_x(fmaxf(0.001f, ax)), alpha_y(fmaxf(0.001f, ay)) {}
    float D(V3 wh) const {
        float tan2Theta = Tan2Theta(wh);
        if (std::isinf(tan2Theta)) return 0.;
        const float cos4Theta = Cos2Theta(wh) * Cos2Theta(wh);
        if (cos4Theta < 1e-16f) return 0;
        float e = (Cos2Phi(wh) / Sqr(alpha_x) + Sin2Phi(wh) / Sqr(alpha_y)) * tan2Theta;
        return 1 / (PI_F * alpha_x * alpha_y * Sqr(1 + e) * cos4Theta);
    }
    float Lambda(V3 w) const {
        float tan2Theta = Tan2Theta(w);
        if (std::isinf(tan2Theta)) return 0.;
        float alpha2 = Sqr(CosPhi(w) * alpha_x) + Sqr(SinPhi(w) * alpha_y);
        return 0.5f * (sqrtf(1 + alpha2 * tan2Theta) - 1);
    }
    float G1(V3 w) const { return 1 / (1 + Lambda(w)); }
    float G(V3 wo, V3 wi) const { return 1 / (1 + Lambda(wo) + Lambda(wi)); }
    float PDF(V3 wo, V3 wh) const { return D(wh) * G1(wo) * fabsf(dot(wo, wh) / CosTheta(wo)); }
    static void Sample11(float cosTheta, float U1, float U2, float* slope_x, float* slope_y) {
        if (cosTheta > .9999f) {
            float r = sqrtf(U1 / (1 - U1));
            float phi = 6.28318530718f * U2;
            *slope_x = r * dm_cosf(phi);
            *slope_y = r * dm_sinf(phi);
            return;
        }
        float sinTheta = sqrtf(fmaxf(0.0f, 1.0f - cosTheta * cosTheta));
        float tanTheta = sinTheta / cosTheta;
        float a = 1 / tanTheta;
        float G1 = 2 / (1 + sqrtf(1.f + 1.f / (a * a)));
        float A = 2 * U1 / G1 - 1;
        float tmp = 1.f / (A * A - 1.f);
        if (tmp > 1e10f) tmp = 1e10f;
        float B = tanTheta;
        float D = sqrtf(fmaxf(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
        float slope_x_1 = B * tmp - D;
        float slope_x_2 = B * tmp + D;
        *slope_x = (A < 0 || slope_x_2 > 1.f / tanTheta) ? slope_x_1 : slope_x_2;
        float S;
        if (U2 > 0.5f) { S = 1.f; U2 = 2.f * (U2 - .5f); }
        else { S = -1.f; U2 = 2.f * (.5f - U2); }
        float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
                  (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
        *slope_y = S * z * sqrtf(1.f + *slope_x * *slope_x);
    }
    V3 sample_wh(V3 wo, V2 u) const {
        bool flip = wo.z < 0;
        V3 wi = flip ? -wo : wo;
        V3 wiStretched = normalize(v3(alpha_x * wi.x, alpha_y * wi.y, wi.z));
        float slope_x, slope_y;
        Sample11(CosTheta(wiStretched), u.x, u.y, &slope_x, &slope_y);
        float tmp = CosPhi(wiStretched) * slope_x - SinPhi(wiStretched) * slope_y;
        slope_y = SinPhi(wiStretched) * slope_x + CosPhi(wiStretched) * slope_y;
        slope_x = tmp;
        slope_x = alpha_x * slope_x;
        slope_y = alpha_y * slope_y;
        V3 wh = normalize(v3(-slope_x, -slope_y, 1.f));
        if (flip) wh = -wh;
        return wh;
    }
};

// ---------------------------------------------------------------- MicrofacetBXDF.h:7-62
template <typename DistType, typename FrType>
struct MicrofacetReflection {
    V3 R; FrType fresnel; DistType distribution;
    V3 F(V3 wo, V3 wi) const {
        float cosThetaO = AbsCosTheta(wo), cosThetaI = AbsCosTheta(wi);
        if (cosThetaI == 0 || cosThetaO == 0) return v3(0);
        V3 wh = wi + wo;
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return v3(0);
        wh = normalize(wh);
        V3 Fr = fresnel.Evaluate(dot(wi, Faceforward(wh, v3(0, 0, 1))));
        return R * distribution.D(wh) * distribution.G(wo, wi) * Fr / (4 * cosThetaI * cosThetaO);
    }
    float PDF(V3 wo, V3 wi) const {
        if (wo.z * wi.z <= 0) return 0;
        V3 wh = normalize(wo + wi);
        return distribution.PDF(wo, wh) / (4 * dot(wo, wh));
    }
    V3 S_F(V3 wo, V3& wi, V2 uu, float& pdf) const {
        if (wo.z == 0) return v3(0);
        V3 wh = distribution.sample_wh(wo, uu);
        if (dot(wo, wh) <= 0) return v3(0);
        wi = Reflect(wo, wh);
        if (wo.z * wi.z <= 0) return v3(0);
        pdf = distribution.PDF(wo, wh) / (4 * dot(wo, wh));
        return F(wo, wi);
    }
};
// MicrofacetBXDF.h:64-135, mode = Importance (factor 1); its own Fresnel term is FresnelDielectric(etaA), :81
template <typename DistType>
struct MicrofacetTransmission {
    V3 T; DistType dist; float etaA, etaB; FresnelDielectric fresnel;
    MicrofacetTransmission(V3 T, DistType d, float etaA, float etaB) : T(T), dist(d), etaA(etaA), etaB(etaB), fresnel{etaA} {}
    V3 F(V3 wo, V3 wi) const {
        if (wo.z * wi.z > 0) return v3(0);
        float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
        if (cosThetaI == 0 || cosThetaO == 0) return v3(0);
        float eta = CosTheta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
        V3 wh = normalize(wo + wi * eta);
        if (wh.z < 0) wh = -wh;
        if (dot(wo, wh) * dot(wi, wh) > 0) return v3(0);
        V3 Fr = fresnel.Evaluate(dot(wo, wh));
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float factor = 1;
        return (v3(1.0f) - Fr) * T *
               fabsf(dist.D(wh) * dist.G(wo, wi) * eta * eta * fabsf(dot(wi, wh)) * fabsf(dot(wo, wh)) * factor * factor /
                     (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
    }
    float PDF(V3 wo, V3 wi) const {
        if (wo.z * wi.z > 0) return 0;
        float eta = CosTheta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
        V3 wh = normalize(wo + wi * eta);
        if (dot(wo, wh) * dot(wi, wh) > 0) return 0;
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrtDenom * sqrtDenom));
        return dist.PDF(wo, wh) * dwh_dwi;
    }
    V3 S_F(V3 wo, V3& wi, V2 uu, float& pdf) const {
        if (wo.z == 0) return v3(0);
        V3 wh = dist.sample_wh(wo, uu);
        if (dot(wo, wh) < 0) return v3(0);
        float eta = CosTheta(wo) > 0 ? (etaA / etaB) : (etaB / etaA);
        if (!Refract(wo, wh, eta, wi)) return v3(0);
        pdf = PDF(wo, wi);
        return F(wo, wi);
    }
};

// ---------------------------------------------------------------- the materials, MicrofacetBXDF.h:436-586, with their literals handed in
struct Params { float alpha_x, alpha_y, eta, pad0; float metal_eta[3], pad1; float metal_k[3], pad2; };      // trc_material_params
typedef MicrofacetReflection<TrowbridgeReitz, FresnelConductor> MetalMaterial;
MetalMaterial createMetalMaterial(const Params& p) {
    return MetalMaterial{v3(1.0f), FresnelConductor{v3a(p.metal_eta), v3a(p.metal_k)}, TrowbridgeReitz(p.alpha_x, p.alpha_y)};
}
typedef MicrofacetReflection<Beckmann, FresnelDielectric> PlasticX;
struct PlasticMaterial {
    V3 ks = v3(0.2f);
    V3 kd = v3(0.35f, 0.12f, 0.48f);
    Lambertian matte;
    PlasticX micro;
    explicit PlasticMaterial(const PlasticX& m) : micro(m) {}
    V3 F(V3 wo, V3 wi, V2 uu) const {
        if (uu.x < 0.5f) return kd * matte.F(wo, wi);
        return ks * micro.F(wo, wi);
    }
    float PDF(V3 wo, V3 wi, V2 uu) const {
        if (uu.x < 0.5f) return matte.PDF(wo, wi);
        return micro.PDF(wo, wi);
    }
    V3 S_F(V3 wo, V3& wi, V2 uu, float& pdf) const {
        V2 _uu_ = uu;
        if (_uu_.x < 0.5f) { _uu_.x *= 2; return kd * matte.S_F(wo, wi, _uu_, pdf); }
        _uu_.x -= 0.5f; _uu_.x *= 2.0f;
        return ks * micro.S_F(wo, wi, _uu_, pdf);
    }
};
PlasticMaterial createPlasticMaterial(const Params& p) {
    return PlasticMaterial(PlasticX{v3(1.0f), FresnelDielectric{p.eta}, Beckmann(p.alpha_x, p.alpha_y)});
}
struct GlassMaterial {
    MicrofacetReflection<Beckmann, FresnelDielectric> _mr;
    MicrofacetTransmission<Beckmann> _mt;
    float ratio = 0.25f;
    GlassMaterial(const FresnelDielectric& fr, const Beckmann& dist) : _mr{v3(0.98f), fr, dist}, _mt(v3(0.98f), dist, 1.0f, fr.eta) {}
    V3 F(V3 wo, V3 wi, V2 uu) const {
        if (uu.x < ratio) return _mr.F(wo, wi);
        return _mt.F(wo, wi);
    }
    float PDF(V3 wo, V3 wi, V2 uu) const {
        if (uu.x < ratio) return ratio * _mr.PDF(wo, wi);
        return (1 - ratio) * _mt.PDF(wo, wi);
    }
    V3 S_F(V3 wo, V3& wi, V2 uu, float& pdf) const {
        if (uu.x < ratio) { V2 _uu = uu; _uu.x = uu.x / ratio; return _mr.S_F(wo, wi, _uu, pdf); }
        V2 _uu = uu; _uu.x = (uu.x - ratio) / (1.0f - ratio); return _mt.S_F(wo, wi, _uu, pdf);
    }
};
GlassMaterial createGlass(const Params& p) { return GlassMaterial(FresnelDielectric{p.eta}, Beckmann(p.alpha_x, p.alpha_y)); }

enum { kLambert = 1, kPlastic = 3, kMetal = 4, kGlass = 5 };      // Material.hh:18-20 by ordinal

}  // namespace

extern "C" {

// Material::S_F, Material.hh:124-146: out7 = wi, color * bx.S_F, pdf; wi starts at 0 and pdf at pdf_init, and an early-out leaves them
void mp_ref_s_f(const uint32_t* type, const float* color3, const float* params12, const float* wo3, const float* uu2, size_t n, float pdf_init,
                float* out7) {
    for (size_t i = 0; i < n; ++i) {
        const Params& p = *reinterpret_cast<const Params*>(params12 + 12 * i);
        const V3 color = v3a(color3 + 3 * i), wo = v3a(wo3 + 3 * i);
        const V2 uu{uu2[2 * i], uu2[2 * i + 1]};
        V3 wi = v3(0), f = v3(0);
        float pdf = pdf_init;
        switch (type[i]) {
            case kLambert: f = color * v3(Lambertian{}.S_F(wo, wi, uu, pdf)); break;
            case kMetal: f = color * createMetalMaterial(p).S_F(wo, wi, uu, pdf); break;
            case kPlastic: f = color * createPlasticMaterial(p).S_F(wo, wi, uu, pdf); break;
            case kGlass: f = color * createGlass(p).S_F(wo, wi, uu, pdf); break;
            default: break;
        }
        put3(out7 + 7 * i, wi); put3(out7 + 7 * i + 3, f);
        out7[7 * i + 6] = pdf;
    }
}
// Material::F, Material.hh:77-99: out4 = color * bx.F, bx.PDF (0 for a type without a lobe)
void mp_ref_f(const uint32_t* type, const float* color3, const float* params12, const float* wo3, const float* wi3, const float* uu2, size_t n,
              float* out4) {
    for (size_t i = 0; i < n; ++i) {
        const Params& p = *reinterpret_cast<const Params*>(params12 + 12 * i);
        const V3 color = v3a(color3 + 3 * i), wo = v3a(wo3 + 3 * i), wi = v3a(wi3 + 3 * i);
        const V2 uu{uu2[2 * i], uu2[2 * i + 1]};
        V3 f = v3(0);
        float pdf = 0;
        switch (type[i]) {
            case kLambert: pdf = Lambertian{}.PDF(wo, wi); f = color * v3(Lambertian{}.F(wo, wi)); break;
            case kMetal: { const MetalMaterial m = createMetalMaterial(p); pdf = m.PDF(wo, wi); f = color * m.F(wo, wi); break; }
            case kPlastic: { const PlasticMaterial m = createPlasticMaterial(p); pdf = m.PDF(wo, wi, uu); f = color * m.F(wo, wi, uu); break; }
            case kGlass: { const GlassMaterial m = createGlass(p); pdf = m.PDF(wo, wi, uu); f = color * m.F(wo, wi, uu); break; }
            default: break;
        }
        put3(out4 + 4 * i, f);
        out4[4 * i + 3] = pdf;
    }
}
// the distributions alone, in orc_microfacet's layout: D(wh), G(wo, wh), G1(wo), PDF(wo, wh), sample_wh(wo, uu), Lambda(wo) (0 for Beckmann)
void mp_ref_microfacet(int dist, float ax, float ay, const float* wo3, const float* wh3, const float* uu2, size_t n, float* out8) {
    const Beckmann bk(ax, ay);
    const TrowbridgeReitz tr(ax, ay);
    for (size_t i = 0; i < n; ++i) {
        const V3 wo = v3a(wo3 + 3 * i), wh = v3a(wh3 + 3 * i);
        const V2 uu{uu2[2 * i], uu2[2 * i + 1]};
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
void mp_ref_fr_dielectric(const float* cosi, const float* eta, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = FrDielectric(cosi[i], eta[i]);
}
void mp_ref_fr_conductor(const float* cosi, const float* eta3, const float* k3, size_t n, float* out3) {
    for (size_t i = 0; i < n; ++i) put3(out3 + 3 * i, FrConductor(cosi[i], v3a(eta3 + 3 * i), v3a(k3 + 3 * i)));
}

}  // extern "C"
