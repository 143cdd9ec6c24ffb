// dev_bsdf.hpp -- BSDF evaluation / sampling on the device, in the local shading frame (z = normal).
//
// Reference (RT_Metal/Metal/): Sampling.hh:18-203, BXDF.hh:24-81, BXDF.metal:3-34,
// MatteBXDF.hh:6-22, MicrofacetBXDF.h:7-586, Texture.hh:17-43, Material.hh:77-146.
// The reference hard-codes every lobe parameter in its create*() functions
// (MicrofacetBXDF.h:438-455,514-530,576-586); they are compile-time constants here, so the
// material switch carries no per-material parameter loads beyond type + albedo.  (TRC_FLAG_MATERIAL_PARAMS: the same lobes with those
// parameters read from a table, at the end of this file; the kernels of trc_render_params.hpp alone use them.)
#pragma once

#include "dev_prof.hpp"
#include "dev_vec.hpp"

namespace trcdev {

// ---------------------------------------------------------------- Sampling.hh
TRC_DEV void coordinate_system(const F3 a, F3& b, F3& c) {          // Sampling.hh:18-34
    if (fabsf(a.x) > fabsf(a.y)) b = f3(-a.z, 0, a.x);
    else b = f3(0, a.z, -a.y);
    b = normalize(b);
    c = cross(a, b);
}
TRC_DEV F2 concentric_sample_disk(const F2 u) {                      // Sampling.hh:79-99
    F2 uo; uo.x = 2.f * u.x - 1; uo.y = 2.f * u.y - 1;
    F2 r0; r0.x = 0; r0.y = 0;
    if (uo.x == 0 && uo.y == 0) return r0;
    const float PiOver2 = kPi / 2.0f, PiOver4 = kPi / 4.0f;
    // one quotient for both cases (half the lanes of a wavefront take each: as two branches they ran one after the other)
    const bool wide = fabsf(uo.x) > fabsf(uo.y);
    const float r = wide ? uo.x : uo.y;
    const float q = (wide ? uo.y : uo.x) / r;
    const float theta = wide ? PiOver4 * q : PiOver2 - PiOver4 * q;
    float s, c;
    dm_sincosf(theta, &s, &c);
    F2 out; out.x = r * c; out.y = r * s;
    return out;
}
TRC_DEV F3 cosine_sample_hemisphere(const F2 u) {                    // Sampling.hh:125-129
    F2 d = concentric_sample_disk(u);
    float z = sqrt_cr(fmaxf(0.0f, 1.0f - d.x * d.x - d.y * d.y));
    return f3(d.x, d.y, z);
}
TRC_DEV float power_heuristic(int nf, float fPdf, int ng, float gPdf) {   // Sampling.hh:137-140
    float f = nf * fPdf, g = ng * gPdf;
    return (f * f) / (f * f + g * g);
}
// Sampling.hh:148-203
TRC_DEV float cos_theta(F3 w) { return w.z; }
TRC_DEV float cos2_theta(F3 w) { return w.z * w.z; }
TRC_DEV float abs_cos_theta(F3 w) { return fabsf(w.z); }
TRC_DEV float sin2_theta(F3 w) { return fmaxf(0.0f, 1.0f - cos2_theta(w)); }
TRC_DEV float sin_theta(F3 w) { return sqrt_cr(sin2_theta(w)); }
TRC_DEV float tan_theta(F3 v) {
    float temp = 1 - v.z * v.z;
    if (temp <= 0.0f || v.z == 0.0f) return 0.0f;
    return sqrt_cr(temp) / v.z;
}
TRC_DEV float tan2_theta(F3 v) {
    float zz = v.z * v.z;
    float temp = 1 - zz;
    if (temp <= 0.0f || zz == 0.0f) return 0.0f;
    return temp / zz;
}
TRC_DEV float cos_phi(F3 w) { float s = sin_theta(w); return (s == 0) ? 1 : clampf(w.x / s, -1.0f, 1.0f); }
TRC_DEV float sin_phi(F3 w) { float s = sin_theta(w); return (s == 0) ? 0 : clampf(w.y / s, -1.0f, 1.0f); }
TRC_DEV float cos2_phi(F3 w) { float r = cos_phi(w); return r * r; }
TRC_DEV float sin2_phi(F3 w) { float r = sin_phi(w); return r * r; }
TRC_DEV float sqr(float v) { return v * v; }
// cos_phi and sin_phi of one direction: two quotients by the same sin_theta.  TRC_PHI_PAIR: reciprocal + Newton step once,
// the quotients' own corrections, operand guards as one wave-uniform range test (dev_vec.hpp: GuardedDivBy / div_core) --
// the same bits as the two divisions (tests/test_gpu_divby.py), which is what everybody computes when some lane's operand is
// outside [2^-60, 2^60] (a direction along the normal: sin_theta == 0)
struct Phi { float c, s; };
// st = sin_theta(w), which the callers share with tan_theta (the same square root: 1 - z * z where that is positive)
TRC_DEV float tan_theta_st(F3 v, float st) {
    float temp = 1 - v.z * v.z;
    if (temp <= 0.0f || v.z == 0.0f) return 0.0f;
    return st / v.z;
}
TRC_DEV Phi phi_of(F3 w, float st) {
    Phi ph;
#if TRC_WAVE_GUARDS
    const GuardedDivBy by = guarded_div_by(st);
    float qc = div_core(w.x, by), qs = div_core(w.y, by);
    const float small = fmin3(fabsf(w.x), fabsf(w.y), st), large = fmax3(fabsf(w.x), fabsf(w.y), st);
    if (__builtin_expect(!wave_all(small >= 0x1p-60f && large <= 0x1p60f), 0)) { qc = w.x / st; qs = w.y / st; }
    ph.c = (st == 0) ? 1 : clampf(qc, -1.0f, 1.0f);
    ph.s = (st == 0) ? 0 : clampf(qs, -1.0f, 1.0f);
#else
    ph.c = (st == 0) ? 1 : clampf(w.x / st, -1.0f, 1.0f);
    ph.s = (st == 0) ? 0 : clampf(w.y / st, -1.0f, 1.0f);
#endif
    return ph;
}
TRC_DEV Phi phi_of(F3 w) { return phi_of(w, sin_theta(w)); }

// ---------------------------------------------------------------- Math.hh:118-167
TRC_DEV float erf_inv(float x) {
    float w, p;
    x = clampf(x, -.99999f, .99999f);
    w = -dm_logf_pos((1 - x) * (1 + x));             // the clamp above leaves (1 - x)(1 + x) in [2e-5, 1], whatever x was
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
        w = sqrt_cr(w) - 3;
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
TRC_DEV float erf_approx(float x) {
    const float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f;
    const float p = 0.3275911f;
    int sign = 1;
    if (x < 0) sign = -1;
    x = fabsf(x);
    float t = rcp1(1 + p * x);
    float y = 1 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * dm_expf(-x * x);
    return sign * y;
}
// erf_approx with its exponential handed in: e must be what dm_expf returns for -x * x with x = |x| (sample11_once, which needs the
// same value once more)
TRC_DEV float erf_approx_exp(float x, float e) {
    const float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f;
    const float p = 0.3275911f;
    int sign = 1;
    if (x < 0) sign = -1;
    x = fabsf(x);
    float t = rcp1(1 + p * x);
    float y = 1 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * e;
    return sign * y;
}

// ---------------------------------------------------------------- BXDF.hh / BXDF.metal
TRC_DEV F3 reflect(F3 wo, F3 n) { return -wo + 2 * dot(wo, n) * n; }             // BXDF.hh:24-26
TRC_DEV bool refract(F3 wo, F3 n, float eta, F3& wi) {                            // BXDF.hh:28-41 (cos from wo.z, B-6)
    float cosThetaI = wo.z;
    float sin2ThetaI = fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI);
    float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return false;
    float cosThetaT = sqrt_cr(1 - sin2ThetaT);
    wi = eta * -wo + (eta * cosThetaI - cosThetaT) * n;
    return true;
}
TRC_DEV float fr_dielectric(float cosi, float eta) {                              // BXDF.metal:3-22
    cosi = clampf(cosi, -1.0f, 1.0f);
    bool entering = cosi > 0.f;
    if (!entering) { eta = rcp1(eta); cosi = -cosi; }
    float sin2Theta_i = 1 - cosi * cosi;
    float sin2Theta_t = sin2Theta_i / sqr(eta);
    if (sin2Theta_t >= 1) return 1.f;
    float cosTheta_t = sqrt_cr(fmaxf(0.0f, 1 - sin2Theta_t));
    float r_parl = (eta * cosi - cosTheta_t) / (eta * cosi + cosTheta_t);
    float r_perp = (cosi - eta * cosTheta_t) / (cosi + eta * cosTheta_t);
    return (r_parl * r_parl + r_perp * r_perp) / 2;
}
template <bool METAL_CONSTANTS = false>
TRC_DEV F3 fr_conductor(float cosi, F3 eta, F3 k) {                               // BXDF.metal:24-34
    F3 tmp = (eta * eta + k * k) * cosi * cosi;
    const F3 n1 = tmp - (2.f * eta * cosi) + f3(1), d1 = tmp + (2.f * eta * cosi) + f3(1);
    F3 tmp_f = eta * eta + k * k;
    const F3 n2 = tmp_f - (2.f * eta * cosi) + f3(cosi * cosi), d2 = tmp_f + (2.f * eta * cosi) + f3(cosi * cosi);
#if TRC_WAVE_GUARDS
    if (METAL_CONSTANTS) {
    // MetalMaterial's constants (eta <= 0.81, k = 1) and 0 <= cosi <= 2 put all twelve operands into [0.5, 16]:
    // n1 = (eta^2 + 1) c^2 - 2 eta c + 1 >= 1 / (eta^2 + 1), n2 = (c - eta)^2 + 1 >= 1, the denominators are sums of
    // non-negative terms and 1 -- the six quotients need no operand guard beyond that ONE compare (which a NaN fails)
    F3 Rparl2 = div_core(n1, d1), Rperp2 = div_core(n2, d2);
    if (__builtin_expect(!wave_all(cosi >= 0.0f && cosi <= 2.0f), 0)) { Rparl2 = n1 / d1; Rperp2 = n2 / d2; }
    return 0.5f * (Rparl2 + Rperp2);
    }
#endif
    F3 Rparl2 = n1 / d1, Rperp2 = n2 / d2;
    return 0.5f * (Rparl2 + Rperp2);
}

// Fresnel policies
struct FrCond {   // BXDF.hh:59-70; MetalMaterial: eta = (0.18, 0.15, 0.81), k = 1 (MicrofacetBXDF.h:445-449)
    TRC_DEV static F3 eval(float cosThetaI) { return fr_conductor<true>(fabsf(cosThetaI), f3(0.18f, 0.15f, 0.81f), f3(1.0f)); }
};
struct FrDiel15 { // BXDF.hh:72-81 with eta = 1.5 (Plastic, Glass reflection)
    TRC_DEV static F3 eval(float cosThetaI) { return f3(fr_dielectric(cosThetaI, 1.5f)); }
};

// ---------------------------------------------------------------- microfacet distributions
// alpha is already clamped to >= 0.001 by the constructors (MicrofacetBXDF.h:164,306-309)
// roughness pairs as types (float literals must match the reference's exactly)
struct Alpha_01_02 {
    TRC_DEV static float x() { return 0.01f; }
    TRC_DEV static float y() { return 0.02f; }
    TRC_DEV static DivConst by_x2() { return div_by_sqr001(); }      // max(0.001, x)^2 and its reciprocal
    TRC_DEV static DivConst by_y2() { return div_by_sqr002(); }
};

// TRC_SAMPLE11_ONCE (read by material_S_F): Beckmann's sample11 with each transcendental body evaluated once per lane and once per
// wavefront.  0 is the reference's text as Beckmann::sample11 and Microfacet::sample11 below state it.  Otherwise a set of bits:
//   1  exp(-cot^2) once: erf_approx's exponential and the normalisation's are the same float (see sample11_once);
//   2  slope_x = erf_inv(b) after the Newton loop is the loop's last invErf wherever the loop was left by `break`: b has not been
//      written since.  Only a lane that ran out of iterations evaluates erf_inv(b) again, in a last trip of the loop;
//   4  one logarithm core ahead of the corner's branch, for the corner's -log(1 - U1) and the Newton lanes' log(base), which are
//      disjoint lanes of one wavefront; the special operands of the corner's dm_logf are patched in afterwards.
// Every lane computes the bits of the reference's text (trc_sample11_test and trc_material_s_f_test hold the two texts against each
// other).  A translation unit sets it before including this header; 7 is all three, which the units of LDS-resident trees set
// (profiles/r31).  CAP is the loop's bound, 10 everywhere but in the hook, which forces the running-out exit with 2 and 3.
#ifndef TRC_SAMPLE11_ONCE
#define TRC_SAMPLE11_ONCE 0
#endif
constexpr int kOnceExp = 1, kOnceErfInv = 2, kOnceLog = 4;
// how a lane left sample11 (the hook reports it)
constexpr int kS11Corner = 0, kS11Break = 1, kS11RanOut = 2, kS11ClosedForm = 3;

// tr: the lane is a Trowbridge-Reitz lane of the microfacet stream (Microfacet::sample11); false for all lanes from Beckmann::sample11
template <int ONCE, int CAP>
TRC_DEV int sample11_once(const bool tr, float cosTheta, float sinTheta, float U1, float U2, float& slope_x, float& slope_y) {
    const bool corner = cosTheta > .9999f;
    const float sample_x = fmaxf(U1, 1e-6f);
    const float base = 1 - sample_x;
    float lg = 0;                                     // corner: dm_logf(1 - U1); Newton lanes: dm_logf_pos(base == 0 ? 1 : base)
    if constexpr ((ONCE & kOnceLog) != 0) {
        // dm_logf is dm_logf_pos behind three operand tests (NaN, <= 0, +inf): the core sees 1.0 on such a lane and the result is
        // overwritten, as dm_asinf patches its special operands in.  Trowbridge-Reitz lanes take no logarithm: they ride along on 1.0
        // and nobody reads their lg.  A Newton lane hands the core the operand the reference's text hands it.
        const float om = 1.0f - U1;
        const bool plain = om > 0.0f && om != DM_INF_F;                 // false for a NaN
        float operand = corner ? (plain ? om : 1.0f) : (base == 0.0f ? 1.0f : base);
        if (tr) operand = 1.0f;
        lg = dm_logf_pos(operand);
        if (corner && !plain) lg = (om != om || om == DM_INF_F) ? om : (om == 0.0f) ? -DM_INF_F : DM_NAN_F;
    }
    if (corner) {
        float r2;                                     // each family's own radius, one root
        if (tr) r2 = U1 / (1 - U1);
        else r2 = -((ONCE & kOnceLog) != 0 ? lg : dm_logf(1.0f - U1));
        float r = sqrt_cr(r2);
        const float phi = tr ? 6.28318530718f * U2 : 2 * kPi * U2;      // each family's own literal
        float s, c;
        dm_sincosf(phi, &s, &c);
        slope_x = r * c;
        slope_y = r * s;
        return kS11Corner;
    }
    const float tanTheta = sinTheta / cosTheta;
    const float cotTheta = rcp1(tanTheta);
    if (tr) {                                         // TrowbridgeReitzD::sample11: the closed form
        const float a = cotTheta;
        float G1 = 2 * rcp1(1 + sqrt_cr(1.f + rcp1(a * a)));
        float A = 2 * U1 / G1 - 1;
        float tmp = rcp1(A * A - 1.f);
        if (tmp > 1e10f) tmp = 1e10f;
        float B = tanTheta;
        float D = sqrt_cr(fmaxf(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
        float slope_x_1 = B * tmp - D;
        float slope_x_2 = B * tmp + D;
        slope_x = (A < 0 || slope_x_2 > a) ? slope_x_1 : slope_x_2;
        float S;
        if (U2 > 0.5f) { S = 1.f; U2 = 2.f * (U2 - .5f); }
        else { S = -1.f; U2 = 2.f * (.5f - U2); }
        float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
                  (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
        slope_y = S * z * sqrt_cr(1.f + slope_x * slope_x);
        return kS11ClosedForm;
    }
    const float tanThetaI = tanTheta, cotThetaI = cotTheta, cosThetaI = cosTheta;      // Beckmann::sample11: the Newton iteration
    // exp(-cot^2): erf_approx states it as -x * x with x = |cot|, the normalisation as -cot * cot.  A float product is the product of
    // the magnitudes, rounded, under the exclusive-or of the signs; (-|c|, |c|) and (-c, c) have the same magnitudes and one negative
    // operand each, so the two arguments are the same float for every c that is a number and dm_expf runs once.  For a NaN c both are
    // NaNs, whose sign and payload may differ: what they reach (c, the normalisation, value) is a NaN in both texts, of whichever
    // sign -- the hooks' tests count a NaN equal to a NaN --, and a sample whose colour comes out NaN is replaced by 0 in finish_sample.
    const float xa = fabsf(cotThetaI);
    const float e = (ONCE & kOnceExp) != 0 ? dm_expf(-xa * xa) : 0.0f;
    float a = -1, c = (ONCE & kOnceExp) != 0 ? erf_approx_exp(cotThetaI, e) : erf_approx(cotThetaI);
    float thetaI = dm_acosf(cosThetaI);
    float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
    if constexpr ((ONCE & kOnceLog) == 0) lg = dm_logf_pos(base == 0.0f ? 1.0f : base);
    const float pw = dm_expf_fin(fit * lg);
    float b = c - (1 + c) * (base == 0.0f ? 0.0f : pw);
    const float SQRT_PI_INV = 1.f / sqrtf(kPi);
    float normalization = rcp1(1 + c + SQRT_PI_INV * tanThetaI * ((ONCE & kOnceExp) != 0 ? e : dm_expf(-cotThetaI * cotThetaI)));
    int it = 0;
    if constexpr ((ONCE & kOnceErfInv) != 0) {
        // the reference's slope_x = erf_inv(b) after the loop as one more trip of the loop's own erf_inv: a lane that leaves by `break`
        // holds erf_inv of the b it leaves with (nothing wrote b since); a lane that runs out of iterations takes a last trip that
        // neither clamps b to [a, c] nor steps -- erf_inv(b) on the b the last step left, as the reference evaluates it.  The
        // wavefront takes that trip only while such a lane is in it, and sample11 holds one erf_inv body less.
        for (;;) {
            const bool last = !(++it < CAP);
            if (!last && !(b >= a && b <= c)) b = 0.5f * (a + c);
            const float invErf = erf_inv(b);
            slope_x = invErf;
            if (last) break;
            float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_expf_fin(-invErf * invErf)) - sample_x;  // |erf_inv| < 3.2
            float derivative = normalization * (1 - invErf * tanThetaI);
            if (fabsf(value) < 1e-5f) break;
            if (value > 0) c = b; else a = b;
            b -= value / derivative;
        }
    } else {
        while (++it < CAP) {
            if (!(b >= a && b <= c)) b = 0.5f * (a + c);
            float invErf = erf_inv(b);
            float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_expf_fin(-invErf * invErf)) - sample_x;  // |erf_inv| < 3.2
            float derivative = normalization * (1 - invErf * tanThetaI);
            if (fabsf(value) < 1e-5f) break;
            if (value > 0) c = b; else a = b;
            b -= value / derivative;
        }
        slope_x = erf_inv(b);
    }
    // `break` leaves it < CAP, running out it == CAP
    const bool ran_out = !(it < CAP);
    slope_y = erf_inv(2.0f * fmaxf(U2, 1e-6f) - 1.0f);
    return ran_out ? kS11RanOut : kS11Break;
}

// Beckmann distribution, MicrofacetBXDF.h:137-290.  The roughness pair is a run-time value (not a template
// parameter) on purpose: Plastic's specular lobe (0.01, 0.1) and Glass's reflection and transmission lobes
// (0.01, 0.01) then run the SAME instructions, so a wavefront holding lanes of several of these lobes executes
// the expensive visible-normal sampling (a Newton iteration over erf^-1 / exp) once instead of once per lobe.
struct Beckmann {
    float alpha_x, alpha_y;
    DivConst by_ax2, by_ay2;         // alpha^2 and its reciprocal (D divides by them)
    // the two roughness pairs the materials use: Plastic's specular lobe (0.01, 0.1), Glass's lobes (0.01, 0.01)
    TRC_DEV static Beckmann make_lobe(bool plastic) {
        Beckmann d; d.alpha_x = fmaxf(0.001f, 0.01f); d.alpha_y = fmaxf(0.001f, plastic ? 0.1f : 0.01f);
        d.by_ax2 = div_by_sqr001();
        const DivConst rough = div_by_sqr01(), smooth = div_by_sqr001();
        d.by_ay2.c = plastic ? rough.c : smooth.c; d.by_ay2.y = plastic ? rough.y : smooth.y;
        return d;
    }
    TRC_DEV float ax() const { return alpha_x; }
    TRC_DEV float ay() const { return alpha_y; }

    TRC_DEV float lambda(F3 w) const {
        const float st = sin_theta(w);
        float absTanTheta = fabsf(tan_theta_st(w, st));
        if (is_inf(absTanTheta)) return 0.;
        const Phi ph = phi_of(w, st);
        float alpha = sqrt_cr((ph.c * ph.c) * ax() * ax() + (ph.s * ph.s) * ay() * ay());
        float a = rcp1(alpha * absTanTheta);
        if (a >= 1.6f) return 0;
        return (1 - 1.259f * a + 0.396f * a * a) / (3.535f * a + 2.181f * a * a);
    }
    TRC_DEV float D(F3 wh) const {
        float tan2Theta = tan2_theta(wh);
        if (is_inf(tan2Theta)) return 0.;
        float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
        const Phi ph = phi_of(wh);
        float qc, qs;                                     // cos2_phi / (ax * ax), sin2_phi / (ay * ay)
        div_const2(ph.c * ph.c, by_ax2, ph.s * ph.s, by_ay2, qc, qs);
        return dm_expf(-tan2Theta * (qc + qs)) /
               (kPi * ax() * ay() * cos4Theta);
    }
    TRC_DEV float G1(F3 w) const { return rcp1(1 + lambda(w)); }
    TRC_DEV float G(F3 wo, F3 wi) const { return rcp1(1 + lambda(wo) + lambda(wi)); }
    TRC_DEV float pdf(F3 wo, F3 wh) const { return D(wh) * G1(wo) * fabsf(dot(wo, wh)) / abs_cos_theta(wo); }

    // returns how the lane left (kS11Corner, kS11Break, kS11RanOut); ONCE != 0: sample11_once above
    template <int ONCE = 0, int CAP = 10>
    TRC_DEV static int sample11(float cosThetaI, float sinThetaI, float U1, float U2, float& slope_x, float& slope_y) {
        if constexpr (ONCE != 0) return sample11_once<ONCE, CAP>(false, cosThetaI, sinThetaI, U1, U2, slope_x, slope_y);
        if (cosThetaI > .9999f) {
            float r = sqrt_cr(-dm_logf(1.0f - U1));
            float sinPhi, cosPhi;
            dm_sincosf(2 * kPi * U2, &sinPhi, &cosPhi);
            slope_x = r * cosPhi;
            slope_y = r * sinPhi;
            return kS11Corner;
        }
        float tanThetaI = sinThetaI / cosThetaI;          // sinThetaI = sqrt(max(0, 1 - cosThetaI^2)) = sin_theta of the caller's vector
        float cotThetaI = rcp1(tanThetaI);
        float a = -1, c = erf_approx(cotThetaI);
        float sample_x = fmaxf(U1, 1e-6f);
        float thetaI = dm_acosf(cosThetaI);
        float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
        // dm_powf(1 - sample_x, fit) with its operands' ranges used: the base lies in {0} U [2^-24, 1), the exponent in [0.44, 1]
        // (fit's minimum over [0, pi]), so log and exp need none of their special cases; a NaN here is replaced by the
        // bisection step below before anybody sees it
        const float base = 1 - sample_x;
        const float pw = dm_expf_fin(fit * dm_logf_pos(base == 0.0f ? 1.0f : base));
        float b = c - (1 + c) * (base == 0.0f ? 0.0f : pw);
        const float SQRT_PI_INV = 1.f / sqrtf(kPi);
        float normalization = rcp1(1 + c + SQRT_PI_INV * tanThetaI * dm_expf(-cotThetaI * cotThetaI));
        int it = 0;
        while (++it < CAP) {
            if (!(b >= a && b <= c)) b = 0.5f * (a + c);
            float invErf = erf_inv(b);
            float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_expf_fin(-invErf * invErf)) - sample_x;      // |erf_inv| < 3.2
            float derivative = normalization * (1 - invErf * tanThetaI);
            if (fabsf(value) < 1e-5f) break;
            if (value > 0) c = b; else a = b;
            b -= value / derivative;
        }
        slope_x = erf_inv(b);
        slope_y = erf_inv(2.0f * fmaxf(U2, 1e-6f) - 1.0f);
        return it < CAP ? kS11Break : kS11RanOut;
    }
    template <int ONCE = 0>
    TRC_DEV F3 sample_wh(F3 wo, F2 u) const {
        const bool flip = wo.z < 0;
        const F3 wi = flip ? -wo : wo;
        F3 wiStretched = normalize(f3(ax() * wi.x, ay() * wi.y, wi.z));
        float slope_x, slope_y;
        const float st = sin_theta(wiStretched);
        sample11<ONCE>(cos_theta(wiStretched), st, u.x, u.y, slope_x, slope_y);
        const Phi ph = phi_of(wiStretched, st);
        float tmp = ph.c * slope_x - ph.s * slope_y;
        slope_y = ph.s * slope_x + ph.c * slope_y;
        slope_x = tmp;
        slope_x = ax() * slope_x;
        slope_y = ay() * slope_y;
        F3 wh = normalize(f3(-slope_x, -slope_y, 1.f));
        return flip ? -wh : wh;
    }
};

template <class Alpha>
struct TrowbridgeReitzD {                                            // MicrofacetBXDF.h:292-434
    TRC_DEV static float ax() { return fmaxf(0.001f, Alpha::x()); }
    TRC_DEV static float ay() { return fmaxf(0.001f, Alpha::y()); }

    TRC_DEV static float D(F3 wh) {
        float tan2Theta = tan2_theta(wh);
        if (is_inf(tan2Theta)) return 0.;
        const float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
        if (cos4Theta < 1e-16f) return 0;
        const Phi ph = phi_of(wh);
        float qc, qs;                                     // cos2_phi / ax^2, sin2_phi / ay^2
        div_const2(ph.c * ph.c, Alpha::by_x2(), ph.s * ph.s, Alpha::by_y2(), qc, qs);
        float e = (qc + qs) * tan2Theta;
        return rcp1(kPi * ax() * ay() * sqr(1 + e) * cos4Theta);
    }
    TRC_DEV static float lambda(F3 w) {
        float tan2Theta = tan2_theta(w);
        if (is_inf(tan2Theta)) return 0.;
        const Phi ph = phi_of(w);
        float alpha2 = sqr(ph.c * ax()) + sqr(ph.s * ay());
        return 0.5f * (sqrt_cr(1 + alpha2 * tan2Theta) - 1);
    }
    TRC_DEV static float G1(F3 w) { return rcp1(1 + lambda(w)); }
    TRC_DEV static float G(F3 wo, F3 wi) { return rcp1(1 + lambda(wo) + lambda(wi)); }
    TRC_DEV static float pdf(F3 wo, F3 wh) { return D(wh) * G1(wo) * fabsf(dot(wo, wh) / cos_theta(wo)); }

    TRC_DEV static void sample11(float cosTheta, float sinTheta, float U1, float U2, float& slope_x, float& slope_y) {
        if (cosTheta > .9999f) {
            float r = sqrt_cr(U1 / (1 - U1));
            float phi = 6.28318530718f * U2;
            float s, c;
            dm_sincosf(phi, &s, &c);
            slope_x = r * c;
            slope_y = r * s;
            return;
        }
        float tanTheta = sinTheta / cosTheta;             // sinTheta = sqrt(max(0, 1 - cosTheta^2)) = sin_theta of the caller's vector
        float a = rcp1(tanTheta);
        float G1 = 2 * rcp1(1 + sqrt_cr(1.f + rcp1(a * a)));     // 2 / x == 2 * (1 / x) bit for bit: x is 1 + a root, so 1 / x is never denormal and the doubling is exact
        float A = 2 * U1 / G1 - 1;
        float tmp = rcp1(A * A - 1.f);
        if (tmp > 1e10f) tmp = 1e10f;
        float B = tanTheta;
        float D = sqrt_cr(fmaxf(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
        float slope_x_1 = B * tmp - D;
        float slope_x_2 = B * tmp + D;
        slope_x = (A < 0 || slope_x_2 > a) ? slope_x_1 : slope_x_2;              // a = 1 / tanTheta
        float S;
        if (U2 > 0.5f) { S = 1.f; U2 = 2.f * (U2 - .5f); }
        else { S = -1.f; U2 = 2.f * (.5f - U2); }
        float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
                  (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
        slope_y = S * z * sqrt_cr(1.f + slope_x * slope_x);
    }
    TRC_DEV static F3 sample_wh(F3 wo, F2 u) {
        const bool flip = wo.z < 0;
        const F3 wi = flip ? -wo : wo;
        F3 wiStretched = normalize(f3(ax() * wi.x, ay() * wi.y, wi.z));
        float slope_x, slope_y;
        const float st = sin_theta(wiStretched);
        sample11(cos_theta(wiStretched), st, u.x, u.y, slope_x, slope_y);
        const Phi ph = phi_of(wiStretched, st);
        float tmp = ph.c * slope_x - ph.s * slope_y;
        slope_y = ph.s * slope_x + ph.c * slope_y;
        slope_x = tmp;
        slope_x = ax() * slope_x;
        slope_y = ay() * slope_y;
        F3 wh = normalize(f3(-slope_x, -slope_y, 1.f));
        return flip ? -wh : wh;
    }
};

// ---------------------------------------------------------------- lobes
struct Lambert {                                                     // MatteBXDF.hh:6-22 (F folds in the cosine)
    TRC_DEV static float F(F3, F3 wi) { return wi.z / kPi; }
    TRC_DEV static float pdf(F3 wo, F3 wi) { return wo.z * wi.z > 0 ? fabsf(wi.z) / kPi : 0; }
    // value and pdf are the same quotient: wi.z comes out of a square root (never negative), so |wi.z| / pi == wi.z / pi
    TRC_DEV static float S_F(F3 wo, F3& wi, F2 uu, float& pdf_out) {
        wi = cosine_sample_hemisphere(uu);
        const float v = div_pi(wi.z);
        pdf_out = wo.z * wi.z > 0 ? fabsf(v) : 0;
        return v;
    }
};

template <class Dist, class Fr>
struct MicroRefl {                                                   // MicrofacetBXDF.h:7-62
    TRC_DEV static F3 F(float R, F3 wo, F3 wi) {
        float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
        if (cosThetaI == 0 || cosThetaO == 0) return f3(0);
        F3 wh = wi + wo;
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return f3(0);
        wh = normalize(wh);
        // Faceforward(wh, (0,0,1)): dot(wh,(0,0,1)) is evaluated like the oracle does
        const float d001 = wh.x * 0.0f + wh.y * 0.0f + wh.z * 1.0f;
        const F3 whf = (d001 < 0.f) ? -wh : wh;
        F3 Fres = Fr::eval(dot(wi, whf));
        return f3(R) * Dist::D(wh) * Dist::G(wo, wi) * Fres / (4 * cosThetaI * cosThetaO);
    }
    TRC_DEV static float pdf(F3 wo, F3 wi) {
        if (wo.z * wi.z <= 0) return 0;
        F3 wh = normalize(wo + wi);
        return Dist::pdf(wo, wh) / (4 * dot(wo, wh));
    }
    // pdf(wo, wh) and F(wo, wi) both need Lambda(wo): written out so that it is computed ONCE (the guarded square roots and
    // reciprocals inside carry wave-level branches, which the compiler will not merge across the two calls).  Every
    // expression is the one pdf() and F() above evaluate, on the same operands in the same order.
    TRC_DEV static F3 S_F(float R, F3 wo, F3& wi, F2 uu, float& pdf_out) {
        if (wo.z == 0) return f3(0);
        F3 wh = Dist::sample_wh(wo, uu);
        if (dot(wo, wh) <= 0) return f3(0);
        wi = reflect(wo, wh);
        if (wo.z * wi.z <= 0) return f3(0);
        const float lam_o = Dist::lambda(wo);
        const float dist_pdf = Dist::D(wh) * rcp1(1 + lam_o) * fabsf(dot(wo, wh) / cos_theta(wo));      // Dist::pdf(wo, wh)
        pdf_out = dist_pdf / (4 * dot(wo, wh));
        float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);                                // F(R, wo, wi)
        if (cosThetaI == 0 || cosThetaO == 0) return f3(0);
        F3 wh2 = wi + wo;
        if (wh2.x == 0 && wh2.y == 0 && wh2.z == 0) return f3(0);
        wh2 = normalize(wh2);
        const float d001 = wh2.x * 0.0f + wh2.y * 0.0f + wh2.z * 1.0f;
        const F3 whf = (d001 < 0.f) ? -wh2 : wh2;
        F3 Fres = Fr::eval(dot(wi, whf));
        const float G = rcp1(1 + lam_o + Dist::lambda(wi));                                               // Dist::G(wo, wi)
        return f3(R) * Dist::D(wh2) * G * Fres / (4 * cosThetaI * cosThetaO);
    }
};

// MicrofacetReflection over a run-time Beckmann distribution with FresnelDielectric(1.5): Plastic's specular
// lobe (R = 1) and Glass's reflection lobe (R = kr = 0.98).  Same expressions as MicroRefl above.
struct BeckRefl {
    TRC_DEV static F3 F(const Beckmann& d, float R, F3 wo, F3 wi) {
        float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
        if (cosThetaI == 0 || cosThetaO == 0) return f3(0);
        F3 wh = wi + wo;
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return f3(0);
        wh = normalize(wh);
        const float d001 = wh.x * 0.0f + wh.y * 0.0f + wh.z * 1.0f;
        const F3 whf = (d001 < 0.f) ? -wh : wh;
        F3 Fres = FrDiel15::eval(dot(wi, whf));
        return f3(R) * d.D(wh) * d.G(wo, wi) * Fres / (4 * cosThetaI * cosThetaO);
    }
    TRC_DEV static float pdf(const Beckmann& d, F3 wo, F3 wi) {
        if (wo.z * wi.z <= 0) return 0;
        F3 wh = normalize(wo + wi);
        return d.pdf(wo, wh) / (4 * dot(wo, wh));
    }
    // S_F after wh = d.sample_wh(wo, u) (MicrofacetBXDF.h:36-48); pdf_out untouched on the zero returns
    TRC_DEV static F3 finish(const Beckmann& d, float R, F3 wo, F3 wh, F3& wi, float& pdf_out) {
        if (dot(wo, wh) <= 0) return f3(0);
        wi = reflect(wo, wh);
        if (wo.z * wi.z <= 0) return f3(0);
        pdf_out = d.pdf(wo, wh) / (4 * dot(wo, wh));
        return F(d, R, wo, wi);
    }
};

// MicrofacetBXDF.h:64-135 as instantiated by GlassMaterial (:541): T = 0.98, etaA = 1, etaB = 1.5,
// mode = Importance (factor 1), and its own Fresnel is FresnelDielectric(etaA = 1.0) (:81).
struct BeckTransGlass {
    TRC_DEV static F3 F(const Beckmann& d, F3 wo, F3 wi) {
        const float etaA = 1.0f, etaB = 1.5f;
        if (wo.z * wi.z > 0) return f3(0);
        float cosThetaO = cos_theta(wo), cosThetaI = cos_theta(wi);
        if (cosThetaI == 0 || cosThetaO == 0) return f3(0);
        float eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
        F3 wh = normalize(wo + wi * eta);
        if (wh.z < 0) wh = -wh;
        if (dot(wo, wh) * dot(wi, wh) > 0) return f3(0);
        F3 Fres = f3(fr_dielectric(dot(wo, wh), etaA));
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float factor = 1;
        return (f3(1.0f) - Fres) * f3(0.98f) *
               fabsf(d.D(wh) * d.G(wo, wi) * eta * eta * fabsf(dot(wi, wh)) * fabsf(dot(wo, wh)) * factor * factor /
                     (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
    }
    TRC_DEV static float pdf(const Beckmann& d, F3 wo, F3 wi) {
        const float etaA = 1.0f, etaB = 1.5f;
        if (wo.z * wi.z > 0) return 0;
        float eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
        F3 wh = normalize(wo + wi * eta);
        if (dot(wo, wh) * dot(wi, wh) > 0) return 0;
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrtDenom * sqrtDenom));
        return d.pdf(wo, wh) * dwh_dwi;
    }
    // S_F after wh = d.sample_wh(wo, u) (MicrofacetBXDF.h:117-133)
    TRC_DEV static F3 finish(const Beckmann& d, F3 wo, F3 wh, F3& wi, float& pdf_out) {
        const float etaA = 1.0f, etaB = 1.5f;
        if (dot(wo, wh) < 0) return f3(0);
        float eta = cos_theta(wo) > 0 ? (etaA / etaB) : (etaB / etaA);
        if (!refract(wo, wh, eta, wi)) return f3(0);
        pdf_out = pdf(d, wo, wi);
        return F(d, wo, wi);
    }
};

// Tail of S_F for the three Beckmann lobes after wh = d.sample_wh(wo, u): MicrofacetReflection::S_F
// (MicrofacetBXDF.h:36-48 -> PDF :50-57, F :15-34) and MicrofacetTransmission::S_F (:117-133 -> PDF :100-115,
// F :83-98).  Written in three phases so that reflection and transmission lanes of a wavefront share the
// expensive part: (A) per-lobe geometry and the lobe's early-outs, (B) D, Lambda and the dielectric Fresnel
// term -- one instruction stream for all lanes, (C) per-lobe combination.  Every expression is the
// reference's, evaluated on the same operands in the same order; D(-w) == D(w) bit for bit (w enters only
// through squares), which is why transmission needs one D.  pdf_out is left untouched on the early-outs.
TRC_DEV F3 beckmann_finish(const Beckmann& d, bool refl, float R, F3 wo, F3 wh, F3& wi_out, float& pdf_out) {
    const float etaA = 1.0f, etaB = 1.5f;
    bool live;                    // got past the early-outs of S_F: pdf_out will be written
    bool pdf_live = false;        // ... with a non-trivial value
    bool f_live = false;          // F reaches its D * G * Fresnel expression
    F3 wi = wi_out, whA = wh, whB = wh;
    float eta = 0, fres_cos = 0, fres_eta = 1.5f;
    // ---- (A)
    if (refl) {
        live = !(dot(wo, wh) <= 0);
        if (live) { wi = reflect(wo, wh); live = !(wo.z * wi.z <= 0); }
        if (live) {
            pdf_live = true;
            const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
            F3 sum = wi + wo;
            f_live = !(cosThetaI == 0 || cosThetaO == 0) && !(sum.x == 0 && sum.y == 0 && sum.z == 0);
            if (f_live) {
                whB = normalize(sum);
                const float d001 = whB.x * 0.0f + whB.y * 0.0f + whB.z * 1.0f;      // Faceforward(wh, (0,0,1))
                const F3 whf = (d001 < 0.f) ? -whB : whB;
                fres_cos = dot(wi, whf);
                fres_eta = 1.5f;
            }
        }
    } else {
        live = !(dot(wo, wh) < 0);
        if (live) live = refract(wo, wh, cos_theta(wo) > 0 ? (etaA / etaB) : (etaB / etaA), wi);
        if (live) {
            eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
            const bool same_side = wo.z * wi.z > 0;
            whA = normalize(wo + wi * eta);
            const bool backfacing = dot(wo, whA) * dot(wi, whA) > 0;               // same truth value for -whA
            pdf_live = !same_side && !backfacing;
            whB = whA;
            if (whB.z < 0) whB = -whB;
            f_live = pdf_live && !(cos_theta(wi) == 0 || cos_theta(wo) == 0);
            fres_cos = dot(wo, whB);
            fres_eta = etaA;
        }
    }
    // ---- (B)
    float D_A = 0, D_B = 0, lam_o = 0, lam_i = 0, fres = 0;
    if (pdf_live) {
        lam_o = d.lambda(wo);
        D_A = d.D(whA);
        D_B = D_A;
        if (refl && f_live) D_B = d.D(whB);
        if (f_live) {
            lam_i = d.lambda(wi);
            fres = fr_dielectric(fres_cos, fres_eta);
        }
    }
    // ---- (C)
    F3 out = f3(0);
    if (live) {
        wi_out = wi;
        const float G1 = rcp1(1 + lam_o);
        const float G = rcp1(1 + lam_o + lam_i);
        if (refl) {
            const float dist_pdf = D_A * G1 * fabsf(dot(wo, wh)) / abs_cos_theta(wo);
            pdf_out = dist_pdf / (4 * dot(wo, wh));
            if (f_live) {
                const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
                out = f3(R) * D_B * G * f3(fres) / (4 * cosThetaI * cosThetaO);
            }
        } else {
            float p = 0;
            if (pdf_live) {
                const float sqrtDenom = dot(wo, whA) + eta * dot(wi, whA);
                const float dwh_dwi = fabsf((eta * eta * dot(wi, whA)) / (sqrtDenom * sqrtDenom));
                const float dist_pdf = D_A * G1 * fabsf(dot(wo, whA)) / abs_cos_theta(wo);
                p = dist_pdf * dwh_dwi;
            }
            pdf_out = p;
            if (f_live) {
                const float cosThetaO = cos_theta(wo), cosThetaI = cos_theta(wi);
                const float sqrtDenom = dot(wo, whB) + eta * dot(wi, whB);
                const float factor = 1;
                out = (f3(1.0f) - f3(fres)) * f3(0.98f) *
                      fabsf(D_B * G * eta * eta * fabsf(dot(wi, whB)) * fabsf(dot(wo, whB)) * factor * factor /
                            (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
            }
        }
    }
    return out;
}

// ---------------------------------------------------------------- one stream for the four microfacet lobes
// TRC_MICROFACET_STREAM (read by material_S_F): the Metal lobe (Trowbridge-Reitz (0.01, 0.02), conductor Fresnel) runs through the
// instruction stream of the three Beckmann lobes instead of a branch of its own beside them -- a wavefront that holds Metal lanes
// and Plastic / Glass lanes then issues the skeleton the two families share (stretch, phi_of, rotate, unstretch, reflect, the
// normalisations, the final quotients) once.  The family is a per-lane value like the roughness pair; what differs between the
// families (sample11's bodies, the tails of Lambda and D, the Fresnel term, two literals) stays each family's own expression.
// Every lane evaluates the reference's expressions for its material on the same operands in the same order
// (trc_material_s_f_test holds the two forms against each other bit for bit).  A translation unit sets it before including this header.
#ifndef TRC_MICROFACET_STREAM
#define TRC_MICROFACET_STREAM 0
#endif

struct Microfacet {
    bool tr;                         // Trowbridge-Reitz (Metal), else Beckmann (Plastic's specular lobe, Glass's two lobes)
    float alpha_x, alpha_y;
    DivConst by_ax2, by_ay2;         // alpha^2 and its reciprocal (D divides by them)
    TRC_DEV static Microfacet make_lobe(bool metal, bool plastic) {
        Microfacet d; d.tr = metal;
        d.alpha_x = fmaxf(0.001f, 0.01f); d.alpha_y = fmaxf(0.001f, metal ? 0.02f : plastic ? 0.1f : 0.01f);
        d.by_ax2 = div_by_sqr001();
        const DivConst rough = div_by_sqr01(), mid = div_by_sqr002(), smooth = div_by_sqr001();
        d.by_ay2.c = metal ? mid.c : plastic ? rough.c : smooth.c; d.by_ay2.y = metal ? mid.y : plastic ? rough.y : smooth.y;
        return d;
    }
    // TRC_FLAG_MATERIAL_PARAMS: any roughness pair, clamped as the reference's constructors clamp it; by_*.c is alpha^2, and by_*.y is
    // not a reciprocal anybody may use -- only D_general below divides by such a lobe's squares
    TRC_DEV static Microfacet make_lobe(bool metal, float ax, float ay) {
        Microfacet d; d.tr = metal;
        d.alpha_x = fmaxf(0.001f, ax); d.alpha_y = fmaxf(0.001f, ay);
        d.by_ax2.c = d.alpha_x * d.alpha_x; d.by_ax2.y = 0.0f;
        d.by_ay2.c = d.alpha_y * d.alpha_y; d.by_ay2.y = 0.0f;
        return d;
    }
    TRC_DEV float ax() const { return alpha_x; }
    TRC_DEV float ay() const { return alpha_y; }

    // Beckmann::lambda / TrowbridgeReitzD::lambda.  Shared: sin_theta, phi_of, ONE quotient (sin / cos for Beckmann's tan_theta,
    // sin^2 / cos^2 for Trowbridge-Reitz's tan2_theta, each with its own zero tests) and ONE square root (of each family's operand)
    TRC_DEV float lambda(F3 w) const {
        const float st = sin_theta(w);
        const Phi ph = phi_of(w, st);
        const float zz = w.z * w.z;
        const float temp = 1 - zz;
        const float num = tr ? temp : st, den = tr ? zz : w.z;
        const float t = (temp <= 0.0f || den == 0.0f) ? 0.0f : num / den;       // tan2_theta(w) | tan_theta_st(w, st)
        const float x = tr ? 1 + (sqr(ph.c * ax()) + sqr(ph.s * ay())) * t
                           : (ph.c * ph.c) * ax() * ax() + (ph.s * ph.s) * ay() * ay();
        const float r = sqrt_cr(x);
        if (is_inf(t)) return 0.;                     // is_inf(tan2Theta) | is_inf(fabsf(tanTheta))
        if (tr) return 0.5f * (r - 1);
        float a = rcp1(r * fabsf(t));
        if (a >= 1.6f) return 0;
        return (1 - 1.259f * a + 0.396f * a * a) / (3.535f * a + 2.181f * a * a);
    }
    TRC_DEV float D(F3 wh) const {
        float tan2Theta = tan2_theta(wh);
        if (is_inf(tan2Theta)) return 0.;
        const float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
        if (tr && cos4Theta < 1e-16f) return 0;
        const Phi ph = phi_of(wh);
        float qc, qs;                                     // cos2_phi / (ax * ax), sin2_phi / (ay * ay)
        div_const2(ph.c * ph.c, by_ax2, ph.s * ph.s, by_ay2, qc, qs);
        if (tr) {
            float e = (qc + qs) * tan2Theta;
            return rcp1(kPi * ax() * ay() * sqr(1 + e) * cos4Theta);
        }
        return dm_expf(-tan2Theta * (qc + qs)) /
               (kPi * ax() * ay() * cos4Theta);
    }
    // D with the two quotients as the divisions the reference writes, correctly rounded: for any roughness pair (DivConst's pairs are
    // each tested exact against this form, so a lobe of the literals gives D's bits)
    TRC_DEV float D_general(F3 wh) const {
        float tan2Theta = tan2_theta(wh);
        if (is_inf(tan2Theta)) return 0.;
        const float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
        if (tr && cos4Theta < 1e-16f) return 0;
        const Phi ph = phi_of(wh);
        const float qc = (ph.c * ph.c) / by_ax2.c, qs = (ph.s * ph.s) / by_ay2.c;
        if (tr) {
            float e = (qc + qs) * tan2Theta;
            return rcp1(kPi * ax() * ay() * sqr(1 + e) * cos4Theta);
        }
        return dm_expf(-tan2Theta * (qc + qs)) /
               (kPi * ax() * ay() * cos4Theta);
    }

    // returns how the lane left (kS11Corner ... kS11ClosedForm); ONCE != 0: sample11_once above
    template <int ONCE = 0, int CAP = 10>
    TRC_DEV int sample11(float cosTheta, float sinTheta, float U1, float U2, float& slope_x, float& slope_y) const {
        if constexpr (ONCE != 0) return sample11_once<ONCE, CAP>(tr, cosTheta, sinTheta, U1, U2, slope_x, slope_y);
        if (cosTheta > .9999f) {
            float r2;                                     // each family's own radius, one root
            if (tr) r2 = U1 / (1 - U1);
            else r2 = -dm_logf(1.0f - U1);
            float r = sqrt_cr(r2);
            const float phi = tr ? 6.28318530718f * U2 : 2 * kPi * U2;      // each family's own literal
            float s, c;
            dm_sincosf(phi, &s, &c);
            slope_x = r * c;
            slope_y = r * s;
            return kS11Corner;
        }
        const float tanTheta = sinTheta / cosTheta;
        const float cotTheta = rcp1(tanTheta);
        if (tr) {                                         // TrowbridgeReitzD::sample11: the closed form
            const float a = cotTheta;
            float G1 = 2 * rcp1(1 + sqrt_cr(1.f + rcp1(a * a)));
            float A = 2 * U1 / G1 - 1;
            float tmp = rcp1(A * A - 1.f);
            if (tmp > 1e10f) tmp = 1e10f;
            float B = tanTheta;
            float D = sqrt_cr(fmaxf(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
            float slope_x_1 = B * tmp - D;
            float slope_x_2 = B * tmp + D;
            slope_x = (A < 0 || slope_x_2 > a) ? slope_x_1 : slope_x_2;
            float S;
            if (U2 > 0.5f) { S = 1.f; U2 = 2.f * (U2 - .5f); }
            else { S = -1.f; U2 = 2.f * (.5f - U2); }
            float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
                      (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
            slope_y = S * z * sqrt_cr(1.f + slope_x * slope_x);
            return kS11ClosedForm;
        }
        const float tanThetaI = tanTheta, cotThetaI = cotTheta, cosThetaI = cosTheta;      // Beckmann::sample11: the Newton iteration
        float a = -1, c = erf_approx(cotThetaI);
        float sample_x = fmaxf(U1, 1e-6f);
        float thetaI = dm_acosf(cosThetaI);
        float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
        const float base = 1 - sample_x;
        const float pw = dm_expf_fin(fit * dm_logf_pos(base == 0.0f ? 1.0f : base));
        float b = c - (1 + c) * (base == 0.0f ? 0.0f : pw);
        const float SQRT_PI_INV = 1.f / sqrtf(kPi);
        float normalization = rcp1(1 + c + SQRT_PI_INV * tanThetaI * dm_expf(-cotThetaI * cotThetaI));
        int it = 0;
        while (++it < CAP) {
            if (!(b >= a && b <= c)) b = 0.5f * (a + c);
            float invErf = erf_inv(b);
            float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_expf_fin(-invErf * invErf)) - sample_x;
            float derivative = normalization * (1 - invErf * tanThetaI);
            if (fabsf(value) < 1e-5f) break;
            if (value > 0) c = b; else a = b;
            b -= value / derivative;
        }
        slope_x = erf_inv(b);
        slope_y = erf_inv(2.0f * fmaxf(U2, 1e-6f) - 1.0f);
        return it < CAP ? kS11Break : kS11RanOut;
    }
    template <int ONCE = 0>
    TRC_DEV F3 sample_wh(F3 wo, F2 u) const {
        const bool flip = wo.z < 0;
        const F3 wi = flip ? -wo : wo;
        F3 wiStretched = normalize(f3(ax() * wi.x, ay() * wi.y, wi.z));
        float slope_x, slope_y;
        const float st = sin_theta(wiStretched);
        sample11<ONCE>(cos_theta(wiStretched), st, u.x, u.y, slope_x, slope_y);
        const Phi ph = phi_of(wiStretched, st);
        float tmp = ph.c * slope_x - ph.s * slope_y;
        slope_y = ph.s * slope_x + ph.c * slope_y;
        slope_x = tmp;
        slope_x = ax() * slope_x;
        slope_y = ay() * slope_y;
        F3 wh = normalize(f3(-slope_x, -slope_y, 1.f));
        return flip ? -wh : wh;
    }
};

// beckmann_finish with the family per lane: Metal takes the reflection side of phase (A) -- MicroRefl::S_F's early-outs are the
// ones written there, in its order --, its own Lambda / D tails and the conductor Fresnel term in phase (B), and in phase (C) the
// shared reflection combination with its own statement of the pdf: D G1 |dot(wo, wh) / cos| where Beckmann's is
// D G1 |dot(wo, wh)| / |cos| (another order of operations, not the same bits) -- one quotient serves both.
TRC_DEV F3 microfacet_finish(const Microfacet& d, bool refl, float R, F3 wo, F3 wh, F3& wi_out, float& pdf_out) {
    const float etaA = 1.0f, etaB = 1.5f;
    bool live;                    // got past the early-outs of S_F: pdf_out will be written
    bool pdf_live = false;        // ... with a non-trivial value
    bool f_live = false;          // F reaches its D * G * Fresnel expression
    F3 wi = wi_out, whA = wh, whB = wh;
    float eta = 0, fres_cos = 0, fres_eta = 1.5f;
    // ---- (A)
    if (refl) {
        live = !(dot(wo, wh) <= 0);
        if (live) {
            wi = reflect(wo, wh);
            if (d.tr) wi_out = wi;            // MicroRefl::S_F assigns its wi before the second early-out, beckmann_finish after it
            live = !(wo.z * wi.z <= 0);
        }
        if (live) {
            pdf_live = true;
            const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
            F3 sum = wi + wo;
            f_live = !(cosThetaI == 0 || cosThetaO == 0) && !(sum.x == 0 && sum.y == 0 && sum.z == 0);
            if (f_live) {
                whB = normalize(sum);
                const float d001 = whB.x * 0.0f + whB.y * 0.0f + whB.z * 1.0f;      // Faceforward(wh, (0,0,1))
                const F3 whf = (d001 < 0.f) ? -whB : whB;
                fres_cos = dot(wi, whf);
                fres_eta = 1.5f;
            }
        }
    } else {
        live = !(dot(wo, wh) < 0);
        if (live) live = refract(wo, wh, cos_theta(wo) > 0 ? (etaA / etaB) : (etaB / etaA), wi);
        if (live) {
            eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
            const bool same_side = wo.z * wi.z > 0;
            whA = normalize(wo + wi * eta);
            const bool backfacing = dot(wo, whA) * dot(wi, whA) > 0;               // same truth value for -whA
            pdf_live = !same_side && !backfacing;
            whB = whA;
            if (whB.z < 0) whB = -whB;
            f_live = pdf_live && !(cos_theta(wi) == 0 || cos_theta(wo) == 0);
            fres_cos = dot(wo, whB);
            fres_eta = etaA;
        }
    }
    // ---- (B)
    float D_A = 0, D_B = 0, lam_o = 0, lam_i = 0;
    F3 fres = f3(0);
    if (pdf_live) {
        lam_o = d.lambda(wo);
        D_A = d.D(whA);
        D_B = D_A;
        if (refl && f_live) D_B = d.D(whB);
        if (f_live) {
            lam_i = d.lambda(wi);
            if (d.tr) fres = FrCond::eval(fres_cos);
            else fres = f3(fr_dielectric(fres_cos, fres_eta));
        }
    }
    // ---- (C)
    F3 out = f3(0);
    if (live) {
        wi_out = wi;
        const float G1 = rcp1(1 + lam_o);
        const float G = rcp1(1 + lam_o + lam_i);
        if (refl) {
            const float dwh = dot(wo, wh);
            const float num = d.tr ? dwh : D_A * G1 * fabsf(dwh), den = d.tr ? cos_theta(wo) : abs_cos_theta(wo);
            const float q = num / den;
            const float dist_pdf = d.tr ? D_A * G1 * fabsf(q) : q;
            pdf_out = dist_pdf / (4 * dot(wo, wh));
            if (f_live) {
                const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
                out = f3(R) * D_B * G * fres / (4 * cosThetaI * cosThetaO);
            }
        } else {
            float p = 0;
            if (pdf_live) {
                const float sqrtDenom = dot(wo, whA) + eta * dot(wi, whA);
                const float dwh_dwi = fabsf((eta * eta * dot(wi, whA)) / (sqrtDenom * sqrtDenom));
                const float dist_pdf = D_A * G1 * fabsf(dot(wo, whA)) / abs_cos_theta(wo);
                p = dist_pdf * dwh_dwi;
            }
            pdf_out = p;
            if (f_live) {
                const float cosThetaO = cos_theta(wo), cosThetaI = cos_theta(wi);
                const float sqrtDenom = dot(wo, whB) + eta * dot(wi, whB);
                const float factor = 1;
                out = (f3(1.0f) - fres) * f3(0.98f) *
                      fabsf(D_B * G * eta * eta * fabsf(dot(wi, whB)) * fabsf(dot(wo, whB)) * factor * factor /
                            (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
            }
        }
    }
    return out;
}

// composites (MicrofacetBXDF.h:436-586)
typedef MicroRefl<TrowbridgeReitzD<Alpha_01_02>, FrCond> MetalLobe;       // alpha (0.01, 0.02), R = 1
// Plastic specular: Beckmann (0.01, 0.1), R = 1; Glass: Beckmann (0.01, 0.01), reflection R = kr = 0.98

// material types (Material.hh:18-20) and texture types (Texture.hh:6) by ordinal
constexpr int kMatDiffuse = 0, kMatLambert = 1, kMatPlastic = 3, kMatMetal = 4, kMatGlass = 5, kMatNil = 10;
constexpr int kTexConstant = 0, kTexChecker = 1, kTexImage = 3;

TRC_DEV F3 texture_value(int tex_type, F3 albedo, F2 uv) {           // Texture.hh:17-43
    if (tex_type == kTexChecker) {
        float s, c, s2, c2;
        dm_sincosf(8 * kPi * uv.x, &s, &c);
        dm_sincosf(kPi / 2 + 4 * kPi * uv.y, &s2, &c2);
        float sines = s * c2;
        return albedo * (0.5f * (sines < 0 ? 0.0f : 1.0f) + 0.5f);
    }
    // Constant; Image with a null texture and Noise resolve to albedo (see oracle/oracle.cpp texture_value); an uploaded image
    // is sampled by hit_color<true> (dev_integrator.hpp) before this is reached
    return (tex_type >= 0 && tex_type <= 3) ? albedo : f3(1.0f);
}

// Material::S_F, Material.hh:124-146.  bxPDF must be pre-set to 0 by the caller (B-3).
// Organised by LOBE rather than by material so that lanes of different materials share instructions: the
// cosine lobe serves Lambert and Plastic's diffuse half, the Beckmann sampling serves Plastic's specular half
// and both Glass lobes.  Every lane evaluates exactly the reference's expressions for its own material.
// STREAM: the four microfacet lobes as one stream (TRC_MICROFACET_STREAM above).  The instrumented kernels (STATS) keep the
// branches apart, so that the per-site profile of trc_debug_profile stays what it says.
// ONCE: sample11's text (TRC_SAMPLE11_ONCE above); the instrumented kernels keep the reference's.
template <bool STATS, bool STREAM = (TRC_MICROFACET_STREAM != 0), int ONCE_ARG = TRC_SAMPLE11_ONCE>
TRC_DEV F3 material_S_F(int type, F3 color, F3 wo, F3& wi, F2 uu, float& pdf, TravCounters& cnt) {
    const bool plastic = type == kMatPlastic, glass = type == kMatGlass;
    constexpr int ONCE = STATS ? 0 : ONCE_ARG;
    F3 out = f3(0);
    if constexpr (STREAM && !STATS) {
        const bool metal = type == kMatMetal;
        if (type == kMatLambert || (plastic && uu.x < 0.5f)) {
            F2 u2 = uu;
            if (plastic) u2.x *= 2;
            const float v = Lambert::S_F(wo, wi, u2, pdf);
            out = plastic ? color * (f3(0.35f, 0.12f, 0.48f) * v) : color * f3(v);
        } else if (metal || plastic || glass) {
            const float ratio = 0.25f;
            const bool refl = metal || plastic || uu.x < ratio;
            F2 u2 = uu;
            if (metal) { }                                           // MetalMaterial::S_F hands uu on as it is
            else if (plastic) { u2.x -= 0.5f; u2.x *= 2.0f; }
            else if (refl) u2.x = uu.x / ratio;
            else u2.x = (uu.x - ratio) / (1.0f - ratio);
            const Microfacet d = Microfacet::make_lobe(metal, plastic);
            F3 lobe = f3(0);
            if (wo.z != 0) {
                const F3 wh = d.template sample_wh<ONCE>(wo, u2);
                lobe = microfacet_finish(d, refl, (metal || plastic) ? 1.0f : 0.98f, wo, wh, wi, pdf);
            }
            out = plastic ? color * (f3(0.2f) * lobe) : color * lobe;
        }
        return out;
    }
    if (type == kMatMetal) {
        ProfScope<STATS> scope(cnt, kProfMetal);
        out = color * MetalLobe::S_F(1.0f, wo, wi, uu, pdf);
    } else if (type == kMatLambert || (plastic && uu.x < 0.5f)) {
        ProfScope<STATS> scope(cnt, kProfLambert);
        F2 u2 = uu;
        if (plastic) u2.x *= 2;                                      // PlasticMaterial::S_F, :497-511
        const float v = Lambert::S_F(wo, wi, u2, pdf);
        out = plastic ? color * (f3(0.35f, 0.12f, 0.48f) * v) : color * f3(v);
    } else if (plastic || glass) {
        const float ratio = 0.25f;                                   // GlassMaterial::S_F, :564-573
        const bool refl = plastic || uu.x < ratio;
        F2 u2 = uu;
        if (plastic) { u2.x -= 0.5f; u2.x *= 2.0f; }
        else if (refl) u2.x = uu.x / ratio;
        else u2.x = (uu.x - ratio) / (1.0f - ratio);
        const Beckmann d = Beckmann::make_lobe(plastic);
        F3 lobe = f3(0);
        if (wo.z != 0) {
            F3 wh;
            { ProfScope<STATS> scope(cnt, kProfBeckSample); wh = d.template sample_wh<ONCE>(wo, u2); }
            ProfScope<STATS> scope(cnt, kProfBeckEval);
            lobe = beckmann_finish(d, refl, plastic ? 1.0f : 0.98f, wo, wh, wi, pdf);
        }
        out = plastic ? color * (f3(0.2f) * lobe) : color * lobe;
    }
    return out;
}
TRC_DEV F3 material_S_F(int type, F3 color, F3 wo, F3& wi, F2 uu, float& pdf) {
    TravCounters none;                                                    // STATS = false: nobody touches it, the compiler drops it
    return material_S_F<false>(type, color, wo, wi, uu, pdf, none);
}

// Material::F, Material.hh:77-99 (pdf = bx.PDF, value = color * bx.F)
TRC_DEV F3 material_F(int type, F3 color, F3 wo, F3 wi, F2 uu, float& pdf) {
    const bool plastic = type == kMatPlastic, glass = type == kMatGlass;
    if (type == kMatMetal) {
        pdf = MetalLobe::pdf(wo, wi);
        return color * MetalLobe::F(1.0f, wo, wi);
    }
    if (type == kMatLambert || (plastic && uu.x < 0.5f)) {           // PlasticMaterial::F/PDF, :469-495
        pdf = Lambert::pdf(wo, wi);
        const float v = Lambert::F(wo, wi);
        return plastic ? color * (f3(0.35f, 0.12f, 0.48f) * v) : color * f3(v);
    }
    if (plastic || glass) {                                          // GlassMaterial::F/PDF, :543-562
        const float ratio = 0.25f;
        const Beckmann d = Beckmann::make_lobe(plastic);
        if (plastic || uu.x < ratio) {
            const float p = BeckRefl::pdf(d, wo, wi);
            pdf = plastic ? p : ratio * p;
            const F3 f = BeckRefl::F(d, plastic ? 1.0f : 0.98f, wo, wi);
            return plastic ? color * (f3(0.2f) * f) : color * f;
        }
        pdf = (1 - ratio) * BeckTransGlass::pdf(d, wo, wi);
        return color * BeckTransGlass::F(d, wo, wi);
    }
    pdf = 0;
    return f3(0);
}

// ---------------------------------------------------------------- TRC_FLAG_MATERIAL_PARAMS: the lobes with their parameters read
// What the reference writes as literals in its create*() functions, per material (tracer_abi.h: trc_material_params, 48 bytes = three
// float4): the roughness pair, the dielectric index (Plastic's and Glass's reflection Fresnel term, Glass's etaB; etaA stays 1), Metal's
// eta and k.  The functions below are material_S_F (its stream form) and material_F with those literals replaced by a LobeParams and
// every form that holds for the literals only replaced by the general one, correctly rounded: DivConst's quotients by the divisions
// (Microfacet::D_general), fr_conductor<true> by fr_conductor<false>, the folded etaA / etaB by the quotient.  Each of those shortcuts is
// tested exact against its general form (trc_unary_test, trc_div_by_test), so LobeParams of the literals give the unflagged bits.
// Plastic's kd / ks, Glass's kr / kt = 0.98 and the lobe-pick ratios stay literals.
struct LobeParams { float alpha_x, alpha_y, eta; F3 metal_eta, metal_k; };
// entry `material` of the table, as three 16-byte loads
TRC_DEV LobeParams lobe_params(const float4* table, uint32_t material) {
    const float4* const p = table + 3u * (size_t)material;
    const float4 a = p[0], e = p[1], k = p[2];
    LobeParams lp;
    lp.alpha_x = a.x; lp.alpha_y = a.y; lp.eta = a.z;
    lp.metal_eta = f3(e.x, e.y, e.z); lp.metal_k = f3(k.x, k.y, k.z);
    return lp;
}

// microfacet_finish with the parameters read: etaB and the reflection Fresnel term's index are lp.eta, Metal's Fresnel term is the
// general conductor form over lp.metal_eta / lp.metal_k, D is D_general.  Everything else is microfacet_finish line by line.
TRC_DEV F3 microfacet_finish_params(const Microfacet& d, const LobeParams& lp, bool refl, float R, F3 wo, F3 wh, F3& wi_out, float& pdf_out) {
    const float etaA = 1.0f, etaB = lp.eta;
    bool live;                    // got past the early-outs of S_F: pdf_out will be written
    bool pdf_live = false;        // ... with a non-trivial value
    bool f_live = false;          // F reaches its D * G * Fresnel expression
    F3 wi = wi_out, whA = wh, whB = wh;
    float eta = 0, fres_cos = 0, fres_eta = etaB;
    // ---- (A)
    if (refl) {
        live = !(dot(wo, wh) <= 0);
        if (live) {
            wi = reflect(wo, wh);
            if (d.tr) wi_out = wi;            // MicroRefl::S_F assigns its wi before the second early-out
            live = !(wo.z * wi.z <= 0);
        }
        if (live) {
            pdf_live = true;
            const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
            F3 sum = wi + wo;
            f_live = !(cosThetaI == 0 || cosThetaO == 0) && !(sum.x == 0 && sum.y == 0 && sum.z == 0);
            if (f_live) {
                whB = normalize(sum);
                const float d001 = whB.x * 0.0f + whB.y * 0.0f + whB.z * 1.0f;      // Faceforward(wh, (0,0,1))
                const F3 whf = (d001 < 0.f) ? -whB : whB;
                fres_cos = dot(wi, whf);
                fres_eta = etaB;
            }
        }
    } else {
        live = !(dot(wo, wh) < 0);
        if (live) live = refract(wo, wh, cos_theta(wo) > 0 ? (etaA / etaB) : (etaB / etaA), wi);
        if (live) {
            eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
            const bool same_side = wo.z * wi.z > 0;
            whA = normalize(wo + wi * eta);
            const bool backfacing = dot(wo, whA) * dot(wi, whA) > 0;               // same truth value for -whA
            pdf_live = !same_side && !backfacing;
            whB = whA;
            if (whB.z < 0) whB = -whB;
            f_live = pdf_live && !(cos_theta(wi) == 0 || cos_theta(wo) == 0);
            fres_cos = dot(wo, whB);
            fres_eta = etaA;
        }
    }
    // ---- (B)
    float D_A = 0, D_B = 0, lam_o = 0, lam_i = 0;
    F3 fres = f3(0);
    if (pdf_live) {
        lam_o = d.lambda(wo);
        D_A = d.D_general(whA);
        D_B = D_A;
        if (refl && f_live) D_B = d.D_general(whB);
        if (f_live) {
            lam_i = d.lambda(wi);
            if (d.tr) fres = fr_conductor(fabsf(fres_cos), lp.metal_eta, lp.metal_k);
            else fres = f3(fr_dielectric(fres_cos, fres_eta));
        }
    }
    // ---- (C)
    F3 out = f3(0);
    if (live) {
        wi_out = wi;
        const float G1 = rcp1(1 + lam_o);
        const float G = rcp1(1 + lam_o + lam_i);
        if (refl) {
            const float dwh = dot(wo, wh);
            const float num = d.tr ? dwh : D_A * G1 * fabsf(dwh), den = d.tr ? cos_theta(wo) : abs_cos_theta(wo);
            const float q = num / den;
            const float dist_pdf = d.tr ? D_A * G1 * fabsf(q) : q;
            pdf_out = dist_pdf / (4 * dot(wo, wh));
            if (f_live) {
                const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
                out = f3(R) * D_B * G * fres / (4 * cosThetaI * cosThetaO);
            }
        } else {
            float p = 0;
            if (pdf_live) {
                const float sqrtDenom = dot(wo, whA) + eta * dot(wi, whA);
                const float dwh_dwi = fabsf((eta * eta * dot(wi, whA)) / (sqrtDenom * sqrtDenom));
                const float dist_pdf = D_A * G1 * fabsf(dot(wo, whA)) / abs_cos_theta(wo);
                p = dist_pdf * dwh_dwi;
            }
            pdf_out = p;
            if (f_live) {
                const float cosThetaO = cos_theta(wo), cosThetaI = cos_theta(wi);
                const float sqrtDenom = dot(wo, whB) + eta * dot(wi, whB);
                const float factor = 1;
                out = (f3(1.0f) - fres) * f3(0.98f) *
                      fabsf(D_B * G * eta * eta * fabsf(dot(wi, whB)) * fabsf(dot(wo, whB)) * factor * factor /
                            (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
            }
        }
    }
    return out;
}

// Material::S_F with the parameters read: material_S_F's stream form (one instruction stream for the four microfacet lobes) whatever
// TRC_MICROFACET_STREAM says.  A lane fetches its entry where the lobe is built: a Lambert vertex and Plastic's diffuse half load nothing.
template <int ONCE = TRC_SAMPLE11_ONCE>
TRC_DEV F3 material_S_F_params(int type, F3 color, const float4* table, uint32_t material, F3 wo, F3& wi, F2 uu, float& pdf) {
    const bool plastic = type == kMatPlastic, glass = type == kMatGlass, metal = type == kMatMetal;
    F3 out = f3(0);
    if (type == kMatLambert || (plastic && uu.x < 0.5f)) {
        F2 u2 = uu;
        if (plastic) u2.x *= 2;
        const float v = Lambert::S_F(wo, wi, u2, pdf);
        out = plastic ? color * (f3(0.35f, 0.12f, 0.48f) * v) : color * f3(v);
    } else if (metal || plastic || glass) {
        const float ratio = 0.25f;
        const bool refl = metal || plastic || uu.x < ratio;
        F2 u2 = uu;
        if (metal) { }                                           // MetalMaterial::S_F hands uu on as it is
        else if (plastic) { u2.x -= 0.5f; u2.x *= 2.0f; }
        else if (refl) u2.x = uu.x / ratio;
        else u2.x = (uu.x - ratio) / (1.0f - ratio);
        const LobeParams lp = lobe_params(table, material);
        const Microfacet d = Microfacet::make_lobe(metal, lp.alpha_x, lp.alpha_y);
        F3 lobe = f3(0);
        if (wo.z != 0) {
            const F3 wh = d.template sample_wh<ONCE>(wo, u2);
            lobe = microfacet_finish_params(d, lp, refl, (metal || plastic) ? 1.0f : 0.98f, wo, wh, wi, pdf);
        }
        out = plastic ? color * (f3(0.2f) * lobe) : color * lobe;
    }
    return out;
}

// Material::F with the parameters read (pdf = bx.PDF, value = color * bx.F): MicrofacetReflection over Trowbridge-Reitz with the
// conductor term (Metal), over Beckmann with the dielectric term (Plastic's specular lobe, Glass's reflection lobe) and
// MicrofacetTransmission over Beckmann (Glass), each as material_F's lobes state them, over one Microfacet with the family per lane
TRC_DEV F3 material_F_params(int type, F3 color, const float4* table, uint32_t material, F3 wo, F3 wi, F2 uu, float& pdf) {
    const bool plastic = type == kMatPlastic, glass = type == kMatGlass, metal = type == kMatMetal;
    if (type == kMatLambert || (plastic && uu.x < 0.5f)) {           // PlasticMaterial::F/PDF, :469-495
        pdf = Lambert::pdf(wo, wi);
        const float v = Lambert::F(wo, wi);
        return plastic ? color * (f3(0.35f, 0.12f, 0.48f) * v) : color * f3(v);
    }
    if (!(metal || plastic || glass)) { pdf = 0; return f3(0); }
    const float ratio = 0.25f;
    const LobeParams lp = lobe_params(table, material);
    const Microfacet d = Microfacet::make_lobe(metal, lp.alpha_x, lp.alpha_y);
    if (metal || plastic || uu.x < ratio) {                          // MicrofacetReflection::PDF / F, MicrofacetBXDF.h:15-34, 50-57
        float p = 0;
        if (!(wo.z * wi.z <= 0)) {
            const F3 wh = normalize(wo + wi);
            const float G1 = rcp1(1 + d.lambda(wo));
            const float dist_pdf = metal ? d.D_general(wh) * G1 * fabsf(dot(wo, wh) / cos_theta(wo))
                                         : d.D_general(wh) * G1 * fabsf(dot(wo, wh)) / abs_cos_theta(wo);
            p = dist_pdf / (4 * dot(wo, wh));
        }
        pdf = (metal || plastic) ? p : ratio * p;
        const float R = (metal || plastic) ? 1.0f : 0.98f;
        F3 f = f3(0);
        const float cosThetaO = abs_cos_theta(wo), cosThetaI = abs_cos_theta(wi);
        F3 wh = wi + wo;
        if (!(cosThetaI == 0 || cosThetaO == 0) && !(wh.x == 0 && wh.y == 0 && wh.z == 0)) {
            wh = normalize(wh);
            const float d001 = wh.x * 0.0f + wh.y * 0.0f + wh.z * 1.0f;          // Faceforward(wh, (0,0,1))
            const F3 whf = (d001 < 0.f) ? -wh : wh;
            const float c = dot(wi, whf);
            const F3 Fres = metal ? fr_conductor(fabsf(c), lp.metal_eta, lp.metal_k) : f3(fr_dielectric(c, lp.eta));
            const float G = rcp1(1 + d.lambda(wo) + d.lambda(wi));
            f = f3(R) * d.D_general(wh) * G * Fres / (4 * cosThetaI * cosThetaO);
        }
        return plastic ? color * (f3(0.2f) * f) : color * f;
    }
    // MicrofacetTransmission::PDF / F, :83-115, as GlassMaterial instantiates it: T = 0.98, etaA = 1, etaB = lp.eta, factor 1
    const float etaA = 1.0f, etaB = lp.eta;
    const float eta = cos_theta(wo) > 0 ? (etaB / etaA) : (etaA / etaB);
    float p = 0;
    if (!(wo.z * wi.z > 0)) {
        const F3 wh = normalize(wo + wi * eta);
        if (!(dot(wo, wh) * dot(wi, wh) > 0)) {
            const float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
            const float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrtDenom * sqrtDenom));
            const float dist_pdf = d.D_general(wh) * rcp1(1 + d.lambda(wo)) * fabsf(dot(wo, wh)) / abs_cos_theta(wo);
            p = dist_pdf * dwh_dwi;
        }
    }
    pdf = (1 - ratio) * p;
    F3 f = f3(0);
    const float cosThetaO = cos_theta(wo), cosThetaI = cos_theta(wi);
    if (!(wo.z * wi.z > 0) && !(cosThetaI == 0 || cosThetaO == 0)) {
        F3 wh = normalize(wo + wi * eta);
        if (wh.z < 0) wh = -wh;
        if (!(dot(wo, wh) * dot(wi, wh) > 0)) {
            const F3 Fres = f3(fr_dielectric(dot(wo, wh), etaA));
            const float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
            const float factor = 1;
            const float G = rcp1(1 + d.lambda(wo) + d.lambda(wi));
            f = (f3(1.0f) - Fres) * f3(0.98f) *
                fabsf(d.D_general(wh) * G * eta * eta * fabsf(dot(wi, wh)) * fabsf(dot(wo, wh)) * factor * factor /
                      (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
        }
    }
    return color * f;
}

}  // namespace trcdev
