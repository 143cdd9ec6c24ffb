// dev_envlight.hpp -- the environment map as a light of traceMIS (TRC_FLAG_ENV_LIGHT, tracer_abi.h): importance sampling of the
// map's cells by a two-level alias table and the solid-angle pdf of a direction.  An extension beyond the reference, which lights
// with the map only where a BSDF-sampled ray escapes (Render.metal:300-305).  The tables are built by trc_envlight.hip;
// tests/envlight_ref restates every function here on the CPU (trc_detmath.h: the same bits).
#pragma once

#include "dev_vec.hpp"
#include "trc_detmath.h"

namespace trcdev {

constexpr float kEnvTwoPi = 6.28318530717958647692f;
constexpr float kEnvInvTwoPi = 0.159154943091895335769f;
constexpr float kEnvInvPi = 0.318309886183790671538f;
constexpr float kEnvTwoPiSq = 19.7392088021787172376f;     // 2 pi^2: d(omega) = 2 pi^2 cos(lat) du dw

// The tables of one map (W x H cells, row j at w in [j/H, (j+1)/H), rows bottom-up like the map's).  rows: per row, W entries
// {accept threshold, alias} of the row's alias table; marg: H entries of the table over rows.  An entry is kept when a 32-bit
// draw is below its threshold (an entry of probability 1 has threshold 2^32 - 1 and is its own alias).  scale = W H / total
// weight, so that weight * scale is the density in (u, w); 0 when the total is 0.
struct EnvLight {
    const uint2* rows;
    const uint2* marg;
    const float* weight;
    uint32_t w, h;
    float scale;
    float p_env;              // probability of picking the map in the light pick (1/2 with square lights, 1 without, 0 for a black map)
    uint32_t squares;         // the scene has squareList[5] and [6]
};

// (u, w) in [0, 1]^2 -> direction: phi = 2 pi (u - 1/2), latitude = pi (w - 1/2)
TRC_DEV F3 env_uw_dir(float u, float w, float& cos_lat) {
    float sp, cp, sl, cl;
    dm_sincosf(kEnvTwoPi * (u - 0.5f), &sp, &cp);
    dm_sincosf(kPi * (w - 0.5f), &sl, &cl);
    cos_lat = cl;
    return f3(cl * cp, sl, cl * sp);
}
TRC_DEV float env_cell_pdf(const EnvLight& L, uint32_t i, uint32_t j, float cos_lat) {
    const float p_uw = L.weight[(size_t)j * L.w + i] * L.scale;
    return cos_lat > 0.0f ? p_uw / (kEnvTwoPiSq * cos_lat) : 0.0f;
}
// One sample: r0 / r1 pick the row (multiply-shift index, alias decision), r2 / r3 the cell in it, f0 / f1 in [0, 1] the point
// inside the cell.  pdf = solid-angle density of the direction (0 at the poles).
TRC_DEV F3 env_light_sample(const EnvLight& L, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, float f0, float f1, float& pdf) {
    uint32_t j = (uint32_t)(((uint64_t)r0 * L.h) >> 32);
    const uint2 m = L.marg[j];
    if (r1 >= m.x) j = m.y;
    uint32_t i = (uint32_t)(((uint64_t)r2 * L.w) >> 32);
    const uint2 a = L.rows[(size_t)j * L.w + i];
    if (r3 >= a.x) i = a.y;
    const float u = ((float)i + f0) / (float)L.w, w = ((float)j + f1) / (float)L.h;
    float cl;
    const F3 dir = env_uw_dir(u, w, cl);
    pdf = env_cell_pdf(L, i, j, cl);
    return dir;
}
// The solid-angle density env_light_sample gives direction d (any length; 0 for a non-finite one, at the poles and for a black map)
TRC_DEV float env_light_pdf(const EnvLight& L, F3 d) {
    if (!(L.scale > 0.0f)) return 0.0f;
    const F3 v = normalize(d);
    if (is_nan(v.x) || is_nan(v.y) || is_nan(v.z)) return 0.0f;
    const float u = dm_atan2f(v.z, v.x) * kEnvInvTwoPi + 0.5f;
    const float w = dm_asinf(fminf(fmaxf(v.y, -1.0f), 1.0f)) * kEnvInvPi + 0.5f;
    auto cell = [](float x, uint32_t n) { const float f = floorf(x * (float)n); return f < 0.0f ? 0u : (f > (float)(n - 1) ? n - 1 : (uint32_t)f); };
    const uint32_t i = cell(u, L.w), j = cell(w, L.h);
    return env_cell_pdf(L, i, j, sqrt_cr(v.x * v.x + v.z * v.z));
}
// power heuristic f^2 / (f^2 + g^2) (Sampling.hh:137-140) written so that a huge f (a squared glass pdf) cannot make inf / inf:
// 1 when g == 0, 0 when f == 0
TRC_DEV float env_mis_weight(float f, float g) {
    if (!(g > 0.0f)) return 1.0f;
    if (!(f > 0.0f)) return 0.0f;
    const float r = g / f;
    return 1.0f / (1.0f + r * r);
}

}  // namespace trcdev
