// envlight_ref.cpp -- CPU restatement of the environment map as a light (TRC_FLAG_ENV_LIGHT, include/tracer_abi.h): the cell
// weights, Vose's alias tables in their stated order, the sampler and the pdf of tracer_amd/csrc/dev_envlight.hpp and
// trc_envlight.hip, written again from the statement with trc_detmath.h's elementary functions (the same bits as the kernels').
// Built into the oracle library (oracle/Makefile, -ffp-contract=off), where the oracle's traceMISLight and envlight_loader.py find it.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "trc_detmath.h"

namespace {
const float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f;
const float kInvTwoPi = 0.159154943091895335769f, kInvPi = 0.318309886183790671538f, kTwoPiSq = 19.7392088021787172376f;

uint32_t threshold(double q) { return q >= 1.0 ? 0xFFFFFFFFu : (q <= 0.0 ? 0u : (uint32_t)(q * 4294967296.0)); }

template <class T>
void vose(const T* w, uint32_t n, double sum, uint32_t* out /* 2 n */) {
    std::vector<double> q(n);
    for (uint32_t i = 0; i < n; ++i) q[i] = sum > 0.0 ? ((double)w[i] * (double)n) / sum : 1.0;
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

struct Tables { uint32_t w, h; const float* weight; const uint32_t* rows; const uint32_t* marg; float scale; };

float cell_pdf(const Tables& L, uint32_t i, uint32_t j, float cl) {
    const float p_uw = L.weight[(size_t)j * L.w + i] * L.scale;
    return cl > 0.0f ? p_uw / (kTwoPiSq * cl) : 0.0f;
}
}  // namespace

extern "C" {
// weights (W*H), rows (2*W*H), marg (2*H), total; rgb = 3*W*H floats, rows bottom-up
void envlight_ref_tables(const float* rgb, uint32_t W, uint32_t H, float* weight, uint32_t* rows, uint32_t* marg, double* total) {
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            float m = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    int y = (int)j + dy, x = (int)i + dx;
                    y = y < 0 ? 0 : (y > (int)H - 1 ? (int)H - 1 : y);
                    x = x < 0 ? 0 : (x > (int)W - 1 ? (int)W - 1 : x);
                    const float* t = rgb + 3 * ((size_t)y * W + x);
                    float lum = 0.212671f * t[0] + 0.715160f * t[1] + 0.072169f * t[2];
                    if (!(lum > 0.0f && lum <= FLT_MAX)) lum = 0.0f;
                    m = std::fmax(m, lum);
                }
            const float cl = dm_cosf(kPi * (((float)j + 0.5f) / (float)H - 0.5f));
            weight[(size_t)j * W + i] = m * std::fmax(cl, 0.0f);
        }
    std::vector<double> rowsum(H);
    for (uint32_t j = 0; j < H; ++j) {
        double s = 0.0;
        for (uint32_t i = 0; i < W; ++i) s += (double)weight[(size_t)j * W + i];
        rowsum[j] = s;
        vose(weight + (size_t)j * W, W, s, rows + 2 * (size_t)j * W);
    }
    double t = 0.0;
    for (uint32_t j = 0; j < H; ++j) t += rowsum[j];
    *total = t;
    vose(rowsum.data(), H, t, marg);
}

float envlight_ref_scale(uint32_t W, uint32_t H, double total) { return total > 0.0 ? (float)((double)W * (double)H / total) : 0.0f; }

// draws: 6 words per item (4 integer draws, 2 float bit patterns) -> dir_pdf 4 floats per item
void envlight_ref_sample(uint32_t W, uint32_t H, const float* weight, const uint32_t* rows, const uint32_t* marg, double total,
                         const uint32_t* draws, size_t n, float* dir_pdf) {
    const Tables L{W, H, weight, rows, marg, envlight_ref_scale(W, H, total)};
    for (size_t k = 0; k < n; ++k) {
        const uint32_t* d = draws + 6 * k;
        uint32_t j = (uint32_t)(((uint64_t)d[0] * H) >> 32);
        if (d[1] >= marg[2 * j]) j = marg[2 * j + 1];
        uint32_t i = (uint32_t)(((uint64_t)d[2] * W) >> 32);
        const uint32_t* a = rows + 2 * ((size_t)j * W + i);
        if (d[3] >= a[0]) i = a[1];
        float f0, f1;
        std::memcpy(&f0, d + 4, 4); std::memcpy(&f1, d + 5, 4);
        const float u = ((float)i + f0) / (float)W, w = ((float)j + f1) / (float)H;
        float sp, cp, sl, cl;
        dm_sincosf(kTwoPi * (u - 0.5f), &sp, &cp);
        dm_sincosf(kPi * (w - 0.5f), &sl, &cl);
        float* o = dir_pdf + 4 * k;
        o[0] = cl * cp; o[1] = sl; o[2] = cl * sp;
        o[3] = cell_pdf(L, i, j, cl);
    }
}

// dirs: 3 floats per direction -> pdf
void envlight_ref_pdf(uint32_t W, uint32_t H, const float* weight, double total, const float* dirs, size_t m, float* pdf) {
    const Tables L{W, H, weight, nullptr, nullptr, envlight_ref_scale(W, H, total)};
    for (size_t k = 0; k < m; ++k) {
        if (!(L.scale > 0.0f)) { pdf[k] = 0.0f; continue; }
        const float* d = dirs + 3 * k;
        const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const float vx = d[0] * inv, vy = d[1] * inv, vz = d[2] * inv;
        if (vx != vx || vy != vy || vz != vz) { pdf[k] = 0.0f; continue; }
        const float u = dm_atan2f(vz, vx) * kInvTwoPi + 0.5f;
        const float w = dm_asinf(std::fmin(std::fmax(vy, -1.0f), 1.0f)) * kInvPi + 0.5f;
        auto cell = [](float x, uint32_t n) { const float f = floorf(x * (float)n); return f < 0.0f ? 0u : (f > (float)(n - 1) ? n - 1 : (uint32_t)f); };
        pdf[k] = cell_pdf(L, cell(u, W), cell(w, H), sqrtf(vx * vx + vz * vz));
    }
}
}  // extern "C"
