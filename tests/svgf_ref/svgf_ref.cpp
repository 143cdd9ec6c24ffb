// svgf_ref.cpp -- scalar CPU restatement of the SVGF stage as include/tracer_abi.h states it ("SVGF denoiser", steps 1-5),
// written from that statement, not from the kernels.  Compiled by tests/test_svgf_ref.py and tests/test_gpu_denoise.py with
//   g++ -O2 -ffp-contract=off -Iinclude -shared -fPIC
// so that every operation is one binary32 IEEE operation in the order written (division and sqrt correctly rounded, exp from
// trc_detmath.h): the device output must equal this bit for bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "tracer_abi.h"
#include "trc_detmath.h"

namespace {

struct V3 { float x, y, z; };
V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 at(const float* p) { return {p[0], p[1], p[2]}; }

float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
bool hit(const trc_gbuffer_texel& t) { return t.id != TRC_GBUFFER_MISS; }

uint32_t squarings(uint32_t e) { uint32_t k = 0; while ((1u << k) < e) ++k; return k; }
float w8(float x, uint32_t nsq) { for (uint32_t k = 0; k < nsq; ++k) x = x * x; return x; }
float normal_w(const trc_gbuffer_texel& a, const trc_gbuffer_texel& b, uint32_t nsq) {
    float d = a.normal[0] * b.normal[0] + a.normal[1] * b.normal[1] + a.normal[2] * b.normal[2];
    return w8(d > 0.0f ? d : 0.0f, nsq);
}

struct Frame {
    const trc_denoise_params* p;
    int W, H;
    uint32_t nsq;
    bool demod;
    const trc_gbuffer_texel* g;
    const trc_gbuffer_texel& G(int x, int y) const { return g[(size_t)y * W + x]; }
    bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < W && y < H; }
    // step 1: the (demodulated) input colour
    void input(const float* accum, int x, int y, float c[3]) const {
        const float* a = accum + 4 * ((size_t)y * W + x);
        for (int k = 0; k < 3; ++k) {
            c[k] = a[k];
            if (demod) { const float al = G(x, y).albedo[k]; c[k] = c[k] / (al > TRC_DENOISE_ALBEDO_EPS ? al : TRC_DENOISE_ALBEDO_EPS); }
        }
    }
    // depth gradient stencil of step 3
    void grad(int x, int y, float& gx, float& gy) const {
        const float z = G(x, y).depth;
        auto one = [&](int ax, int ay, int bx, int by) {
            float best = INFINITY;
            if (inside(ax, ay) && hit(G(ax, ay))) best = fabsf(G(ax, ay).depth - z);
            if (inside(bx, by) && hit(G(bx, by))) { const float d = fabsf(G(bx, by).depth - z); if (d < best) best = d; }
            return best == INFINITY ? 0.0f : best;
        };
        gx = one(x + 1, y, x - 1, y);
        gy = one(x, y + 1, x, y - 1);
    }
    float depth_den(int x, int y, float gx, float gy, int ox, int oy) const {
        return p->sigma_z * (gx * fabsf((float)ox) + gy * fabsf((float)oy)) + 0.001f * G(x, y).depth;
    }
};

}  // namespace

extern "C" {

float svgf_ref_normal_weight(float d, uint32_t exponent) { return w8(d > 0.0f ? d : 0.0f, squarings(exponent)); }

// One trc_denoise.  cam / prev_cam: 12 floats (lookFrom, horizontal, vertical, cornerLowLeft); prev_cam == NULL: no history.
// g / g_prev: this frame's and the previous frame's G-buffer; every plane W*H float4.  Outputs: integ = (colour, variance) of
// the temporal pass, hist_col_out / hist_mom_out = the history the next frame reads, out = the denoised RGBA frame.
int svgf_ref_frame(const trc_denoise_params* p, uint32_t Wu, uint32_t Hu, const float* cam, const float* prev_cam,
                   const trc_gbuffer_texel* g, const trc_gbuffer_texel* g_prev, const float* accum, const float* hist_col,
                   const float* hist_mom, float* integ, float* hist_col_out, float* hist_mom_out, float* out) {
    Frame f{p, (int)Wu, (int)Hu, squarings(p->normal_exponent), (p->flags & TRC_DENOISE_DEMODULATE) != 0, g};
    const int W = f.W, H = f.H;
    const size_t n = (size_t)W * H;
    const bool same = prev_cam && memcmp(cam, prev_cam, 12 * sizeof(float)) == 0;

    // steps 1-3
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const trc_gbuffer_texel& t = g[i];
            const float* a = accum + 4 * i;
            if (!hit(t)) {
                const float L = luminance(a[0], a[1], a[2]);
                const float I[4] = {a[0], a[1], a[2], 0.0f}, M[4] = {L, L * L, 1.0f, 0.0f};
                memcpy(integ + 4 * i, I, 16); memcpy(hist_mom_out + 4 * i, M, 16);
                continue;
            }
            float c[3];
            f.input(accum, x, y, c);
            const float L = luminance(c[0], c[1], c[2]);
            float W_ = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, M1 = 0.0f, M2 = 0.0f, N = 0.0f;
            if (prev_cam) {
                int tx[4], ty[4], nt = 0;
                float tw[4], zq = t.depth;
                if (same) {
                    tx[0] = x; ty[0] = y; tw[0] = 1.0f; nt = 1;
                } else {
                    const float u = (float)x / (float)W, v = (float)y / (float)H;
                    const V3 eye = at(cam);
                    const V3 dir = sub(add(add(at(cam + 9), mul(at(cam + 3), u)), mul(at(cam + 6), v)), eye);
                    const V3 d = mul(dir, 1.0f / sqrtf(dot(dir, dir)));
                    const V3 P = add(eye, mul(d, t.depth));
                    const V3 pe = at(prev_cam), ph = at(prev_cam + 3), pv = at(prev_cam + 6);
                    const V3 q = sub(P, pe), av = sub(at(prev_cam + 9), pe), m = cross(ph, pv);
                    const float s = dot(av, m) / dot(q, m);
                    const float pu = (dot(q, ph) * s - dot(av, ph)) / dot(ph, ph);
                    const float pvv = (dot(q, pv) * s - dot(av, pv)) / dot(pv, pv);
                    const float px = pu * (float)W, py = pvv * (float)H;
                    zq = sqrtf(dot(q, q));
                    if (s > 0.0f && s < INFINITY && px > -1.0f && px < (float)W && py > -1.0f && py < (float)H) {
                        const float x0 = floorf(px), y0 = floorf(py), fx = px - x0, fy = py - y0;
                        const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                        for (int k = 0; k < 4; ++k) { tx[k] = (int)x0 + (k & 1); ty[k] = (int)y0 + (k >> 1); tw[k] = wx[k & 1] * wy[k >> 1]; }
                        nt = 4;
                    }
                }
                for (int k = 0; k < nt; ++k) {
                    if (!f.inside(tx[k], ty[k])) continue;
                    const size_t j = (size_t)ty[k] * W + tx[k];
                    const trc_gbuffer_texel& o = g_prev[j];
                    if (o.id != t.id) continue;
                    if (!(fabsf(o.depth - zq) <= 0.1f * zq)) continue;
                    if (!(t.normal[0] * o.normal[0] + t.normal[1] * o.normal[1] + t.normal[2] * o.normal[2] >= 0.9f)) continue;
                    const float w = tw[k];
                    W_ += w;
                    for (int ch = 0; ch < 3; ++ch) C[ch] += w * hist_col[4 * j + ch];
                    M1 += w * hist_mom[4 * j]; M2 += w * hist_mom[4 * j + 1]; N += w * hist_mom[4 * j + 2];
                }
            }
            float col[3], mu1, mu2, hl;
            if (W_ >= 0.01f) {
                hl = N / W_ + 1.0f;
                if (hl > 64.0f) hl = 64.0f;
                const float inv = 1.0f / hl;
                const float ac = inv > p->alpha_color ? inv : p->alpha_color, am = inv > p->alpha_moments ? inv : p->alpha_moments;
                for (int ch = 0; ch < 3; ++ch) { const float prev = C[ch] / W_; col[ch] = prev + (c[ch] - prev) * ac; }
                const float m1 = M1 / W_, m2 = M2 / W_;
                mu1 = m1 + (L - m1) * am;
                mu2 = m2 + (L * L - m2) * am;
            } else {
                hl = 1.0f;
                for (int ch = 0; ch < 3; ++ch) col[ch] = c[ch];
                mu1 = L; mu2 = L * L;
            }
            float var;
            if (hl >= (float)p->min_history) {
                var = mu2 - mu1 * mu1;
                if (!(var > 0.0f)) var = 0.0f;
            } else {
                float gx, gy;
                f.grad(x, y, gx, gy);
                float ws = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -3; dx <= 3; ++dx) {
                        const int xx = x + dx, yy = y + dy;
                        if (!f.inside(xx, yy) || !hit(f.G(xx, yy))) continue;
                        float qc[3];
                        f.input(accum, xx, yy, qc);
                        const float Lq = luminance(qc[0], qc[1], qc[2]);
                        const float w = dm_expf(-(fabsf(t.depth - f.G(xx, yy).depth) / f.depth_den(x, y, gx, gy, dx, dy))) * normal_w(t, f.G(xx, yy), f.nsq);
                        ws += w; s1 += w * Lq; s2 += w * (Lq * Lq);
                    }
                var = 0.0f;
                if (ws > 0.0f) {
                    const float m1 = s1 / ws;
                    var = s2 / ws - m1 * m1;
                    if (!(var > 0.0f)) var = 0.0f;
                }
            }
            const float I[4] = {col[0], col[1], col[2], var}, M[4] = {mu1, mu2, hl, 0.0f};
            memcpy(integ + 4 * i, I, 16); memcpy(hist_mom_out + 4 * i, M, 16);
        }

    // step 4
    std::vector<float> cur(integ, integ + 4 * n), next(4 * n);
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}, gk[3] = {0.25f, 0.5f, 0.25f};
    if (p->iterations == 0) memcpy(hist_col_out, integ, 16 * n);
    for (uint32_t it = 0; it < p->iterations; ++it) {
        const int step = 1 << it;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                const trc_gbuffer_texel& t = g[i];
                if (!hit(t)) { memcpy(&next[4 * i], &cur[4 * i], 16); continue; }
                float gx, gy;
                f.grad(x, y, gx, gy);
                float sg = 0.0f, sv = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!f.inside(x + dx, y + dy) || !hit(f.G(x + dx, y + dy))) continue;
                        const float gw = gk[dy + 1] * gk[dx + 1];
                        sg += gw; sv += gw * cur[4 * ((size_t)(y + dy) * W + x + dx) + 3];
                    }
                const float vf = sv / sg;
                const float phi = p->sigma_l * sqrtf(vf > 0.0f ? vf : 0.0f) + 1e-10f;
                const float L = luminance(cur[4 * i], cur[4 * i + 1], cur[4 * i + 2]);
                float ws = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, V = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int xx = x + dx * step, yy = y + dy * step;
                        if (!f.inside(xx, yy) || !hit(f.G(xx, yy))) continue;
                        const float* q = &cur[4 * ((size_t)yy * W + xx)];
                        const float wz = fabsf(t.depth - f.G(xx, yy).depth) / f.depth_den(x, y, gx, gy, dx * step, dy * step);
                        const float wl = fabsf(L - luminance(q[0], q[1], q[2])) / phi;
                        const float w = ((hk[dx + 2] * hk[dy + 2]) * normal_w(t, f.G(xx, yy), f.nsq)) * dm_expf(-(wz + wl));
                        ws += w;
                        for (int ch = 0; ch < 3; ++ch) C[ch] += w * (q[ch] - cur[4 * i + ch]);
                        V += (w * w) * q[3];
                    }
                if (ws > 0.0f) {
                    for (int ch = 0; ch < 3; ++ch) next[4 * i + ch] = cur[4 * i + ch] + C[ch] / ws;
                    next[4 * i + 3] = V / (ws * ws);
                } else {
                    memcpy(&next[4 * i], &cur[4 * i], 16);
                }
            }
        cur.swap(next);
        if (it == 0) memcpy(hist_col_out, cur.data(), 16 * n);
    }

    // step 5
    for (size_t i = 0; i < n; ++i) {
        const float* a = accum + 4 * i;
        if (!hit(g[i])) { memcpy(out + 4 * i, a, 16); continue; }
        for (int ch = 0; ch < 3; ++ch) {
            float c = cur[4 * i + ch];
            if (f.demod) { const float al = g[i].albedo[ch]; c = c * (al > TRC_DENOISE_ALBEDO_EPS ? al : TRC_DENOISE_ALBEDO_EPS); }
            out[4 * i + ch] = c;
        }
        out[4 * i + 3] = a[3];
    }
    return 0;
}

}  // extern "C"
