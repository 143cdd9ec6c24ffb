// svgf_motion_ref.cpp -- scalar CPU restatement of the SVGF stage WITH motion tracking, as include/tracer_abi.h states it: "SVGF
// denoiser" steps 1-5 and the amendment of step 2 under "Motion tracking".  Written from that text, not from the kernels and not from
// tests/svgf_ref/svgf_ref.cpp (which restates the stage without the amendment and stays as it is: with an all-zero motion plane the two
// must agree bit for bit, tests/test_svgf_motion_ref.py).  The motion plane is an INPUT here: what writes it is restated in
// tests/motion_ref.py.  Compiled with
//   g++ -O2 -ffp-contract=off -Iinclude -shared -fPIC
// so that every operation is one binary32 IEEE operation in the order written.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "tracer_abi.h"
#include "trc_detmath.h"

namespace {

struct Vec { float x, y, z; };
Vec operator+(Vec a, Vec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
Vec operator-(Vec a, Vec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
Vec operator*(Vec a, float s) { return {a.x * s, a.y * s, a.z * s}; }
float dot(Vec a, Vec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
Vec cross(Vec a, Vec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
Vec load(const float* p) { return {p[0], p[1], p[2]}; }

struct Camera {                       // the four vectors the filter reads, in the order the tests pass them
    Vec eye, hor, ver, cll;
    explicit Camera(const float* c) : eye(load(c)), hor(load(c + 3)), ver(load(c + 6)), cll(load(c + 9)) {}
};

float L(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
float max0(float v) { return v > 0.0f ? v : 0.0f; }

struct Stage {
    const trc_denoise_params& prm;
    int W, H;
    const trc_gbuffer_texel* gb;
    const float* accum;
    uint32_t squarings;
    bool demod;

    Stage(const trc_denoise_params& p, int w, int h, const trc_gbuffer_texel* g, const float* a)
        : prm(p), W(w), H(h), gb(g), accum(a), squarings(0), demod((p.flags & TRC_DENOISE_DEMODULATE) != 0) {
        while ((1u << squarings) < p.normal_exponent) ++squarings;
    }
    size_t at(int x, int y) const { return (size_t)y * W + x; }
    bool in(int x, int y) const { return 0 <= x && x < W && 0 <= y && y < H; }
    bool is_hit(int x, int y) const { return gb[at(x, y)].id != TRC_GBUFFER_MISS; }
    bool tap(int x, int y) const { return in(x, y) && is_hit(x, y); }      // "in-bounds hit taps only"
    float albedo(size_t i, int ch) const { const float a = gb[i].albedo[ch]; return a > TRC_DENOISE_ALBEDO_EPS ? a : TRC_DENOISE_ALBEDO_EPS; }
    // step 1
    void input(int x, int y, float c[3]) const {
        const size_t i = at(x, y);
        for (int ch = 0; ch < 3; ++ch) c[ch] = demod ? accum[4 * i + ch] / albedo(i, ch) : accum[4 * i + ch];
    }
    float w8(const trc_gbuffer_texel& a, const trc_gbuffer_texel& b) const {
        float w = max0(a.normal[0] * b.normal[0] + a.normal[1] * b.normal[1] + a.normal[2] * b.normal[2]);
        for (uint32_t k = 0; k < squarings; ++k) w = w * w;
        return w;
    }
    // the depth gradient stencil of step 3, along one axis
    float gradient(int x, int y, int ax, int ay) const {
        const float z = gb[at(x, y)].depth;
        float m = INFINITY;
        if (tap(x + ax, y + ay)) m = fabsf(gb[at(x + ax, y + ay)].depth - z);
        if (tap(x - ax, y - ay)) m = fminf(m, fabsf(gb[at(x - ax, y - ay)].depth - z));
        return m == INFINITY ? 0.0f : m;
    }
    float D(float z, float gx, float gy, int ox, int oy) const { return prm.sigma_z * (gx * fabsf((float)ox) + gy * fabsf((float)oy)) + 0.001f * z; }
};

}  // namespace

extern "C" {

// One trc_denoise with tracking on.  cam / prev_cam: 12 floats (lookFrom, horizontal, vertical, cornerLowLeft); prev_cam == NULL: no
// history.  motion: W*H texels (NULL: all zero, no snapshot in force).  Every other plane W*H float4, as in svgf_ref_frame.
int svgf_motion_ref_frame(const trc_denoise_params* p, uint32_t Wu, uint32_t Hu, const float* cam_f, const float* prev_cam_f,
                          const trc_gbuffer_texel* g, const trc_gbuffer_texel* g_prev, const trc_motion_texel* motion, const float* accum,
                          const float* hist_col, const float* hist_mom, float* integ, float* hist_col_out, float* hist_mom_out, float* out) {
    const Stage st(*p, (int)Wu, (int)Hu, g, accum);
    const int W = st.W, H = st.H;
    const size_t n_px = (size_t)W * H;
    const Camera cam(cam_f);
    const bool have_prev = prev_cam_f != nullptr;
    const bool same_camera = have_prev && memcmp(cam_f, prev_cam_f, 12 * sizeof(float)) == 0;

    // ---- steps 1 to 3, pixel by pixel
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = st.at(x, y);
            float* o_integ = integ + 4 * i;
            float* o_mom = hist_mom_out + 4 * i;
            if (!st.is_hit(x, y)) {                       // a miss passes the accumulator through, history 1
                const float l = L(accum + 4 * i);
                o_integ[0] = accum[4 * i]; o_integ[1] = accum[4 * i + 1]; o_integ[2] = accum[4 * i + 2]; o_integ[3] = 0.0f;
                o_mom[0] = l; o_mom[1] = l * l; o_mom[2] = 1.0f; o_mom[3] = 0.0f;
                continue;
            }
            const trc_gbuffer_texel& t = g[i];
            float c[3];
            st.input(x, y, c);
            const float lc = L(c);

            // step 2 (amended): which taps of the previous frame, with what weights, and the depth to compare
            struct Tap { int x, y; float w; } taps[4];
            int n_taps = 0;
            float zq = t.depth;
            if (have_prev) {
                const bool moved = motion && motion[i].moved == 1u;
                if (same_camera && !moved) {
                    taps[0] = {x, y, 1.0f};
                    n_taps = 1;
                } else {
                    const Camera prev(prev_cam_f);
                    Vec P;
                    if (moved) {
                        P = load(motion[i].prev);
                    } else {
                        const float u = (float)x / (float)W, v = (float)y / (float)H;
                        const Vec dir = ((cam.cll + cam.hor * u) + cam.ver * v) - cam.eye;
                        const Vec d = dir * (1.0f / sqrtf(dot(dir, dir)));
                        P = cam.eye + d * t.depth;
                    }
                    const Vec q = P - prev.eye;
                    const Vec a = prev.cll - prev.eye;
                    const Vec m = cross(prev.hor, prev.ver);
                    const float s = dot(a, m) / dot(q, m);
                    const float up = (dot(q, prev.hor) * s - dot(a, prev.hor)) / dot(prev.hor, prev.hor);
                    const float vp = (dot(q, prev.ver) * s - dot(a, prev.ver)) / dot(prev.ver, prev.ver);
                    const float px = up * (float)W, py = vp * (float)H;
                    zq = sqrtf(dot(q, q));
                    const bool valid = s > 0.0f && s < INFINITY && -1.0f < px && px < (float)W && -1.0f < py && py < (float)H;
                    if (valid) {
                        const float x0 = floorf(px), y0 = floorf(py);
                        const float fx = px - x0, fy = py - y0;
                        taps[0] = {(int)x0, (int)y0, (1.0f - fx) * (1.0f - fy)};
                        taps[1] = {(int)x0 + 1, (int)y0, fx * (1.0f - fy)};
                        taps[2] = {(int)x0, (int)y0 + 1, (1.0f - fx) * fy};
                        taps[3] = {(int)x0 + 1, (int)y0 + 1, fx * fy};
                        n_taps = 4;
                    }
                }
            }
            float Wsum = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, M1 = 0.0f, M2 = 0.0f, N = 0.0f;
            for (int k = 0; k < n_taps; ++k) {
                if (!st.in(taps[k].x, taps[k].y)) continue;
                const size_t j = st.at(taps[k].x, taps[k].y);
                const trc_gbuffer_texel& o = g_prev[j];
                const bool consistent = o.id == t.id && fabsf(o.depth - zq) <= 0.1f * zq &&
                                        t.normal[0] * o.normal[0] + t.normal[1] * o.normal[1] + t.normal[2] * o.normal[2] >= 0.9f;
                if (!consistent) continue;
                const float w = taps[k].w;
                Wsum += w;
                for (int ch = 0; ch < 3; ++ch) C[ch] += w * hist_col[4 * j + ch];
                M1 += w * hist_mom[4 * j];
                M2 += w * hist_mom[4 * j + 1];
                N += w * hist_mom[4 * j + 2];
            }
            const bool valid = Wsum >= 0.01f;
            float n = 1.0f, colour[3] = {c[0], c[1], c[2]}, mu1 = lc, mu2 = lc * lc;
            if (valid) {
                n = N / Wsum + 1.0f;
                if (n > 64.0f) n = 64.0f;
                const float r = 1.0f / n;
                const float a = r > p->alpha_color ? r : p->alpha_color, am = r > p->alpha_moments ? r : p->alpha_moments;
                for (int ch = 0; ch < 3; ++ch) { const float prev = C[ch] / Wsum; colour[ch] = prev + (c[ch] - prev) * a; }
                const float m1 = M1 / Wsum, m2 = M2 / Wsum;
                mu1 = m1 + (lc - m1) * am;
                mu2 = m2 + (lc * lc - m2) * am;
            }

            // step 3
            float variance;
            if (n >= (float)p->min_history) {
                variance = max0(mu2 - mu1 * mu1);
            } else {
                const float gx = st.gradient(x, y, 1, 0), gy = st.gradient(x, y, 0, 1);
                float Ws = 0.0f, S1 = 0.0f, S2 = 0.0f;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -3; dx <= 3; ++dx) {
                        if (!st.tap(x + dx, y + dy)) continue;
                        const trc_gbuffer_texel& o = g[st.at(x + dx, y + dy)];
                        float cq[3];
                        st.input(x + dx, y + dy, cq);
                        const float lq = L(cq);
                        const float w = dm_expf(-(fabsf(t.depth - o.depth) / st.D(t.depth, gx, gy, dx, dy))) * st.w8(t, o);
                        Ws += w; S1 += w * lq; S2 += w * (lq * lq);
                    }
                variance = 0.0f;
                if (Ws > 0.0f) { const float m1 = S1 / Ws; variance = max0(S2 / Ws - m1 * m1); }
            }
            o_integ[0] = colour[0]; o_integ[1] = colour[1]; o_integ[2] = colour[2]; o_integ[3] = variance;
            o_mom[0] = mu1; o_mom[1] = mu2; o_mom[2] = n; o_mom[3] = 0.0f;
        }

    // ---- step 4
    std::vector<float> src(integ, integ + 4 * n_px), dst(4 * n_px);
    if (p->iterations == 0) memcpy(hist_col_out, integ, 4 * n_px * sizeof(float));
    static const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}, gauss[3] = {0.25f, 0.5f, 0.25f};
    for (uint32_t it = 0; it < p->iterations; ++it) {
        const int step = 1 << it;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = st.at(x, y);
                const float* s = &src[4 * i];
                float* r = &dst[4 * i];
                memcpy(r, s, 4 * sizeof(float));
                if (!st.is_hit(x, y)) continue;
                const trc_gbuffer_texel& t = g[i];
                const float gx = st.gradient(x, y, 1, 0), gy = st.gradient(x, y, 0, 1);
                float G = 0.0f, V3 = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!st.tap(x + dx, y + dy)) continue;
                        const float w = gauss[dy + 1] * gauss[dx + 1];
                        G += w; V3 += w * src[4 * st.at(x + dx, y + dy) + 3];
                    }
                const float phi = p->sigma_l * sqrtf(max0(V3 / G)) + 1e-10f;
                const float lc = L(s);
                float Ws = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, V = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int qx = x + step * dx, qy = y + step * dy;
                        if (!st.tap(qx, qy)) continue;
                        const trc_gbuffer_texel& o = g[st.at(qx, qy)];
                        const float* q = &src[4 * st.at(qx, qy)];
                        const float wz = fabsf(t.depth - o.depth) / st.D(t.depth, gx, gy, step * dx, step * dy);
                        const float wl = fabsf(lc - L(q)) / phi;
                        const float w = ((h[dx + 2] * h[dy + 2]) * st.w8(t, o)) * dm_expf(-(wz + wl));
                        Ws += w;
                        for (int ch = 0; ch < 3; ++ch) C[ch] += w * (q[ch] - s[ch]);
                        V += (w * w) * q[3];
                    }
                if (Ws > 0.0f) {
                    for (int ch = 0; ch < 3; ++ch) r[ch] = s[ch] + C[ch] / Ws;
                    r[3] = V / (Ws * Ws);
                }
            }
        src.swap(dst);
        if (it == 0) memcpy(hist_col_out, src.data(), 4 * n_px * sizeof(float));
    }

    // ---- step 5
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = st.at(x, y);
            if (!st.is_hit(x, y)) { memcpy(out + 4 * i, accum + 4 * i, 4 * sizeof(float)); continue; }
            for (int ch = 0; ch < 3; ++ch) out[4 * i + ch] = st.demod ? src[4 * i + ch] * st.albedo(i, ch) : src[4 * i + ch];
            out[4 * i + 3] = accum[4 * i + 3];
        }
    return 0;
}

}  // extern "C"
