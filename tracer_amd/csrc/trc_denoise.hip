// trc_denoise.hip -- the SVGF stage of the frame (include/tracer_abi.h, "SVGF denoiser"): the G-buffer pass, the fused
// temporal + variance pass and the a-trous iterations of Schied et al., HPG 2017, on the context's accumulator.
//
// gfx950 shape: one wavefront per 8x8 pixel tile, one pixel per lane.  Every plane a tap reads is a float4: (colour, variance)
// and the G-buffer's first half (depth, normal), so a tap is one 16-byte load; the albedo half is read at the centre pixel only
// (and by the 7x7 variance estimate of the first frames).  A 1080p plane is 33 MB: the working set stays in the Infinity Cache.
// Arithmetic is the header's statement operation by operation (tests/svgf_ref/svgf_ref.cpp restates it on the CPU): binary32,
// no contraction, correctly rounded division and square root, exp from trc_detmath.h.
#include "trc_ctx.hpp"
#include "trc_render_config.hpp"     // TRC_DEFER_*: the record policy trc_trace_rays' production walk uses

#include <cstring>

namespace {

constexpr float kInf = __builtin_inff();
constexpr float kDepthRel = 0.1f, kNormalCos = 0.9f, kMinHistoryWeight = 0.01f, kMaxHistory = 64.0f;
constexpr float kDepthEpsRel = 0.001f, kPhiEps = 1e-10f;

struct DnCam { float eye[3], hor[3], ver[3], cll[3]; };     // the four camera vectors the filter reads

DnCam dn_cam(const DCamera& c) {
    DnCam d;
    for (int k = 0; k < 3; ++k) { d.eye[k] = c.lookFrom[k]; d.hor[k] = c.horizontal[k]; d.ver[k] = c.vertical[k]; d.cll[k] = c.cornerLowLeft[k]; }
    return d;
}

struct DnParams {
    uint32_t W, H;
    uint32_t demod, nsq;            // nsq: log2 of the normal exponent (squarings)
    float alpha_c, alpha_m, sigma_z, sigma_l;
    uint32_t min_hist;
};

TRC_DEV float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
TRC_DEV bool is_hit(float depth) { return depth < kInf; }        // depth is +inf exactly on a miss (id == TRC_GBUFFER_MISS)
TRC_DEV float normal_weight(float4 a, float4 b, uint32_t nsq) {
    const float d = a.y * b.y + a.z * b.z + a.w * b.w;
    float w = d > 0.0f ? d : 0.0f;
    for (uint32_t k = 0; k < nsq; ++k) w = w * w;
    return w;
}
TRC_DEV float nonneg(float v) { return v > 0.0f ? v : 0.0f; }          // max(0, v), +0 for -0 and NaN
TRC_DEV float demod1(float c, float albedo) { return c / (albedo > TRC_DENOISE_ALBEDO_EPS ? albedo : TRC_DENOISE_ALBEDO_EPS); }
TRC_DEV float remod1(float c, float albedo) { return c * (albedo > TRC_DENOISE_ALBEDO_EPS ? albedo : TRC_DENOISE_ALBEDO_EPS); }

// the tile of this lane: 8x8 pixels per wavefront
TRC_DEV bool tile_pixel(uint32_t W, uint32_t H, uint32_t& x, uint32_t& y) {
    x = blockIdx.x * 8u + (threadIdx.x & 7u);
    y = blockIdx.y * 8u + (threadIdx.x >> 3);
    return x < W && y < H;
}

// depth gradient stencil: the smaller one-sided difference to the in-bounds hit neighbours, per axis (0 when there are none)
TRC_DEV void depth_grad(const float4* gb, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float z, float& gx, float& gy) {
    const size_t i = (size_t)y * W + x;
    float a = kInf, b = kInf;
    if (x + 1 < W) { const float zz = gb[2 * (i + 1)].x; if (is_hit(zz)) a = fabsf(zz - z); }
    if (x > 0)     { const float zz = gb[2 * (i - 1)].x; if (is_hit(zz)) b = fabsf(zz - z); }
    gx = fminf(a, b);
    if (gx == kInf) gx = 0.0f;
    a = kInf; b = kInf;
    if (y + 1 < H) { const float zz = gb[2 * (i + W)].x; if (is_hit(zz)) a = fabsf(zz - z); }
    if (y > 0)     { const float zz = gb[2 * (i - W)].x; if (is_hit(zz)) b = fabsf(zz - z); }
    gy = fminf(a, b);
    if (gy == kInf) gy = 0.0f;
}

// ---------------------------------------------------------------- G-buffer: the camera pass's primary hit, walked by the
// production scene_hit (the same instantiation trc_trace_rays' TRC_TRACE_PRODUCTION runs); no RNG is consumed
// TEX: image textures (trc_upload_textures; hit_color<true> over `tt`, which the other instantiations do not read)
// MOTION (trc_denoise_track_motion, a snapshot in force): the motion texel of the pixel besides (header, "Motion tracking"); the other
// instantiations do not read `mo`
struct KMotion {
    const uint32_t* idx;        // the scene's index array: triangle t names vertices idx[3t .. 3t + 2]
    const float4* snap;         // the snapshot: one float4 per vertex, its position when the last trc_denoise ran
    const uint32_t* psnap;      // ... and the blob's primitive section [off_spheres, off_materials) as it stood then (null: no primitives)
    float4* plane;              // W*H motion texels: (prev, moved)
};
TRC_DEV float pick(const F3& a, uint32_t axis) { return axis == 0u ? a.x : axis == 1u ? a.y : a.z; }
TRC_DEV void put(F3& a, uint32_t axis, float v) { if (axis == 0u) a.x = v; else if (axis == 1u) a.y = v; else a.z = v; }
// The motion texel of an analytic winner (header, "Motion tracking"): where the point rec.p of the primitive was under the snapshot's
// record -- the same direction from a sphere's centre, the same fractions of a square's ranges, the same object-space point of a cube.
// The current record is the staged one (LDS), the snapshot's comes from memory.  moved = 0: the all-zero texel
TRC_DEV float4 analytic_motion(const SceneRef& S, const uint32_t* psnap, const HitRec& rec) {
    const uint32_t type = rec.tag >> kTagIndexBits, index = rec.tag & kTagIndexMask;
    const F3 p = rec.p;
    bool moved;
    F3 prev;
    if (type == 0u) {                                   // TRC_PRIM_SPHERE
        const uint32_t off = S.off_spheres + index * kSphereDwords;
        const float4 c = ld4_lds(S.small_base + off), s = ld4_global(psnap + (off - S.off_spheres));
        moved = c.x != s.x || c.y != s.y || c.z != s.z || c.w != s.w;
        const F3 n = f3((p.x - c.x) / c.w, (p.y - c.y) / c.w, (p.z - c.z) / c.w);
        prev = f3(s.x + n.x * s.w, s.y + n.y * s.w, s.z + n.z * s.w);
    } else if (type == 1u) {                            // TRC_PRIM_SQUARE
        const uint32_t off = S.off_squares + index * kSquareDwords;
        const float4 rg = ld4_lds(S.small_base + off), kx = ld4_lds(S.small_base + off + 4);
        const float4 rs = ld4_global(psnap + (off - S.off_spheres)), ks = ld4_global(psnap + (off - S.off_spheres) + 4);
        const uint32_t axes = __float_as_uint(kx.z), axes_s = __float_as_uint(ks.z);
        moved = rg.x != rs.x || rg.y != rs.y || rg.z != rs.z || rg.w != rs.w || kx.x != ks.x || axes != axes_s;
        const float a = pick(p, axes & 3u), b = pick(p, (axes >> 2) & 3u);
        const float fu = (a - rg.x) / (rg.y - rg.x), fv = (b - rg.z) / (rg.w - rg.z);
        prev = f3(0.0f);
        put(prev, (axes_s >> 4) & 3u, ks.x);
        put(prev, axes_s & 3u, rs.x + fu * (rs.y - rs.x));
        put(prev, (axes_s >> 2) & 3u, rs.z + fv * (rs.w - rs.z));
    } else {                                            // TRC_PRIM_CUBE: inverse columns in dwords 0..11, model columns in 12..23
        const uint32_t off = S.off_cubes + index * kCubeDwords;
        const uint32_t* cb = S.small_base + off;
        const uint32_t* cs = psnap + (off - S.off_spheres);
        const float4 i0 = ld4_lds(cb), i1 = ld4_lds(cb + 4), i2 = ld4_lds(cb + 8), m0 = ld4_lds(cb + 12), m1 = ld4_lds(cb + 16), m2 = ld4_lds(cb + 20);
        const float4 j0 = ld4_global(cs), j1 = ld4_global(cs + 4), j2 = ld4_global(cs + 8), n0 = ld4_global(cs + 12), n1 = ld4_global(cs + 16), n2 = ld4_global(cs + 20);
        moved = i0.x != j0.x || i0.y != j0.y || i0.z != j0.z || i0.w != j0.w || i1.x != j1.x || i1.y != j1.y || i1.z != j1.z || i1.w != j1.w ||
                i2.x != j2.x || i2.y != j2.y || i2.z != j2.z || i2.w != j2.w || m0.x != n0.x || m0.y != n0.y || m0.z != n0.z || m0.w != n0.w ||
                m1.x != n1.x || m1.y != n1.y || m1.z != n1.z || m1.w != n1.w || m2.x != n2.x || m2.y != n2.y || m2.z != n2.z || m2.w != n2.w;
        const F3 ic0 = f3(i0.x, i0.y, i0.z), ic1 = f3(i0.w, i1.x, i1.y), ic2 = f3(i1.z, i1.w, i2.x), ic3 = f3(i2.y, i2.z, i2.w);
        const F3 mc0 = f3(n0.x, n0.y, n0.z), mc1 = f3(n0.w, n1.x, n1.y), mc2 = f3(n1.z, n1.w, n2.x), mc3 = f3(n2.y, n2.z, n2.w);
        const F3 q = ((ic0 * p.x + ic1 * p.y) + ic2 * p.z) + ic3;
        prev = ((mc0 * q.x + mc1 * q.y) + mc2 * q.z) + mc3;
    }
    return moved ? make_float4(prev.x, prev.y, prev.z, __uint_as_float(1u)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// RAYS (trc_denoise_guide_rays): the pixel's ray is its record of set 0 of the context's ray sets (`rays`: W*H records of two float4, origin | tmax
// and direction | pad), made as trc_trace_rays makes one; the other instantiations read the camera and not `rays`
template <bool LDS, bool TEX = false, bool MOTION = false, bool RAYS = false>
__global__ void __launch_bounds__(kBlock) k_gbuffer(const KScene ks, const DnCam cam, uint32_t W, uint32_t H, float4* gb, const TexTable tt, const KMotion mo,
                                                    const float4* __restrict__ rays) {
    const DScene& sc = ks.sc;
    const uint32_t* small_base = stage_scene(sc);
    uint32_t* stack = lane_stack(sc);
    uint32_t* lvstack = lane_lvstack(sc);
    uint32_t x, y;
    if (!tile_pixel(W, H, x, y)) return;
    Ray ray;
    if constexpr (RAYS) {
        const float4* const rec = rays + 2u * ((size_t)y * W + x);
        const float4 o = rec[0], d = rec[1];
        ray = make_ray(f3(o.x, o.y, o.z), f3(d.x, d.y, d.z));      // normalised on entry; tmax and pad are not read
    } else {
        const float u = (float)x / (float)W, v = (float)y / (float)H;
        const F3 eye = f3(cam.eye[0], cam.eye[1], cam.eye[2]);
        const F3 sample = f3(cam.cll[0], cam.cll[1], cam.cll[2]) + f3(cam.hor[0], cam.hor[1], cam.hor[2]) * u + f3(cam.ver[0], cam.ver[1], cam.ver[2]) * v;
        ray = make_ray(eye, sample - eye);
    }
    SceneRef S = make_scene_ref(sc, small_base);
    HitRec rec;
    hit_init(rec);
    TravCounters cnt;
    counters_zero(cnt);
    const F3 root_min = f3(ks.root_box[0], ks.root_box[1], ks.root_box[2]), root_max = f3(ks.root_box[3], ks.root_box[4], ks.root_box[5]);
    const bool h = scene_hit<LDS, false, false, true, false, false, LDS ? TRC_DEFER_LDS : TRC_DEFER_GLOBAL>(S, root_min, root_max, ray, rec, FLT_MAX, stack, lvstack, cnt);
    const size_t i = (size_t)y * W + x;
    if (MOTION) {
        // an analytic winner: analytic_motion.  A triangle winner: its position record and its three indices in one round trip, the three snapshot positions in a second; the
        // barycentrics are triangle_hit_test's (dev_intersect.hpp) operation by operation, prev is rec.p's expression over the snapshot
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (h && (rec.tag >> kTagIndexBits) == kTagTriangle) {
            const uint32_t t = rec.tag & kTagIndexMask;
            const TriPos pos = load_tripos(S, t);
            const uint32_t i0 = mo.idx[3 * (size_t)t], i1 = mo.idx[3 * (size_t)t + 1], i2 = mo.idx[3 * (size_t)t + 2];
            const float4 pa = mo.snap[i0], pb = mo.snap[i1], pc = mo.snap[i2];
            const F3 v0 = f3(pos.a.x, pos.a.y, pos.a.z), v1 = f3(pos.b.x, pos.b.y, pos.b.z), v2 = f3(pos.c.x, pos.c.y, pos.c.z);
            const F3 e1 = v1 - v0;
            const F3 e2 = v2 - v0;
            const F3 pvec = cross(ray.d, e2);
            const float det = dot(e1, pvec);
            const float inv = 1 / det;
            const F3 tvec = ray.o - v0;
            const float bu = dot(tvec, pvec) * inv;
            const F3 qvec = cross(tvec, e1);
            const float bv = dot(ray.d, qvec) * inv;
            const float bw = 1.0f - bu - bv;
            const F3 prev = (bu * f3(pb.x, pb.y, pb.z) + bv * f3(pc.x, pc.y, pc.z)) + bw * f3(pa.x, pa.y, pa.z);
            const bool moved = pos.a.x != pa.x || pos.a.y != pa.y || pos.a.z != pa.z || pos.b.x != pb.x || pos.b.y != pb.y || pos.b.z != pb.z ||
                               pos.c.x != pc.x || pos.c.y != pc.y || pos.c.z != pc.z;
            m = make_float4(prev.x, prev.y, prev.z, __uint_as_float(moved ? 1u : 0u));
        } else if (h && mo.psnap) {
            m = analytic_motion(S, mo.psnap, rec);
        }
        mo.plane[i] = m;
    }
    if (!h) {
        gb[2 * i] = make_float4(kInf, 0.0f, 0.0f, 0.0f);
        gb[2 * i + 1] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(TRC_GBUFFER_MISS));
        return;
    }
    Shade sh;
    sh.mats = small_base + sc.off_materials;
    const F3 alb = mat_type(sh, rec.material) == kMatDiffuse ? f3(1.0f) : hit_color<TEX>(S, sh, rec, &tt);     // emitters: 1
    gb[2 * i] = make_float4(rec.t, rec.sn.x, rec.sn.y, rec.sn.z);
    gb[2 * i + 1] = make_float4(alb.x, alb.y, alb.z, __uint_as_float(rec.material));
}

// the snapshot (trc_denoise_moved): the position of every 32-byte vertex as one float4, w = 0
__global__ void __launch_bounds__(256) k_snapshot_positions(const float4* __restrict__ verts, uint32_t n, float4* __restrict__ snap) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 v = verts[2 * (size_t)i];
    snap[i] = make_float4(v.x, v.y, v.z, 0.0f);
}

// ---------------------------------------------------------------- temporal pass + variance (header steps 1-3)
struct KTemporal {
    DnParams p;
    DnCam cur, prev;
    uint32_t have_prev, same_cam;
    uint32_t guide;             // trc_denoise_guide_rays: a ray set defines no inverse -- a moved pixel has no valid history (same_cam is 1)
    const float4* accum;
    const float4* gb;
    const float4* gb_prev;
    const float4* hist_col;
    const float4* hist_mom;
    float4* integ;
    float4* mom;
    const float4* motion;       // MOTION only
};

// MOTION: k.motion is the plane k_gbuffer<.., .., true> wrote for this frame; a pixel with moved = 1 takes the four-tap rule with P = prev
template <bool MOTION>
__global__ void __launch_bounds__(64) k_svgf_temporal(const KTemporal k) {
    const DnParams& p = k.p;
    uint32_t x, y;
    if (!tile_pixel(p.W, p.H, x, y)) return;
    const uint32_t W = p.W, H = p.H;
    const size_t i = (size_t)y * W + x;
    const float4 a = k.accum[i];
    const float4 g0 = k.gb[2 * i];
    if (!is_hit(g0.x)) {                                  // a miss passes through, history 1
        const float L = lum(a.x, a.y, a.z);
        k.integ[i] = make_float4(a.x, a.y, a.z, 0.0f);
        k.mom[i] = make_float4(L, L * L, 1.0f, 0.0f);
        return;
    }
    const float4 g1 = k.gb[2 * i + 1];
    const float z = g0.x;
    float c[3] = {a.x, a.y, a.z};
    if (p.demod) { c[0] = demod1(c[0], g1.x); c[1] = demod1(c[1], g1.y); c[2] = demod1(c[2], g1.z); }
    const float L = lum(c[0], c[1], c[2]);

    // reprojection into the previous frame
    float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sm1 = 0.0f, sm2 = 0.0f, sn = 0.0f;
    if (k.have_prev) {
        int tx[4], ty[4];
        float tw[4];
        int ntaps;
        float zq;
        bool ok = true;
        float4 mt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MOTION) mt = k.motion[i];
        const bool moved = MOTION && __float_as_uint(mt.w) != 0u;
        if (k.same_cam && !moved) {
            ntaps = 1; tx[0] = (int)x; ty[0] = (int)y; tw[0] = 1.0f; zq = z;
        } else if (k.guide) {
            ntaps = 0; zq = z; ok = false;
        } else {
            ntaps = 4;
            const float u = (float)x / (float)W, v = (float)y / (float)H;
            const F3 eye = f3(k.cur.eye[0], k.cur.eye[1], k.cur.eye[2]);
            const F3 sample = f3(k.cur.cll[0], k.cur.cll[1], k.cur.cll[2]) + f3(k.cur.hor[0], k.cur.hor[1], k.cur.hor[2]) * u +
                              f3(k.cur.ver[0], k.cur.ver[1], k.cur.ver[2]) * v;
            const F3 d = normalize(sample - eye);
            const F3 P = moved ? f3(mt.x, mt.y, mt.z) : eye + d * z;
            const F3 pe = f3(k.prev.eye[0], k.prev.eye[1], k.prev.eye[2]);
            const F3 ph = f3(k.prev.hor[0], k.prev.hor[1], k.prev.hor[2]), pv = f3(k.prev.ver[0], k.prev.ver[1], k.prev.ver[2]);
            const F3 q = P - pe;
            const F3 av = f3(k.prev.cll[0], k.prev.cll[1], k.prev.cll[2]) - pe;
            const F3 m = cross(ph, pv);
            const float s = dot(av, m) / dot(q, m);
            const float pu = (dot(q, ph) * s - dot(av, ph)) / dot(ph, ph);
            const float pvv = (dot(q, pv) * s - dot(av, pv)) / dot(pv, pv);
            const float px = pu * (float)W, py = pvv * (float)H;
            ok = s > 0.0f && s < kInf && px > -1.0f && px < (float)W && py > -1.0f && py < (float)H;
            zq = length(q);
            if (ok) {
                const float fx0 = floorf(px), fy0 = floorf(py);
                const float fx = px - fx0, fy = py - fy0;
                const int x0 = (int)fx0, y0 = (int)fy0;
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                for (int t = 0; t < 4; ++t) { tx[t] = x0 + (t & 1); ty[t] = y0 + (t >> 1); tw[t] = wx[t & 1] * wy[t >> 1]; }
            }
        }
        if (ok) {
            const uint32_t id = __float_as_uint(g1.w);
            for (int t = 0; t < ntaps; ++t) {
                if (tx[t] < 0 || ty[t] < 0 || tx[t] >= (int)W || ty[t] >= (int)H) continue;
                const size_t j = (size_t)ty[t] * W + (uint32_t)tx[t];
                const float4 q0 = k.gb_prev[2 * j];
                if (__float_as_uint(k.gb_prev[2 * j + 1].w) != id) continue;
                if (!(fabsf(q0.x - zq) <= kDepthRel * zq)) continue;
                if (!(g0.y * q0.y + g0.z * q0.z + g0.w * q0.w >= kNormalCos)) continue;
                const float w = tw[t];
                const float4 hc = k.hist_col[j], hm = k.hist_mom[j];
                sw += w;
                sc[0] += w * hc.x; sc[1] += w * hc.y; sc[2] += w * hc.z;
                sm1 += w * hm.x; sm2 += w * hm.y; sn += w * hm.z;
            }
        }
    }
    const bool valid = sw >= kMinHistoryWeight;
    float col[3], mu1, mu2, n;
    if (valid) {
        n = sn / sw + 1.0f;
        if (n > kMaxHistory) n = kMaxHistory;
        const float inv = 1.0f / n;
        const float ac = inv > p.alpha_c ? inv : p.alpha_c, am = inv > p.alpha_m ? inv : p.alpha_m;
        for (int ch = 0; ch < 3; ++ch) { const float pc = sc[ch] / sw; col[ch] = pc + (c[ch] - pc) * ac; }
        const float m1 = sm1 / sw, m2 = sm2 / sw;
        mu1 = m1 + (L - m1) * am;
        mu2 = m2 + (L * L - m2) * am;
    } else {
        n = 1.0f;
        col[0] = c[0]; col[1] = c[1]; col[2] = c[2];
        mu1 = L; mu2 = L * L;
    }

    float var;
    if (n >= (float)p.min_hist) {
        var = nonneg(mu2 - mu1 * mu1);
    } else {                                              // 7x7 estimate from the demodulated input
        float gx, gy;
        depth_grad(k.gb, W, H, x, y, z, gx, gy);
        float ws = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int yy = (int)y + dy;
            if (yy < 0 || yy >= (int)H) continue;
            for (int dx = -3; dx <= 3; ++dx) {
                const int xx = (int)x + dx;
                if (xx < 0 || xx >= (int)W) continue;
                const size_t j = (size_t)yy * W + (uint32_t)xx;
                const float4 q0 = k.gb[2 * j];
                if (!is_hit(q0.x)) continue;
                const float4 qa = k.accum[j];
                float qc[3] = {qa.x, qa.y, qa.z};
                if (p.demod) { const float4 q1 = k.gb[2 * j + 1]; qc[0] = demod1(qc[0], q1.x); qc[1] = demod1(qc[1], q1.y); qc[2] = demod1(qc[2], q1.z); }
                const float Lq = lum(qc[0], qc[1], qc[2]);
                const float D = p.sigma_z * (gx * fabsf((float)dx) + gy * fabsf((float)dy)) + kDepthEpsRel * z;
                const float w = dm_expf(-(fabsf(z - q0.x) / D)) * normal_weight(g0, q0, p.nsq);
                ws += w; s1 += w * Lq; s2 += w * (Lq * Lq);
            }
        }
        if (ws > 0.0f) {
            const float m1 = s1 / ws;
            var = nonneg(s2 / ws - m1 * m1);
        } else {
            var = 0.0f;
        }
    }
    k.integ[i] = make_float4(col[0], col[1], col[2], var);
    k.mom[i] = make_float4(mu1, mu2, n, 0.0f);
}

// ---------------------------------------------------------------- one a-trous iteration (header step 4), + the output (step 5)
struct KAtrous {
    DnParams p;
    uint32_t step;
    const float4* src;          // (colour, variance)
    const float4* gb;
    const float4* accum;        // misses and alpha of the output
    float4* dst;                // (colour, variance) or null
    float4* final_out;          // remodulated RGBA or null (the last iteration)
};

__global__ void __launch_bounds__(64) k_svgf_atrous(const KAtrous k) {
    const DnParams& p = k.p;
    uint32_t x, y;
    if (!tile_pixel(p.W, p.H, x, y)) return;
    const uint32_t W = p.W, H = p.H;
    const size_t i = (size_t)y * W + x;
    const float4 s = k.src[i];
    const float4 g0 = k.gb[2 * i];
    if (!is_hit(g0.x)) {
        if (k.dst) k.dst[i] = s;
        if (k.final_out) k.final_out[i] = k.accum[i];
        return;
    }
    const float z = g0.x;
    float gx, gy;
    depth_grad(k.gb, W, H, x, y, z, gx, gy);
    // 3x3 Gaussian of the variance
    const float kG[3] = {0.25f, 0.5f, 0.25f};
    float sg = 0.0f, sv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = (int)y + dy;
        if (yy < 0 || yy >= (int)H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = (int)x + dx;
            if (xx < 0 || xx >= (int)W) continue;
            const size_t j = (size_t)yy * W + (uint32_t)xx;
            if (!is_hit(k.gb[2 * j].x)) continue;
            const float g = kG[dy + 1] * kG[dx + 1];
            sg += g; sv += g * k.src[j].w;
        }
    }
    const float phi = p.sigma_l * sqrtf(nonneg(sv / sg)) + kPhiEps;
    const float L = lum(s.x, s.y, s.z);
    const float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int st = (int)k.step;
    float ws = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, v = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = (int)y + dy * st;
        if (yy < 0 || yy >= (int)H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = (int)x + dx * st;
            if (xx < 0 || xx >= (int)W) continue;
            const size_t j = (size_t)yy * W + (uint32_t)xx;
            const float4 q0 = k.gb[2 * j];
            if (!is_hit(q0.x)) continue;
            const float4 qs = k.src[j];
            const float D = p.sigma_z * (gx * fabsf((float)(dx * st)) + gy * fabsf((float)(dy * st))) + kDepthEpsRel * z;
            const float wz = fabsf(z - q0.x) / D;
            const float wl = fabsf(L - lum(qs.x, qs.y, qs.z)) / phi;
            const float w = ((kH[dx + 2] * kH[dy + 2]) * normal_weight(g0, q0, p.nsq)) * dm_expf(-(wz + wl));
            ws += w;
            c0 += w * (qs.x - s.x); c1 += w * (qs.y - s.y); c2 += w * (qs.z - s.z);
            v += (w * w) * qs.w;
        }
    }
    const float4 o = ws > 0.0f ? make_float4(s.x + c0 / ws, s.y + c1 / ws, s.z + c2 / ws, v / (ws * ws)) : s;
    if (k.dst) k.dst[i] = o;
    if (k.final_out) {
        float r = o.x, g = o.y, b = o.z;
        if (p.demod) { const float4 g1 = k.gb[2 * i + 1]; r = remod1(r, g1.x); g = remod1(g, g1.y); b = remod1(b, g1.z); }
        k.final_out[i] = make_float4(r, g, b, k.accum[i].w);
    }
}

// 0 iterations: the output is the temporal colour, remodulated
__global__ void __launch_bounds__(64) k_svgf_finish(const DnParams p, const float4* src, const float4* gb, const float4* accum, float4* out) {
    uint32_t x, y;
    if (!tile_pixel(p.W, p.H, x, y)) return;
    const size_t i = (size_t)y * p.W + x;
    if (!is_hit(gb[2 * i].x)) { out[i] = accum[i]; return; }
    const float4 s = src[i];
    float r = s.x, g = s.y, b = s.z;
    if (p.demod) { const float4 g1 = gb[2 * i + 1]; r = remod1(r, g1.x); g = remod1(g, g1.y); b = remod1(b, g1.z); }
    out[i] = make_float4(r, g, b, accum[i].w);
}

bool same_dn_cam(const DnCam& a, const DnCam& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

// ---------------------------------------------------------------- context state
struct DenoiseState {
    uint32_t W = 0, H = 0;
    float4* gb[2] = {nullptr, nullptr};       // 2 float4 per pixel: (depth, normal), (albedo, id)
    float4* hist_col[2] = {nullptr, nullptr};
    float4* hist_mom[2] = {nullptr, nullptr};
    float4* integ = nullptr;
    float4* tmp[2] = {nullptr, nullptr};
    float4* out = nullptr;
    int gb_cur = 0, hist_cur = 0;              // gb[gb_cur]: the G-buffer of the last trc_denoise; hist_*[hist_cur]: its history
    bool gb_valid = false;                     // gb[gb_cur] belongs to the scene and to gb_cam
    DCamera gb_cam{};
    bool have_hist = false;                    // history of a frame of this scene exists
    DnCam hist_cam{};                          // the camera that frame was taken with
    bool has_output = false;
    // trc_denoise_track_motion (trc_ctx::track_motion); all of it goes with the frame, the snapshot with the scene too
    float4* motion = nullptr;                  // W*H motion texels, written by every trc_denoise while tracking is on
    bool motion_ready = false;                 // ... and one has been: trc_download_motion answers
    bool motion_zero = false;                  // the plane holds zeros (a denoise with no snapshot in force)
    float4* snap = nullptr; uint32_t snap_n = 0;      // one position per vertex (allocated by trc_denoise), for snap_n vertices
    uint32_t* psnap = nullptr; uint32_t psnap_dwords = 0;      // the blob's primitive section (allocated by trc_denoise where the scene has one)
    bool snap_live = false;                    // both filled by the first moving call since the last trc_denoise: in force for the next
    // trc_denoise_guide_rays (trc_ctx::guide_rays): the generation of the ray sets (trc_ctx::ray_gen) gb[gb_cur] was walked along, and the
    // one the history was made under
    uint64_t gb_ray_gen = 0, hist_ray_gen = 0;
};

// k_gbuffer<LDS, TEX, MOTION, RAYS> by its four switches
template <bool LDS, bool TEX, bool MOTION, bool RAYS, class... A>
static void launch_gbuffer(hipStream_t st, dim3 grid, size_t lds, A... a) { hipLaunchKernelGGL((k_gbuffer<LDS, TEX, MOTION, RAYS>), grid, dim3(kBlock), lds, st, a...); }
template <bool LDS, bool TEX, bool MOTION, class... A>
static void launch_gbuffer(bool rays, A... a) { if (rays) launch_gbuffer<LDS, TEX, MOTION, true>(a...); else launch_gbuffer<LDS, TEX, MOTION, false>(a...); }
template <bool LDS, bool TEX, class... A>
static void launch_gbuffer(bool motion, bool rays, A... a) { if (motion) launch_gbuffer<LDS, TEX, true>(rays, a...); else launch_gbuffer<LDS, TEX, false>(rays, a...); }
template <bool LDS, class... A>
static void launch_gbuffer(bool tex, bool motion, bool rays, A... a) { if (tex) launch_gbuffer<LDS, true>(motion, rays, a...); else launch_gbuffer<LDS, false>(motion, rays, a...); }

void trc_denoise_release(trc_ctx* ctx) {
    DenoiseState* s = ctx ? ctx->denoise : nullptr;
    if (!s) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (float4* b : {s->gb[0], s->gb[1], s->hist_col[0], s->hist_col[1], s->hist_mom[0], s->hist_mom[1], s->integ, s->tmp[0], s->tmp[1], s->out, s->motion, s->snap})
        (void)hipFree(b);
    (void)hipFree(s->psnap);
    delete s;
    ctx->denoise = nullptr;
}

void trc_denoise_invalidate(trc_ctx* ctx) {
    if (!ctx || !ctx->denoise) return;
    ctx->denoise->gb_valid = false;
    ctx->denoise->have_hist = false;
}

// the snapshots and the motion plane (tracking switched off), or the snapshots alone (the scene goes: another vertex count, another primitive section)
static void motion_free(trc_ctx* ctx, bool plane_too) {
    DenoiseState* s = ctx->denoise;
    if (!s || (!s->snap && !s->psnap && !(plane_too && s->motion))) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(s->snap); s->snap = nullptr; s->snap_n = 0; s->snap_live = false;
    (void)hipFree(s->psnap); s->psnap = nullptr; s->psnap_dwords = 0;
    if (plane_too) { (void)hipFree(s->motion); s->motion = nullptr; s->motion_ready = s->motion_zero = false; }
}
void trc_denoise_scene_released(trc_ctx* ctx) { if (ctx) motion_free(ctx, false); }

static uint32_t primitive_section_dwords(const trc_ctx* ctx) { return ctx->ks.sc.off_materials - ctx->ks.sc.off_spheres; }
static bool scene_has_vertices(const trc_ctx* ctx) { return ctx->n_vertex != 0 && ctx->d_verts; }

// Tracking on: the surfaces moved (or their normals, or the tree), and the temporal pass follows them -- the G-buffer is stale, the
// history stays.  The first call since the last trc_denoise that moves geometry (vertices or analytic primitives) finds all of it as that
// trc_denoise saw it: the vertex positions and the blob's primitive section go into the snapshot, on the context's stream, in front of
// whatever the caller queues next.  ONE event for both kinds: a later call of the other kind takes no second snapshot.  Without the
// snapshot buffers there is no history to keep either (trc_denoise allocates them before it leaves one)
void trc_denoise_moved(trc_ctx* ctx, bool geometry) {
    if (!ctx || !ctx->denoise) return;
    DenoiseState* s = ctx->denoise;
    const uint32_t prim_dwords = primitive_section_dwords(ctx);
    const bool buffers = (!scene_has_vertices(ctx) || (s->snap && s->snap_n == ctx->n_vertex)) && (prim_dwords == 0 || (s->psnap && s->psnap_dwords == prim_dwords));
    if (!ctx->track_motion || (geometry && !buffers)) { trc_denoise_invalidate(ctx); return; }
    s->gb_valid = false;
    if (!geometry || s->snap_live) return;
    if (scene_has_vertices(ctx))
        hipLaunchKernelGGL(k_snapshot_positions, dim3((s->snap_n + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(ctx->d_verts), s->snap_n, s->snap);
    if (prim_dwords != 0)
        (void)hipMemcpyAsync(s->psnap, ctx->d_blob + ctx->ks.sc.off_spheres, (size_t)prim_dwords * 4, hipMemcpyDeviceToDevice, ctx->stream);
    s->snap_live = true;
}

static trc_status denoise_alloc(trc_ctx* ctx) {
    if (ctx->denoise && ctx->denoise->W == ctx->width && ctx->denoise->H == ctx->height) return TRC_OK;
    trc_denoise_release(ctx);
    DenoiseState* s = new (std::nothrow) DenoiseState;
    if (!s) return trc_fail(ctx, TRC_ERR_OOM, "trc_denoise: state");
    ctx->denoise = s;
    s->W = ctx->width; s->H = ctx->height;
    const size_t plane = (size_t)s->W * s->H * sizeof(float4);
    for (float4** b : {&s->gb[0], &s->gb[1]}) HIP_TRY(ctx, hipMalloc((void**)b, 2 * plane));
    for (float4** b : {&s->hist_col[0], &s->hist_col[1], &s->hist_mom[0], &s->hist_mom[1], &s->integ, &s->tmp[0], &s->tmp[1], &s->out})
        HIP_TRY(ctx, hipMalloc((void**)b, plane));
    return TRC_OK;
}

static trc_status motion_alloc(trc_ctx* ctx) {
    DenoiseState* s = ctx->denoise;
    if (!s->motion) {
        if (hipMalloc((void**)&s->motion, (size_t)s->W * s->H * sizeof(float4)) != hipSuccess) { s->motion = nullptr; (void)hipGetLastError(); return trc_fail(ctx, TRC_ERR_OOM, "trc_denoise: motion plane"); }
        s->motion_zero = false;
    }
    if (s->snap && s->snap_n != ctx->n_vertex) motion_free(ctx, false);
    if (!s->snap && ctx->n_vertex != 0 && ctx->d_verts) {
        if (hipMalloc((void**)&s->snap, (size_t)ctx->n_vertex * sizeof(float4)) != hipSuccess) { s->snap = nullptr; (void)hipGetLastError(); return trc_fail(ctx, TRC_ERR_OOM, "trc_denoise: vertex snapshot"); }
        s->snap_n = ctx->n_vertex; s->snap_live = false;
    }
    const uint32_t prim_dwords = primitive_section_dwords(ctx);
    if (s->psnap && s->psnap_dwords != prim_dwords) motion_free(ctx, false);
    if (!s->psnap && prim_dwords != 0) {
        if (hipMalloc((void**)&s->psnap, (size_t)prim_dwords * 4) != hipSuccess) { s->psnap = nullptr; (void)hipGetLastError(); return trc_fail(ctx, TRC_ERR_OOM, "trc_denoise: primitive snapshot"); }
        s->psnap_dwords = prim_dwords; s->snap_live = false;
    }
    return TRC_OK;
}

static uint32_t log2_pow2(uint32_t v) { uint32_t k = 0; while ((1u << k) < v) ++k; return k; }

extern "C" {

void trc_denoise_default_params(trc_denoise_params* out) {
    if (!out) return;
    out->flags = 0;
    out->iterations = 5;
    out->alpha_color = 0.1f;
    out->alpha_moments = 0.2f;
    out->sigma_z = 1.0f;
    out->normal_exponent = 128;
    out->sigma_l = 4.0f;
    out->min_history = 4;
}

trc_status trc_denoise(trc_ctx* ctx, const trc_denoise_params* prm) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !prm) return TRC_ERR_INVALID_ARG;
    if (ctx->grouped()) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_denoise: composed multi-rank frames are not denoised");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_denoise before trc_resize");
    if (!ctx->has_scene || !ctx->has_camera) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_denoise before trc_upload_scene / trc_set_camera");
    if (ctx->guide_rays && !ctx->d_cam_rays)      // before anything of the state is touched: the history stays
        return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_denoise: trc_denoise_guide_rays is on and no camera rays are in force (trc_upload_camera_rays / trc_generate_camera_rays)");
    const uint32_t e = prm->normal_exponent;
    if ((prm->flags & ~TRC_DENOISE_DEMODULATE) || prm->iterations > TRC_DENOISE_MAX_ITERATIONS ||
        !(prm->alpha_color > 0.0f && prm->alpha_color <= 1.0f) || !(prm->alpha_moments > 0.0f && prm->alpha_moments <= 1.0f) ||
        !(prm->sigma_z > 0.0f && prm->sigma_z < kInf) || !(prm->sigma_l > 0.0f && prm->sigma_l < kInf) ||
        e == 0 || e > 1024 || (e & (e - 1)) || prm->min_history < 1 || prm->min_history > 64)
        return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_denoise: parameter out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { const trc_status as = denoise_alloc(ctx); if (as != TRC_OK) { trc_denoise_release(ctx); return as; } }
    DenoiseState* s = ctx->denoise;
    if (ctx->track_motion) {                    // what tracking owns: the plane, and the snapshot the next moving call fills
        const trc_status ms = motion_alloc(ctx);
        if (ms != TRC_OK) { trc_denoise_release(ctx); return ms; }
    }
    trc_sppm_order_after_camera(ctx);          // the SPPM camera stream may still be writing the accumulator

    DnParams p{};
    p.W = s->W; p.H = s->H;
    p.demod = (prm->flags & TRC_DENOISE_DEMODULATE) ? 1u : 0u;
    p.nsq = log2_pow2(e);
    p.alpha_c = prm->alpha_color; p.alpha_m = prm->alpha_moments; p.sigma_z = prm->sigma_z; p.sigma_l = prm->sigma_l;
    p.min_hist = prm->min_history;
    const dim3 grid((s->W + 7) / 8, (s->H + 7) / 8), block(64);

    // G-buffer, lazily: only for another scene, camera or frame size -- under trc_denoise_guide_rays for another scene, frame size or
    // generation of the ray sets, and not for another camera: the rays hold their own
    const bool guide = ctx->guide_rays;
    const bool rebuild = !s->gb_valid || (guide ? s->gb_ray_gen != ctx->ray_gen : std::memcmp(&s->gb_cam, &ctx->cam, sizeof(DCamera)) != 0);
    // ... and a history made under other ray sets is dropped, whatever their bits: the tap (x, y) below is the rays' own pixel
    if (guide && s->have_hist && s->hist_ray_gen != ctx->ray_gen) s->have_hist = false;
    // a snapshot in force: a moving call filled it since the last trc_denoise, so the G-buffer is stale and this call rebuilds it
    const bool motion = ctx->track_motion && s->snap_live && rebuild;
    if (rebuild) {
        s->gb_cur ^= 1;
        const size_t lds = trc_dyn_lds_bytes(ctx, true);
        const DnCam cam = dn_cam(ctx->cam);
        TexTable tt{};
        if (ctx->tex_active()) { tt.texels = ctx->d_tex_texels; tt.desc = ctx->d_tex_desc; tt.n = ctx->n_tex; }      // an active image texture (trc_upload_textures): the albedo plane samples it
        const KMotion mo{ctx->d_idx, s->snap, s->psnap, s->motion};
        const float4* const rays = guide ? reinterpret_cast<const float4*>(ctx->d_cam_rays) : nullptr;      // set 0
        if (ctx->lds_scene) launch_gbuffer<true>(ctx->tex_active(), motion, guide, ctx->stream, grid, lds, ctx->ks, cam, s->W, s->H, s->gb[s->gb_cur], tt, mo, rays);
        else launch_gbuffer<false>(ctx->tex_active(), motion, guide, ctx->stream, grid, lds, ctx->ks, cam, s->W, s->H, s->gb[s->gb_cur], tt, mo, rays);
        if (motion) s->motion_zero = false;
        HIP_TRY(ctx, hipGetLastError());
        s->gb_cam = ctx->cam;
        s->gb_ray_gen = ctx->ray_gen;
        s->gb_valid = true;
    }

    KTemporal kt{};
    kt.p = p;
    kt.cur = dn_cam(ctx->cam);
    kt.prev = s->hist_cam;
    kt.have_prev = s->have_hist ? 1u : 0u;
    kt.same_cam = (s->have_hist && (guide || same_dn_cam(kt.cur, s->hist_cam))) ? 1u : 0u;      // guide: the history's rays are this frame's (above)
    kt.guide = guide ? 1u : 0u;
    kt.accum = reinterpret_cast<const float4*>(ctx->d_accum);
    kt.gb = s->gb[s->gb_cur];
    kt.gb_prev = rebuild ? s->gb[s->gb_cur ^ 1] : s->gb[s->gb_cur];
    kt.hist_col = s->hist_col[s->hist_cur];
    kt.hist_mom = s->hist_mom[s->hist_cur];
    const int nh = s->hist_cur ^ 1;
    kt.integ = s->integ;
    kt.mom = s->hist_mom[nh];
    if (ctx->track_motion && !motion && !s->motion_zero) {      // no snapshot in force: the plane of this call is all zero
        HIP_TRY(ctx, hipMemsetAsync(s->motion, 0, (size_t)s->W * s->H * sizeof(float4), ctx->stream));
        s->motion_zero = true;
    }
    kt.motion = s->motion;
    if (motion && s->have_hist) hipLaunchKernelGGL(k_svgf_temporal<true>, grid, block, 0, ctx->stream, kt);
    else hipLaunchKernelGGL(k_svgf_temporal<false>, grid, block, 0, ctx->stream, kt);
    HIP_TRY(ctx, hipGetLastError());
    s->snap_live = false;                       // in force for this call, and no longer
    s->motion_ready = ctx->track_motion;

    const uint32_t K = prm->iterations;
    if (K == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(s->hist_col[nh], s->integ, (size_t)s->W * s->H * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_svgf_finish, grid, block, 0, ctx->stream, p, (const float4*)s->integ, (const float4*)kt.gb, kt.accum, s->out);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        const float4* src = s->integ;
        for (uint32_t it = 0; it < K; ++it) {
            KAtrous ka{};
            ka.p = p;
            ka.step = 1u << it;
            ka.src = src;
            ka.gb = kt.gb;
            ka.accum = kt.accum;
            ka.dst = it == 0 ? s->hist_col[nh] : (it + 1 == K ? nullptr : s->tmp[it & 1]);
            ka.final_out = it + 1 == K ? s->out : nullptr;
            hipLaunchKernelGGL(k_svgf_atrous, grid, block, 0, ctx->stream, ka);
            HIP_TRY(ctx, hipGetLastError());
            src = ka.dst;
        }
    }
    s->hist_cur = nh;
    s->have_hist = true;
    s->hist_cam = kt.cur;
    s->hist_ray_gen = ctx->ray_gen;
    s->has_output = true;
    return TRC_OK;
}

static trc_status denoise_download(trc_ctx* ctx, void* host, const void* dev, size_t bytes) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(trc_copy_to_host(ctx, host, dev, bytes, ctx->stream));
    return TRC_OK;
}

static trc_status denoise_ready(trc_ctx* ctx, const char* what) {
    if (!ctx->d_accum || !ctx->denoise || !ctx->denoise->has_output) return trc_fail(ctx, TRC_ERR_NO_FRAME, std::string(what) + " before trc_denoise");
    return TRC_OK;
}

trc_status trc_download_denoised(trc_ctx* ctx, float* rgba) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !rgba) return TRC_ERR_INVALID_ARG;
    TRC_TRY(denoise_ready(ctx, "trc_download_denoised"));
    return denoise_download(ctx, rgba, ctx->denoise->out, (size_t)ctx->width * ctx->height * sizeof(float4));
}

trc_status trc_tonemap_denoised(trc_ctx* ctx, uint8_t* rgba8, float* exposure_out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !rgba8) return TRC_ERR_INVALID_ARG;
    TRC_TRY(denoise_ready(ctx, "trc_tonemap_denoised"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_tonemap_plane(ctx, reinterpret_cast<const float*>(ctx->denoise->out), rgba8, exposure_out);
}

trc_status trc_download_gbuffer(trc_ctx* ctx, trc_gbuffer_texel* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    TRC_TRY(denoise_ready(ctx, "trc_download_gbuffer"));
    static_assert(sizeof(trc_gbuffer_texel) == 2 * sizeof(float4), "one texel = the two float4 of the G-buffer planes");
    return denoise_download(ctx, out, ctx->denoise->gb[ctx->denoise->gb_cur], (size_t)ctx->width * ctx->height * sizeof(trc_gbuffer_texel));
}

trc_status trc_denoise_track_motion(trc_ctx* ctx, int on) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    const bool want = on != 0;
    if (want == ctx->track_motion) return TRC_OK;
    ctx->track_motion = want;
    if (!ctx->denoise) return TRC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->denoise->have_hist = false;            // either way: the next frame has n = 1 everywhere
    ctx->denoise->snap_live = false;
    if (!want) motion_free(ctx, true);
    return TRC_OK;
}

trc_status trc_denoise_guide_rays(trc_ctx* ctx, int on) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    const bool want = on != 0;
    if (want == ctx->guide_rays) return TRC_OK;
    ctx->guide_rays = want;
    trc_denoise_invalidate(ctx);                // either way: another G-buffer ray, and the next frame has n = 1 everywhere
    return TRC_OK;
}

trc_status trc_download_motion(trc_ctx* ctx, trc_motion_texel* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    if (!ctx->track_motion || !ctx->d_accum || !ctx->denoise || !ctx->denoise->motion || !ctx->denoise->motion_ready)
        return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_download_motion before a trc_denoise with tracking on (trc_denoise_track_motion)");
    static_assert(sizeof(trc_motion_texel) == sizeof(float4), "one texel = one float4 of the motion plane");
    return denoise_download(ctx, out, ctx->denoise->motion, (size_t)ctx->width * ctx->height * sizeof(trc_motion_texel));
}

trc_status trc_download_history_length(trc_ctx* ctx, float* n) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !n) return TRC_ERR_INVALID_ARG;
    TRC_TRY(denoise_ready(ctx, "trc_download_history_length"));
    const DenoiseState* s = ctx->denoise;
    const size_t px = (size_t)ctx->width * ctx->height;
    std::vector<float4> moments(px);            // (mu1, mu2, n, 0) per pixel: the third of each is what the caller gets
    TRC_TRY(denoise_download(ctx, moments.data(), s->hist_mom[s->hist_cur], px * sizeof(float4)));
    for (size_t i = 0; i < px; ++i) n[i] = moments[i].z;
    return TRC_OK;
}

trc_status trc_denoise_reset(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (ctx->denoise) ctx->denoise->have_hist = false;
    return TRC_OK;
}

#ifdef TRC_TEST_HOOKS
trc_status trc_debug_denoise_state(trc_ctx* ctx, float* integrated, float* history, float* moments) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    TRC_TRY(denoise_ready(ctx, "trc_debug_denoise_state"));
    const DenoiseState* s = ctx->denoise;
    const size_t bytes = (size_t)ctx->width * ctx->height * sizeof(float4);
    const void* src[3] = {s->integ, s->hist_col[s->hist_cur], s->hist_mom[s->hist_cur]};
    void* dst[3] = {integrated, history, moments};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) TRC_TRY(denoise_download(ctx, dst[k], src[k], bytes));
    return TRC_OK;
}
#endif

}  // extern "C"
