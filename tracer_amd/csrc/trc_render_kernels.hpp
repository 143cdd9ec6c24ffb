// trc_render_kernels.hpp -- kernelPathTracing (RT_Metal/Metal/Render.metal:495-558) as HIP kernels: DEFINITIONS.  Included by the
// five translation units that instantiate them through their kernel tables (render_kernels below; trc_render_config.hpp says which
// and why); trc_render_pass.hip only launches them.
#pragma once

#include <hip/hip_runtime.h>

#include "trc_render_config.hpp"

// the per-triangle-material twins (TRC_TRIANGLE_MATERIALS 1: trc_render_*_tm.hip) are the same kernels and tables in namespace trimat
#if TRC_TRIANGLE_MATERIALS
#define TRC_RENDER_NS_BEGIN namespace trimat {
#define TRC_RENDER_NS_END }
#else
#define TRC_RENDER_NS_BEGIN
#define TRC_RENDER_NS_END
#endif
TRC_RENDER_NS_BEGIN

// One pixel block (8x8 pixels on 64 lanes, or 4x4 on 16) of kernelPathTracing: all `spp` samples of every pixel, RNG texel
// and accumulator read and written once.  `slot` = position of the block in the launch order; `stack` / `lvstack` / `ovf` =
// this lane's columns of the wavefront's traversal stack.  Shared by k_render (one block per one-wavefront workgroup) and
// k_render_pwg (wavefronts of a persistent workgroup pulling blocks from a queue).
//
// PARK = 8 | 10 (k_render_pwg on trees read from memory, k_render_dense): the values a lane touches only where a sample begins or ends
// -- the running mean, (u, v), the sample counter, with 10 rows the pixel's coordinates -- and the two work counters live in PARK words
// of the lane's LDS column `park` (row r at park[r * kBlock]) instead of registers: that many values fewer to carry through the walk and
// the shading code of every iteration, i.e. fewer spills to scratch -- which on a mesh scene streams through the L2 the node fetches
// live in, and on the LDS-resident headline scene are issue slots.  Same loads, same arithmetic, same stores per lane.
// TEX: image textures (trc_upload_textures; hit_color<true>): instantiated only for what a scene with an active image launches --
// the production kernels under the PCG sampler (k_render_tex, k_render_strip_tex, k_render_pwg_tex) -- so the others stay as they are.
template <bool TEX, class CX>
__device__ __forceinline__ void set_ctx_tex(CX& cx, const KRender& kp) {       // TEX: the image table of the launch (PathCtxTex)
    if constexpr (TEX) { cx.tex.texels = kp.tex_texels; cx.tex.desc = kp.tex_desc; cx.tex.n = kp.n_tex; }
}
// LIGHT (dev_integrator.hpp: Light; traceMIS): the environment map (TRC_FLAG_ENV_LIGHT) or the mesh's emissive triangles
// (TRC_FLAG_MESH_LIGHTS) are lights too (mis_step<.., LIGHT>); `tables` = that light's sampling tables, null without one
template <Light LIGHT, class CX>
__device__ __forceinline__ void set_ctx_light(CX& cx, const LightTables<LIGHT>* tables) {
    if constexpr (LIGHT != Light::None) cx.light = *tables;
}
// What a path reads of the launch, the same for every pixel of a kernel.  The call sites add what differs between them: cx.S.ovf, and
// (SOBOL) the pixel in cx.sobol_xy.
template <bool SOBOL, bool TEX, Light LIGHT>
__device__ __forceinline__ void fill_path_ctx(PathCtxOf<TEX, LIGHT>& cx, const KRender& kp, const DScene& sc, const uint32_t* small_base,
                                              uint32_t* stack, uint32_t* lvstack, const LightTables<LIGHT>* tables) {
    cx.S = make_scene_ref(sc, small_base);
    cx.root_min = f3(kp.ks.root_box[0], kp.ks.root_box[1], kp.ks.root_box[2]);
    cx.root_max = f3(kp.ks.root_box[3], kp.ks.root_box[4], kp.ks.root_box[5]);
    cx.sh.mats = small_base + sc.off_materials;
    set_ctx_tex<TEX>(cx, kp);
    set_ctx_light<LIGHT>(cx, tables);
    cx.ambient = f3(kp.ambient[0], kp.ambient[1], kp.ambient[2]);
    cx.env.rgb = kp.env_rgb; cx.env.w = kp.env_w; cx.env.h = kp.env_h;
    cx.stack = stack;
    cx.lvstack = lvstack;
    cx.max_depth = kp.max_depth;
    cx.density = kp.density;
    cx.dinfo = kp.dinfo;
    cx.occupancy = kp.occupancy;
    if (SOBOL) {                                       // SobolSampler(rng, frame, thread_pos, vsize), SobolSampler.hh:50-61
        cx.sobol32 = kp.sobol32; cx.sobol_vdc = kp.sobol_vdc;
        cx.sobol_m = kp.sobol_m; cx.sobol_res = 1u << kp.sobol_m;
    }
}
// MEMO = 7 | 8 | 10 (round 8, tracePath production kernels; trc_render_config.hpp: primary replay): the hit of the pixel's camera ray, kept
// after the block's first walk in MEMO words of the lane's column `memo` (LDS or global rows).  A later sample whose camera ray has the
// same origin bits -- the direction follows from (origin, u, v, camera) -- takes its record from there: no walk, and (kp.replay lanes) it is
// shaded before the wavefront's next walk, so that a lane needs one trip round the loop per BOUNCE ray.  The ray is still counted
// (trc_stats.rays is the algorithm's Scene::hit count); what was answered from the memo is summed into kStatReplays.
template <bool LDS, bool STATS, int INTEGRATOR, bool SOBOL, bool HYB, int PARK = 0, bool TEX = false, Light LIGHT = Light::None, int MEMO = 0, class COUNT = uint32_t>
__device__ __forceinline__ void render_block(const KRender& kp, const DScene& sc, const uint32_t* small_base, uint32_t* stack, uint32_t* lvstack,
                                             uint32_t* ovf, uint32_t* park, const uint32_t slot, const uint32_t lane,
                                             COUNT& n_rays, COUNT& n_shaded, uint32_t& n_paths, TravCounters& cnt,
                                             const LightTables<LIGHT>* tables = nullptr, uint32_t* memo = nullptr) {
    static_assert(MEMO == 0 || (INTEGRATOR == TRC_INTEGRATOR_PATH && !STATS && !SOBOL && LIGHT == Light::None), "primary replay: tracePath production kernels");
    static_assert(MEMO == 0 || MEMO == 10 || !TEX, "an image texture reads rec.uv: 10 memo rows");
    constexpr bool kPacked = MEMO == 7;          // material, side, tag and replay count in ONE word (trc_lds_fit.hpp), row kMemoWord
    uint32_t replays = 0;                        // camera rays of this lane answered from the memo
    const uint64_t t_start = clock64();          // this wavefront's own duration = the next launch's sort key
    const uint32_t entry = kp.order ? kp.order[slot] : slot;     // adaptive launch order / cost-adaptive block size (trc_render)
    const uint32_t index = entry & kLaunchIndexMask, code = entry >> kLaunchCodeShift;
    if (index >= kp.n_tiles) return;                            // padding of the launch list's part region (k_pad_launch)
    const uint32_t tile = kp.tiles[index];                      // pixel block: x | y << 16 in units of the block edge
    // 3: 8x8 pixels, all 64 lanes; 2: 4x4 pixels, lanes 0..15; 1: 2x2 pixels, lanes 0..3; 0: one pixel, lane 0 -- the whole list
    // (kp.blk_shift), or a part of an 8x8 block whose previous launch ran long (trc_ctx.hpp: launch codes)
    const uint32_t part = code >= 21u ? (code - 21u) >> 2 : (code >= 5u ? code - 5u : 0u);      // sixteenth 0..15
    const uint32_t quarter = code >= 5u ? part >> 2 : (code ? code - 1u : 0u);
    const uint32_t bs = code >= 21u ? 0u : (code >= 5u ? 1u : (code ? 2u : kp.blk_shift));
    const uint32_t pixel = code >= 21u ? (code - 21u) & 3u : 0u;
    const uint32_t qx = code ? ((quarter & 1u) << 2) + (code >= 5u ? (part & 1u) << 1 : 0u) + (pixel & 1u) : 0u;
    const uint32_t qy = code ? ((quarter >> 1) << 2) + (code >= 5u ? ((part >> 1) & 1u) << 1 : 0u) + (pixel >> 1) : 0u;
    const uint32_t px = ((tile & 0xFFFFu) << kp.blk_shift) + qx + (lane & ((1u << bs) - 1u));
    const uint32_t py = ((tile >> 16) << kp.blk_shift) + qy + (lane >> bs);
    const uint32_t W = kp.fr.width, H = kp.fr.height;
    const bool active = lane < (1u << (2u * bs)) && px < W && py < H;
    const uint32_t canon = index * kp.cost_stride + (code ? code - 1u : 0u);

    if (active) {
        PathCtxOf<TEX, LIGHT> cx;
        fill_path_ctx<SOBOL, TEX, LIGHT>(cx, kp, sc, small_base, stack, lvstack, tables);
        cx.S.ovf = ovf;
        if (SOBOL) { cx.sobol_xy[0] = px; cx.sobol_xy[1] = py % kp.view_height; }

        // the values that are touched only where a sample begins or ends: registers, or (PARK) rows of the lane's LDS column
        F3 cached_r = f3(0);
        float u_r = 0, v_r = 0;
        uint32_t s_r = 0;
        size_t pix_r = 0;
        auto row_f = [&](uint32_t r) { return __uint_as_float(park[r * kBlock]); };
        auto put_f = [&](uint32_t r, float x) { park[r * kBlock] = __float_as_uint(x); };
        auto get_cached = [&]() { if constexpr (PARK) return f3(row_f(kParkCachedX), row_f(kParkCachedY), row_f(kParkCachedZ)); else return cached_r; };
        auto set_cached = [&](F3 c) { if constexpr (PARK) { put_f(kParkCachedX, c.x); put_f(kParkCachedY, c.y); put_f(kParkCachedZ, c.z); } else cached_r = c; };
        auto get_sample = [&]() { if constexpr (PARK) return park[kParkSample * kBlock]; else return s_r; };
        auto set_sample = [&](uint32_t s) { if constexpr (PARK) park[kParkSample * kBlock] = s; else s_r = s; };
        uint4 texel;
        {
            const size_t pix = (size_t)py * W + px;
            texel = reinterpret_cast<const uint4*>(kp.fr.rng)[pix];       // r, g, b, a
            const float4 acc = reinterpret_cast<const float4*>(kp.fr.accum)[pix];
            const float u = (float)px / (float)W;                               // no sub-pixel jitter (B-2)
            const float v = (float)(py % kp.view_height) / (float)kp.view_height;      // one view: view_height == H
            set_cached(f3(acc.x, acc.y, acc.z));
            set_sample(0u);
            if constexpr (PARK) { put_f(kParkU, u); put_f(kParkV, v); }
            if constexpr (PARK >= 10) { park[kParkPx * kBlock] = px; park[kParkPy * kBlock] = py; }
            else { u_r = u; v_r = v; pix_r = pix; }
        }

        PathState ps;
        Pcg rng;
        uint64_t state_after_cast = 0;       // SOBOL: the sampler draws from a copy, the texel keeps this (SobolSampler.hh:50)
        // MEMO: `first` -- the lane's next walk is its first of the block, the camera ray of the launch's first sample: its result is kept;
        // `have` -- ps.rec already holds the hit of ps.ray (taken from the memo by begin_sample); `terminal` -- the memoised camera ray
        // ends the sample by itself (it escapes, or meets an emitter): its radiance, a function of the ray alone, is in the memo too.
        // The memo never outlives the block.
        const bool replay_on = MEMO != 0 && kp.replay != 0u;
        bool first = replay_on, have = false, terminal = false;
        auto memo_f = [&](uint32_t r) { return __uint_as_float(memo[r * kBlock]); };
        auto at_eye = [&](const F3& o) {      // bits, not values: a NaN offset or a zero of the other sign is another ray
            return __float_as_uint(o.x) == __float_as_uint(kp.cam.lookFrom[0]) && __float_as_uint(o.y) == __float_as_uint(kp.cam.lookFrom[1]) &&
                   __float_as_uint(o.z) == __float_as_uint(kp.cam.lookFrom[2]);
        };
        // castRay, then (SOBOL) the sampler of this frame: Render.metal:527-530
        auto begin_sample = [&](uint32_t s) {
            const float u = PARK ? row_f(kParkU) : u_r, v = PARK ? row_f(kParkV) : v_r;
            path_begin(ps, cast_ray(kp.cam, u, v, rng), kp.max_depth);
            if constexpr (MEMO != 0) {
                if (replay_on && s != 0u) {
                    const uint32_t mat = memo[(kPacked ? kMemoWord : kMemoMat) * kBlock];
                    if (kPacked ? !trc_memo_is_none(mat) : mat != kMemoNone) {
                        if (at_eye(ps.ray.o)) {                 // the memoised ray: its record, as Scene::hit left it for the integrator
                            const uint32_t tag = kPacked ? (trc_memo_is_ends(mat) ? kTagNone : (trc_memo_tag_type(mat) << kTagIndexBits) | trc_memo_tag_index(mat))
                                                         : memo[kMemoTag * kBlock];
                            if (tag == kTagNone) terminal = true;
                            else {
                                ps.rec.p = f3(memo_f(kMemoPx), memo_f(kMemoPy), memo_f(kMemoPz));
                                ps.rec.gn = f3(memo_f(kMemoNx), memo_f(kMemoNy), memo_f(kMemoNz));
                                ps.rec.sn = (kPacked ? trc_memo_same_side(mat) : (mat & kMemoSameSide) != 0u) ? ps.rec.gn : -ps.rec.gn;
                                ps.rec.material = kPacked ? trc_memo_material(mat) : mat & ~kMemoSameSide;
                                ps.rec.tag = tag;
                                if constexpr (MEMO >= 10) { ps.rec.uv.x = memo_f(kMemoU); ps.rec.uv.y = memo_f(kMemoV); }
                                have = true;
                            }
                            bump(n_rays);                       // still one Scene::hit of the algorithm
                        } else {                                // another ray (a lens): the pixel walks from here on; s - 1 samples replayed
                            if constexpr (kPacked) memo[kMemoWord * kBlock] = trc_memo_pack_none(s - 1u);
                            else { memo[kMemoMat * kBlock] = kMemoNone; memo[kMemoTag * kBlock] = s - 1u; }
                        }
                    }
                }
            }
            if (SOBOL) {
                state_after_cast = rng.state;
                ps.sobol_index = sobol_interval_to_index(cx, (uint64_t)(kp.frame0 + s));
                ps.sobol_dim = 0;
            }
        };
        bool alive = kp.spp > 0;
        if (alive) {
            // pcg32_t rng = { rng_inc, rng_state } aggregate-initialises {state, inc}: the two 64-bit
            // words trade roles every frame (Render.metal:516-519,545-557, B-1)
            rng.state = ((uint64_t)texel.z << 32) | texel.w;
            rng.inc = ((uint64_t)texel.x << 32) | texel.y;
            begin_sample(0u);
        }
        // end of a sample: accumulate, hand the RNG words back to the texel, start the next sample (or stop)
        auto finish_sample = [&](F3 color) {
            ProfScope<STATS> scope(cnt, kProfFinish);
            for (;;) {
                const bool bad = is_inf(color.x) || is_nan(color.x) || is_inf(color.y) || is_nan(color.y) ||
                                 is_inf(color.z) || is_nan(color.z);
                if (bad) color = f3(0);                                         // :537-538
                uint32_t s = get_sample();
                const uint32_t frame = kp.frame0 + s;
                set_cached(div_shared(get_cached() * (float)frame + color, (float)(frame + 1)));  // running mean, :540-541
                if (SOBOL) rng.state = state_after_cast;
                // PARK: the texel is not carried through the loop -- the last sample's write-back is the RNG's own words (below)
                if constexpr (!PARK) {
                    texel.y = (uint32_t)rng.state; texel.x = (uint32_t)(rng.state >> 32);
                    texel.w = (uint32_t)rng.inc;   texel.z = (uint32_t)(rng.inc >> 32);
                    n_paths++;
                }
                ++s;
                set_sample(s);
                if (s == kp.spp) {
                    alive = false;
                } else {
                    if constexpr (PARK) { const uint64_t t = rng.state; rng.state = rng.inc; rng.inc = t; }      // the words trade roles (B-1)
                    else {
                        rng.state = ((uint64_t)texel.z << 32) | texel.w;
                        rng.inc = ((uint64_t)texel.x << 32) | texel.y;
                    }
                    begin_sample(s);
                }
                if constexpr (MEMO != 0) {      // a sample that its memoised camera ray ends: the same radiance again, and on to the next one
                    if (terminal) { terminal = false; color = f3(memo_f(kMemoPx), memo_f(kMemoPy), memo_f(kMemoPz)); continue; }
                }
                break;
            }
        };
        // what the integrator reads of the first walk's result goes to the memo -- if the ray left the eye itself, and the record fits the
        // rows.  Returns whether the ray ends its sample by itself: its radiance then follows the step (the rows of p)
        auto memo_store = [&](bool hitted) {
            uint32_t mat = kMemoNone, tag = 0u;                  // no record: the tag word counts the replays so far
            bool ends = false;
            if (at_eye(ps.ray.o)) {
                ends = !hitted || mat_type(cx.sh, ps.rec.material) == kMatDiffuse;         // path_step: :434-445
                if (ends) { mat = 0u; tag = kTagNone; }
                else {
                    // 8 rows have no room for uv, which only a checker texture on a cube or a triangle reads (hit_color): such a hit is not kept
                    const bool uv_read = MEMO < 10 && (ps.rec.tag >> kTagIndexBits) >= 2u && mat_tex(cx.sh, ps.rec.material) == kTexChecker;
                    const bool fits = kPacked ? trc_memo_packable(ps.rec.material, ps.rec.tag >> kTagIndexBits, ps.rec.tag & kTagIndexMask)
                                              : ps.rec.material < kMemoSameSide - 1u;
                    if (!uv_read && fits) {
                        const bool same = __float_as_uint(ps.rec.sn.x) == __float_as_uint(ps.rec.gn.x);      // sn is gn or -gn (check_face)
                        mat = ps.rec.material | (same ? kMemoSameSide : 0u); tag = ps.rec.tag;
                        memo[kMemoPx * kBlock] = __float_as_uint(ps.rec.p.x); memo[kMemoPy * kBlock] = __float_as_uint(ps.rec.p.y);
                        memo[kMemoPz * kBlock] = __float_as_uint(ps.rec.p.z);
                        memo[kMemoNx * kBlock] = __float_as_uint(ps.rec.gn.x); memo[kMemoNy * kBlock] = __float_as_uint(ps.rec.gn.y);
                        memo[kMemoNz * kBlock] = __float_as_uint(ps.rec.gn.z);
                        if constexpr (MEMO >= 10) { memo[kMemoU * kBlock] = __float_as_uint(ps.rec.uv.x); memo[kMemoV * kBlock] = __float_as_uint(ps.rec.uv.y); }
                    }
                }
            }
            if constexpr (kPacked) {
                memo[kMemoWord * kBlock] = mat == kMemoNone ? trc_memo_pack_none(0u) : tag == kTagNone ? trc_memo_pack_ends()
                                         : trc_memo_pack_hit(mat & ~kMemoSameSide, (mat & kMemoSameSide) != 0u, tag >> kTagIndexBits, tag & kTagIndexMask);
            } else { memo[kMemoMat * kBlock] = mat; memo[kMemoTag * kBlock] = tag; }
            return ends;
        };
        // flat loop: one Scene::hit per iteration; a finished path immediately regenerates the next sample
        uint32_t drained = 0;                                   // MEMO: trips in a row that shaded replayed hits only (wave-uniform)
        while (alive) {
            ProfScope<STATS> loop_scope(cnt, kProfLoop);
            constexpr bool kVolume = INTEGRATOR == TRC_INTEGRATOR_VOLUME;
            constexpr int kDefer = STATS ? 0 : (LDS ? TRC_DEFER_LDS : TRC_DEFER_GLOBAL);      // dev_intersect.hpp: trav_test_leaf
            bool hitted = true;                                  // (a replayed hit in hand is a hit: a memoised miss ends in finish_sample)
            // MEMO: a lane that holds a replayed hit has nothing to walk.  Where at least kp.replay lanes of the wavefront do, this trip shades
            // them alone -- they are then level with the lanes whose ray is a bounce, one trip per BOUNCE ray -- but no more than
            // kp.replay_chain such trips in a row (every one costs the whole wavefront a shading pass); otherwise those lanes sit out the walk
            // and are shaded with everybody.  Wave-uniform decisions; which trip shades a lane changes nothing the lane computes.
            bool drain = false, ends = false;
            if constexpr (MEMO != 0) {
                drain = (uint32_t)__popcll(__ballot(have)) >= kp.replay && drained < kp.replay_chain && replay_on;
                drained = drain ? drained + 1u : 0u;
            }
            if (!drain && !have && !(kVolume && TRC_TRACK_SLICE > 0 && ps.tracking)) {       // a lane between two slices of its delta tracker has no ray to trace
                bump(n_rays);
                hitted = scene_hit<LDS, STATS, false, false, kVolume, HYB, kDefer>(cx.S, cx.root_min, cx.root_max, ps.ray, ps.rec, FLT_MAX,
                                                                                  cx.stack, cx.lvstack, cnt);
                if constexpr (MEMO != 0) {
                    if (first) { ends = memo_store(hitted); first = false; }
                }
            }
            if (!drain || have) {
                have = false;
                F3 color;
                const bool finished = (INTEGRATOR == TRC_INTEGRATOR_PATH)
                                          ? path_step<STATS, SOBOL, TEX>(cx, ps, hitted, rng, cnt, n_shaded, color)
                                          : mis_step<LDS, STATS, kVolume, SOBOL, HYB, TEX, LIGHT>(cx, ps, hitted, rng, cnt, n_rays, n_shaded, color);
                if constexpr (MEMO != 0) {
                    if (ends) { memo[kMemoPx * kBlock] = __float_as_uint(color.x); memo[kMemoPy * kBlock] = __float_as_uint(color.y); memo[kMemoPz * kBlock] = __float_as_uint(color.z); }
                }
                if (finished) finish_sample(color);
            }
        }
        if constexpr (MEMO != 0) {      // a column that still holds its record answered every sample but the first; one that lost it says how many
            if constexpr (kPacked) { if (replay_on) { const uint32_t w = memo[kMemoWord * kBlock]; replays = trc_memo_is_none(w) ? trc_memo_count(w) : kp.spp - 1u; } }
            else if (replay_on) replays = memo[kMemoMat * kBlock] != kMemoNone ? kp.spp - 1u : memo[kMemoTag * kBlock];
        }
        if constexpr (PARK) {       // the loop is left by the last finish_sample only (trc_render launches spp >= 1): what that one would
            n_paths += kp.spp;      // have put into the texel, and one finished sample per call of it
            texel.y = (uint32_t)rng.state; texel.x = (uint32_t)(rng.state >> 32);
            texel.w = (uint32_t)rng.inc;   texel.z = (uint32_t)(rng.inc >> 32);
        }
        const F3 cached = get_cached();
        size_t pix = pix_r;
        if constexpr (PARK >= 10) pix = (size_t)park[kParkPy * kBlock] * W + park[kParkPx * kBlock];
        else if constexpr (PARK != 0) {
            // 8 rows: the pixel's coordinates are not carried at all -- the launch entry is read once more (volatile: a second load, not
            // a value kept alive through the loop) and decoded as at the top.  (Written out twice: one decode function for both places,
            // tried in round 12 in four forms, changed the register allocation of every k_render / k_render_pwg kernel.)
            const uint32_t entry2 = kp.order ? *reinterpret_cast<const volatile uint32_t*>(kp.order + slot) : slot;
            const uint32_t code2 = entry2 >> kLaunchCodeShift;
            const uint32_t tile2 = *reinterpret_cast<const volatile uint32_t*>(kp.tiles + (entry2 & kLaunchIndexMask));
            const uint32_t part2 = code2 >= 21u ? (code2 - 21u) >> 2 : (code2 >= 5u ? code2 - 5u : 0u);
            const uint32_t quarter2 = code2 >= 5u ? part2 >> 2 : (code2 ? code2 - 1u : 0u);
            const uint32_t bs2 = code2 >= 21u ? 0u : (code2 >= 5u ? 1u : (code2 ? 2u : kp.blk_shift));
            const uint32_t pixel2 = code2 >= 21u ? (code2 - 21u) & 3u : 0u;
            const uint32_t qx2 = code2 ? ((quarter2 & 1u) << 2) + (code2 >= 5u ? (part2 & 1u) << 1 : 0u) + (pixel2 & 1u) : 0u;
            const uint32_t qy2 = code2 ? ((quarter2 >> 1) << 2) + (code2 >= 5u ? ((part2 >> 1) & 1u) << 1 : 0u) + (pixel2 >> 1) : 0u;
            pix = (size_t)(((tile2 >> 16) << kp.blk_shift) + qy2 + (lane >> bs2)) * W + ((tile2 & 0xFFFFu) << kp.blk_shift) + qx2 + (lane & ((1u << bs2) - 1u));
        }
        float4 out; out.x = cached.x; out.y = cached.y; out.z = cached.z; out.w = 1.0f;
        reinterpret_cast<float4*>(kp.fr.accum)[pix] = out;
        reinterpret_cast<uint4*>(kp.fr.rng)[pix] = texel;
    }

    // per SAMPLE (cost_div = 4 x spp), so that launches of different lengths speak of the same quantity
    if (lane == 0) kp.block_cost[canon] = (uint32_t)min((unsigned long long)(clock64() - t_start) / kp.cost_div, 0xFFFFFFull);
    if constexpr (MEMO != 0) {
        const uint32_t r_replays = wave_sum(replays);
        if (lane == 0 && r_replays) atomicAdd(&stat_row(kp.stats, slot)[kStatReplays], (unsigned long long)r_replays);
    }
}

// the body of k_render (one one-wavefront workgroup = one entry of the launch list)
// MEMO, MEMO_GLOBAL: the primary-replay rows (render_block) -- behind the stack and park rows of this workgroup's LDS, or rows of its own in kp.memo
template <bool LDS, bool STATS, int INTEGRATOR, bool SOBOL, int PARK = 0, bool TEX = false, Light LIGHT = Light::None, int MEMO = 0, bool MEMO_GLOBAL = false>
__device__ __forceinline__ void render_workgroup(const KRender& kp, const LightTables<LIGHT>* tables = nullptr) {
    if (kp.n_launch && blockIdx.x >= *kp.n_launch) return;      // the grid is sized for the most quarters a plan may splice in
    const DScene& sc = kp.ks.sc;
    const uint32_t* small_base = stage_scene(sc);
    uint32_t* stack = lane_stack(sc);
    uint32_t* lvstack = lane_lvstack(sc);

    const uint32_t lane = threadIdx.x;
    uint32_t n_rays = 0, n_shaded = 0, n_paths = 0;
    TravCounters cnt;
    counters_zero(cnt);
    constexpr bool kHybridStack = !LDS && !STATS && hybrid_stack(INTEGRATOR);     // plan_launch_lds
    uint32_t* ovf = kHybridStack ? kp.stack_ovf + (size_t)blockIdx.x * sc.stack_ovf_rows * kBlock + lane : nullptr;
    uint32_t* memo = nullptr;
    if constexpr (MEMO != 0 && MEMO_GLOBAL) memo = kp.memo + (size_t)blockIdx.x * MEMO * kBlock + lane;
    else if constexpr (MEMO != 0) memo = stack + (sc.stack_lds + PARK) * kBlock;
    if constexpr (PARK != 0) {                  // the park rows follow the stack rows of this one-wavefront workgroup (trc_render_pass.hip: choose_kernel)
        uint32_t* park = stack + sc.stack_lds * kBlock;
        park[kParkRays * kBlock] = 0u; park[kParkShaded * kBlock] = 0u;
        LdsCount c_rays{park + kParkRays * kBlock}, c_shaded{park + kParkShaded * kBlock};
        render_block<LDS, STATS, INTEGRATOR, SOBOL, kHybridStack, PARK, TEX, LIGHT, MEMO>(kp, sc, small_base, stack, lvstack, ovf, park, blockIdx.x, lane, c_rays, c_shaded, n_paths, cnt, tables, memo);
        n_rays = park[kParkRays * kBlock]; n_shaded = park[kParkShaded * kBlock];
    } else
    render_block<LDS, STATS, INTEGRATOR, SOBOL, kHybridStack, 0, TEX, LIGHT, MEMO>(kp, sc, small_base, stack, lvstack, ovf, nullptr, blockIdx.x, lane, n_rays, n_shaded, n_paths, cnt, tables, memo);

    // exact work counters: wave reduction, one 64-bit atomic per wave and counter
    uint32_t r_paths = wave_sum(n_paths), r_rays = wave_sum(n_rays), r_shaded = wave_sum(n_shaded);
    unsigned long long* const stats = stat_row(kp.stats, blockIdx.x);
    if (lane == 0) {
        atomicAdd(&stats[kStatPaths], (unsigned long long)r_paths);
        atomicAdd(&stats[kStatRays], (unsigned long long)r_rays);
        atomicAdd(&stats[kStatShaded], (unsigned long long)r_shaded);
    }
    if (STATS) {
        uint32_t v[8] = {cnt.n_descend, cnt.n_return, cnt.leaf[0], cnt.leaf[1], cnt.leaf[2], cnt.leaf[3],
                         cnt.hit_triangle, cnt.hit_cube};
        const int slot[8] = {kStatDescend, kStatReturn, kStatLeafSphere, kStatLeafSquare, kStatLeafCube,
                             kStatLeafTriangle, kStatHitTriangle, kStatHitCube};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t r = wave_sum(v[i]);
            if (lane == 0) atomicAdd(&stats[slot[i]], (unsigned long long)r);
        }
        for (int i = 0; i < kProfCount; ++i) {       // divergence profile: lanes and wavefronts per site
            uint32_t rl = wave_sum(cnt.prof_lane[i]), rw = wave_sum(cnt.prof_wave[i]);
            unsigned long long rc = cnt.prof_cycles[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) rc += __shfl_xor(rc, off);
            if (lane == 0) {
                atomicAdd(&stats[kStatCount + 3 * i], (unsigned long long)rl);
                atomicAdd(&stats[kStatCount + 3 * i + 1], (unsigned long long)rw);
                atomicAdd(&stats[kStatCount + 3 * i + 2], rc);
            }
        }
    }
}
template <bool LDS, bool STATS, int INTEGRATOR, bool SOBOL>
__global__ void __launch_bounds__(kBlock, render_waves(LDS, STATS, INTEGRATOR)) k_render(const KRender kp) { render_workgroup<LDS, STATS, INTEGRATOR, SOBOL>(kp); }
// ... k_render<LDS, false, INTEGRATOR, false> with image textures
template <bool LDS, int INTEGRATOR>
__global__ void __launch_bounds__(kBlock, render_waves(LDS, false, INTEGRATOR)) k_render_tex(const KRender kp) { render_workgroup<LDS, false, INTEGRATOR, false, 0, true>(kp); }
// ... with the environment map as a light (TRC_FLAG_ENV_LIGHT), without and with image textures
template <bool LDS, int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(kBlock, render_waves(LDS, false, INTEGRATOR)) k_render_env(const KRenderEnv kpe) {
    render_workgroup<LDS, false, INTEGRATOR, false, 0, TEX, Light::Env>(kpe.kp, &kpe.el);
}
// ... with the mesh's emissive triangles as lights (TRC_FLAG_MESH_LIGHTS), without and with image textures
template <bool LDS, int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(kBlock, render_waves(LDS, false, INTEGRATOR)) k_render_mesh(const KRenderMesh kpm) {
    render_workgroup<LDS, false, INTEGRATOR, false, 0, TEX, Light::Mesh>(kpm.kp, &kpm.ml);
}

// kernelPathTracing on a tree that is READ FROM MEMORY (mesh scenes), production launches of >= 8 spp: persistent
// workgroups.  With one wavefront per workgroup every wavefront stages its own copy of the top of the tree, and 16-24 copies
// per CU leave room for ~45 nodes (5 levels) each.  Here a workgroup is as many wavefronts as one (tracePath: half a) CU
// holds, they stage ONE prefix -- 30-60 KB, the top 9-10 levels -- and then every wavefront on its own pulls pixel
// blocks from a device-wide queue in the launch order (longest first) until it is empty, so no wavefront slot waits
// for a sibling (what cost the 4-wavefront workgroups of docs/HISTORY.md section 9 their 20 %).  Same blocks, same arithmetic per
// lane.  Measured (profiles/r02/persistent_workgroups.txt): 2.4-3 % on configs 3 / 4 and the traceVolume scene -- most
// of a mesh ray's steps are deep in the tree, below any prefix.  Workgroup shapes (trc_render_config.hpp): tracePath 4 wavefronts x 7
// per CU -- seven waves per SIMD at 72 registers, the one shape of 28 wavefronts that packs (round 5; rounds 2-4 ran 12 x 2 and 16 x 2) --,
// traceMIS 16 x 2 with 8 stack entries per lane in LDS, traceVolume 16 x 1.
// TEX (image textures): k_render_pwg_tex<INTEGRATOR>, the same body (trc_render_pwg_body.inc) with hit_color<true>
template <int INTEGRATOR, bool SOBOL>
__global__ void __launch_bounds__(64 * pwg_waves(INTEGRATOR), pwg_simd_waves(INTEGRATOR)) k_render_pwg(const KRender kp) {
    constexpr bool TEX = false;
    constexpr Light LIGHT = Light::None;
    const void* const tables = nullptr;
#include "trc_render_pwg_body.inc"
}
template <int INTEGRATOR>
__global__ void __launch_bounds__(64 * pwg_waves(INTEGRATOR), pwg_simd_waves(INTEGRATOR)) k_render_pwg_tex(const KRender kp) {
    constexpr bool SOBOL = false, TEX = true;
    constexpr Light LIGHT = Light::None;
    const void* const tables = nullptr;
#include "trc_render_pwg_body.inc"
}
template <int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(64 * pwg_waves(INTEGRATOR), pwg_simd_waves(INTEGRATOR)) k_render_pwg_env(const KRenderEnv kpe) {
    constexpr bool SOBOL = false;
    constexpr Light LIGHT = Light::Env;
    const KRender& kp = kpe.kp;
    const EnvLight* const tables = &kpe.el;
#include "trc_render_pwg_body.inc"
}

template <int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(64 * pwg_waves(INTEGRATOR), pwg_simd_waves(INTEGRATOR)) k_render_pwg_mesh(const KRenderMesh kpm) {
    constexpr bool SOBOL = false;
    constexpr Light LIGHT = Light::Mesh;
    const KRender& kp = kpm.kp;
    const MeshLight* const tables = &kpm.ml;
#include "trc_render_pwg_body.inc"
}

// kernelPathTracing for launches of FEW samples per pixel (the reference's own pattern is one per dispatch): with one 8x8
// block per wavefront a lane that has finished its few samples waits for the longest path of the wavefront -- at 1 spp
// the wavefront runs ~9 iterations for 1.7 rays per lane.  Here a wavefront owns a strip of `kp.strip` consecutive
// blocks of the list and every lane walks its own pixel of block after block, so a lane whose pixel is done starts
// the same pixel of the next block at once (path regeneration across pixels instead of across samples).  The strip
// is the unit of the adaptive launch order.  Pixels are independent: the frame is k_render's, bit for bit.
// TEX (image textures): k_render_strip_tex<LDS, INTEGRATOR>, the same body (trc_render_strip_body.inc) with hit_color<true>
template <bool LDS, int INTEGRATOR, bool SOBOL>
__global__ void __launch_bounds__(kBlock, strip_waves(INTEGRATOR)) k_render_strip(const KRender kp) {
    constexpr bool TEX = false;
    constexpr Light LIGHT = Light::None;
    const void* const tables = nullptr;
#include "trc_render_strip_body.inc"
}
template <bool LDS, int INTEGRATOR>
__global__ void __launch_bounds__(kBlock, strip_waves(INTEGRATOR)) k_render_strip_tex(const KRender kp) {
    constexpr bool SOBOL = false, TEX = true;
    constexpr Light LIGHT = Light::None;
    const void* const tables = nullptr;
#include "trc_render_strip_body.inc"
}
template <bool LDS, int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(kBlock, strip_waves(INTEGRATOR)) k_render_strip_env(const KRenderEnv kpe) {
    constexpr bool SOBOL = false;
    constexpr Light LIGHT = Light::Env;
    const KRender& kp = kpe.kp;
    const EnvLight* const tables = &kpe.el;
#include "trc_render_strip_body.inc"
}

template <bool LDS, int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(kBlock, strip_waves(INTEGRATOR)) k_render_strip_mesh(const KRenderMesh kpm) {
    constexpr bool SOBOL = false;
    constexpr Light LIGHT = Light::Mesh;
    const KRender& kp = kpm.kp;
    const MeshLight* const tables = &kpm.ml;
#include "trc_render_strip_body.inc"
}

// The kernel table of one tree residence and integrator (trc_render_config.hpp: RenderKernels).  Taking a kernel's address is what
// instantiates it, so this is also the list of what each translation unit compiles: Sobol' for tracePath / traceMIS only,
// persistent workgroups on trees read from memory only; no statistics twin of the strip / persistent kernels or of the texture ones.
template <bool LDS, int INTEGRATOR>
inline RenderKernels render_kernels() {
    constexpr bool kSobol = INTEGRATOR != TRC_INTEGRATOR_VOLUME;
    RenderKernels t{};
    t.one[kVariantPlain] = render_kernel(&k_render<LDS, false, INTEGRATOR, false>, render_waves(LDS, false, INTEGRATOR));
    t.one[kVariantStats] = render_kernel(&k_render<LDS, true, INTEGRATOR, false>, render_waves(LDS, true, INTEGRATOR));
    t.one[kVariantTex] = render_kernel(&k_render_tex<LDS, INTEGRATOR>, render_waves(LDS, false, INTEGRATOR));
    t.strip[kVariantPlain] = render_kernel(&k_render_strip<LDS, INTEGRATOR, false>, strip_waves(INTEGRATOR));
    t.strip[kVariantTex] = render_kernel(&k_render_strip_tex<LDS, INTEGRATOR>, strip_waves(INTEGRATOR));
    if constexpr (kSobol) {
        t.one[kVariantSobol] = render_kernel(&k_render<LDS, false, INTEGRATOR, true>, render_waves(LDS, false, INTEGRATOR));
        t.strip[kVariantSobol] = render_kernel(&k_render_strip<LDS, INTEGRATOR, true>, strip_waves(INTEGRATOR));
    }
    if constexpr (!LDS) {
        t.pwg[kVariantPlain] = render_kernel(&k_render_pwg<INTEGRATOR, false>, pwg_simd_waves(INTEGRATOR));
        t.pwg[kVariantTex] = render_kernel(&k_render_pwg_tex<INTEGRATOR>, pwg_simd_waves(INTEGRATOR));
        if constexpr (kSobol) t.pwg[kVariantSobol] = render_kernel(&k_render_pwg<INTEGRATOR, true>, pwg_simd_waves(INTEGRATOR));
    }
    if constexpr (INTEGRATOR == TRC_INTEGRATOR_MIS) {        // TRC_FLAG_ENV_LIGHT: traceMIS only
        t.one[kVariantEnv] = render_kernel(&k_render_env<LDS, INTEGRATOR, false>, render_waves(LDS, false, INTEGRATOR));
        t.one[kVariantEnvTex] = render_kernel(&k_render_env<LDS, INTEGRATOR, true>, render_waves(LDS, false, INTEGRATOR));
        t.strip[kVariantEnv] = render_kernel(&k_render_strip_env<LDS, INTEGRATOR, false>, strip_waves(INTEGRATOR));
        t.strip[kVariantEnvTex] = render_kernel(&k_render_strip_env<LDS, INTEGRATOR, true>, strip_waves(INTEGRATOR));
        if constexpr (!LDS) {
            t.pwg[kVariantEnv] = render_kernel(&k_render_pwg_env<INTEGRATOR, false>, pwg_simd_waves(INTEGRATOR));
            t.pwg[kVariantEnvTex] = render_kernel(&k_render_pwg_env<INTEGRATOR, true>, pwg_simd_waves(INTEGRATOR));
        }
        // TRC_FLAG_MESH_LIGHTS: traceMIS only.  (The two blocks stay written out: the kernels are laid out in the code object in the order they
        // are named here, and a helper that names each once interleaves the Env and Mesh kernels.)
        t.one[kVariantMesh] = render_kernel(&k_render_mesh<LDS, INTEGRATOR, false>, render_waves(LDS, false, INTEGRATOR));
        t.one[kVariantMeshTex] = render_kernel(&k_render_mesh<LDS, INTEGRATOR, true>, render_waves(LDS, false, INTEGRATOR));
        t.strip[kVariantMesh] = render_kernel(&k_render_strip_mesh<LDS, INTEGRATOR, false>, strip_waves(INTEGRATOR));
        t.strip[kVariantMeshTex] = render_kernel(&k_render_strip_mesh<LDS, INTEGRATOR, true>, strip_waves(INTEGRATOR));
        if constexpr (!LDS) {
            t.pwg[kVariantMesh] = render_kernel(&k_render_pwg_mesh<INTEGRATOR, false>, pwg_simd_waves(INTEGRATOR));
            t.pwg[kVariantMeshTex] = render_kernel(&k_render_pwg_mesh<INTEGRATOR, true>, pwg_simd_waves(INTEGRATOR));
        }
    }
    return t;
}
TRC_RENDER_NS_END
