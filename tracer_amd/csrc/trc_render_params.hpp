// trc_render_params.hpp -- the kernels of TRC_FLAG_MATERIAL_PARAMS: DEFINITIONS.  render_block's sample loop (trc_render_kernels.hpp)
// with the integrator's step instantiated over the parametrised lobes (dev_integrator.hpp: PARAMS; dev_bsdf.hpp: material_S_F_params,
// material_F_params), and nothing else about a sample changed: cast_ray, path_begin, the same path_step / mis_step, the running mean
// weighted by frame0 + s, the NaN / Inf clamp and the counters.  Beside the kernels of trc_render_kernels.hpp, not inside them: those are
// tuned to the register, and the table's pointer and a lane's entry are state they have no room for.  So, as for the kernels of
// TRC_FLAG_CAMERA_RAYS (trc_render_rays.hpp): one pixel block per one-wavefront workgroup, no parked state, no memo, no strips, no
// persistent workgroups, no dense kernel, no Sobol', no statistics, no light besides the squares.  A lane fetches its material's entry
// (48 bytes, three 16-byte loads) where the lobe is built, not at the hit: Lambert and emitter vertices never load it, and nothing of it
// is live across the walk.  Included by trc_render_params.hip / trc_render_params_mem.hip, which instantiate the kernels through their
// tables (trc_render_config.hpp: RenderParamsKernels); trc_render_pass.hip launches them.
#pragma once

#include "trc_render_kernels.hpp"

TRC_RENDER_NS_BEGIN

// One pixel block of a flagged launch: the launch entry is decoded as render_block decodes it (the split plan may hand out quarters,
// sixteenths and single pixels), RNG texel and accumulator are read and written once, the block's cost is written per sample.
template <bool LDS, int INTEGRATOR, bool HYB, bool TEX>
__device__ __forceinline__ void render_params_block(const KRenderParams& kr, const DScene& sc, const uint32_t* small_base, uint32_t* stack, uint32_t* lvstack,
                                                    uint32_t* ovf, const uint32_t slot, const uint32_t lane,
                                                    uint32_t& n_rays, uint32_t& n_shaded, uint32_t& n_paths, TravCounters& cnt) {
    const KRender& kp = kr.kp;
    const uint64_t t_start = clock64();          // this wavefront's own duration = the next launch's sort key
    const uint32_t entry = kp.order ? kp.order[slot] : slot;
    const uint32_t index = entry & kLaunchIndexMask, code = entry >> kLaunchCodeShift;
    if (index >= kp.n_tiles) return;                            // padding of the launch list's part region (k_pad_launch)
    const uint32_t tile = kp.tiles[index];                      // pixel block: x | y << 16 in units of the block edge
    // the launch codes of trc_ctx.hpp, as in render_block: 0 the whole block, 1..4 a quarter, 5..20 a sixteenth, 21..84 one pixel
    const uint32_t part = code >= 21u ? (code - 21u) >> 2 : (code >= 5u ? code - 5u : 0u);
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

    if (active && kp.spp > 0) {
        PathCtxParams<TEX> cx;
        fill_path_ctx<false, TEX, Light::None>(cx, kp, sc, small_base, stack, lvstack, nullptr);
        cx.S.ovf = ovf;
        cx.mparams = kr.table;

        const size_t pix = (size_t)py * W + px;
        uint4 texel = reinterpret_cast<const uint4*>(kp.fr.rng)[pix];       // r, g, b, a
        const float4 acc = reinterpret_cast<const float4*>(kp.fr.accum)[pix];
        F3 cached = f3(acc.x, acc.y, acc.z);
        const float u = (float)px / (float)W;                               // no sub-pixel jitter (B-2)
        const float v = (float)(py % kp.view_height) / (float)kp.view_height;      // one view: view_height == H (a stacked view is refused)
        uint32_t s = 0;

        PathState ps;
        Pcg rng;
        // pcg32_t rng = { rng_inc, rng_state } aggregate-initialises {state, inc}: the two 64-bit words trade roles every frame
        // (Render.metal:516-519,545-557, B-1)
        rng.state = ((uint64_t)texel.z << 32) | texel.w;
        rng.inc = ((uint64_t)texel.x << 32) | texel.y;
        path_begin(ps, cast_ray(kp.cam, u, v, rng), kp.max_depth);
        bool alive = true;
        // flat loop: one Scene::hit per iteration; a finished path immediately regenerates the next sample
        while (alive) {
            constexpr int kDefer = LDS ? TRC_DEFER_LDS : TRC_DEFER_GLOBAL;      // dev_intersect.hpp: trav_test_leaf
            bump(n_rays);
            const bool hitted = scene_hit<LDS, false, false, false, false, HYB, kDefer>(cx.S, cx.root_min, cx.root_max, ps.ray, ps.rec, FLT_MAX,
                                                                                       cx.stack, cx.lvstack, cnt);
            F3 color;
            const bool finished = (INTEGRATOR == TRC_INTEGRATOR_PATH)
                                      ? path_step<false, false, TEX, uint32_t, true>(cx, ps, hitted, rng, cnt, n_shaded, color)
                                      : mis_step<LDS, false, false, false, HYB, TEX, Light::None, uint32_t, true>(cx, ps, hitted, rng, cnt, n_rays, n_shaded, color);
            if (finished) {      // accumulate, hand the RNG words back to the texel, start the next sample (or stop)
                const bool bad = is_inf(color.x) || is_nan(color.x) || is_inf(color.y) || is_nan(color.y) ||
                                 is_inf(color.z) || is_nan(color.z);
                if (bad) color = f3(0);                                         // :537-538
                const uint32_t frame = kp.frame0 + s;
                cached = div_shared(cached * (float)frame + color, (float)(frame + 1));      // running mean, :540-541
                texel.y = (uint32_t)rng.state; texel.x = (uint32_t)(rng.state >> 32);
                texel.w = (uint32_t)rng.inc;   texel.z = (uint32_t)(rng.inc >> 32);
                n_paths++;
                if (++s == kp.spp) alive = false;
                else {
                    rng.state = ((uint64_t)texel.z << 32) | texel.w;
                    rng.inc = ((uint64_t)texel.x << 32) | texel.y;
                    path_begin(ps, cast_ray(kp.cam, u, v, rng), kp.max_depth);
                }
            }
        }
        float4 out; out.x = cached.x; out.y = cached.y; out.z = cached.z; out.w = 1.0f;
        reinterpret_cast<float4*>(kp.fr.accum)[pix] = out;
        reinterpret_cast<uint4*>(kp.fr.rng)[pix] = texel;
    }

    // per SAMPLE (cost_div = 4 x spp), so that launches of different lengths speak of the same quantity
    if (lane == 0) kp.block_cost[canon] = (uint32_t)min((unsigned long long)(clock64() - t_start) / kp.cost_div, 0xFFFFFFull);
}

// the kernel: one one-wavefront workgroup = one entry of the launch list, at the launch bounds of the k_render entry it shadows
template <bool LDS, int INTEGRATOR, bool TEX>
__global__ void __launch_bounds__(kBlock, render_waves(LDS, false, INTEGRATOR)) k_render_params(const KRenderParams kr) {
    const KRender& kp = kr.kp;
    if (kp.n_launch && blockIdx.x >= *kp.n_launch) return;      // the grid is sized for the most quarters a plan may splice in
    const DScene& sc = kp.ks.sc;
    const uint32_t* small_base = stage_scene(sc);
    uint32_t* stack = lane_stack(sc);
    uint32_t* lvstack = lane_lvstack(sc);

    const uint32_t lane = threadIdx.x;
    uint32_t n_rays = 0, n_shaded = 0, n_paths = 0;
    TravCounters cnt;
    counters_zero(cnt);
    constexpr bool kHybridStack = !LDS && hybrid_stack(INTEGRATOR);     // plan_launch_lds
    uint32_t* ovf = kHybridStack ? kp.stack_ovf + (size_t)blockIdx.x * sc.stack_ovf_rows * kBlock + lane : nullptr;
    render_params_block<LDS, INTEGRATOR, kHybridStack, TEX>(kr, sc, small_base, stack, lvstack, ovf, blockIdx.x, lane, n_rays, n_shaded, n_paths, cnt);

    // exact work counters: wave reduction, one 64-bit atomic per wave and counter
    uint32_t r_paths = wave_sum(n_paths), r_rays = wave_sum(n_rays), r_shaded = wave_sum(n_shaded);
    unsigned long long* const stats = stat_row(kp.stats, blockIdx.x);
    if (lane == 0) {
        atomicAdd(&stats[kStatPaths], (unsigned long long)r_paths);
        atomicAdd(&stats[kStatRays], (unsigned long long)r_rays);
        atomicAdd(&stats[kStatShaded], (unsigned long long)r_shaded);
    }
}

// the table of one tree residence (trc_render_config.hpp: RenderParamsKernels); taking a kernel's address is what instantiates it
template <bool LDS>
inline RenderParamsKernels render_params_kernels() {
    RenderParamsKernels t{};
    t.one[0][0] = render_kernel(&k_render_params<LDS, TRC_INTEGRATOR_PATH, false>, render_waves(LDS, false, TRC_INTEGRATOR_PATH));
    t.one[0][1] = render_kernel(&k_render_params<LDS, TRC_INTEGRATOR_PATH, true>, render_waves(LDS, false, TRC_INTEGRATOR_PATH));
    t.one[1][0] = render_kernel(&k_render_params<LDS, TRC_INTEGRATOR_MIS, false>, render_waves(LDS, false, TRC_INTEGRATOR_MIS));
    t.one[1][1] = render_kernel(&k_render_params<LDS, TRC_INTEGRATOR_MIS, true>, render_waves(LDS, false, TRC_INTEGRATOR_MIS));
    return t;
}
TRC_RENDER_NS_END
