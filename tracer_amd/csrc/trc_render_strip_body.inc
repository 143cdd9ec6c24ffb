// trc_render_strip_body.inc -- the body of k_render_strip / _tex / _env / _mesh, included as the body of each kernel (trc_render_kernels.hpp)
// rather than called from a helper: every kernel keeps its code and its name, and the twins share the source.  (Tried in round 12 as a
// __forceinline__ template taking const KRender&: it changed the code of every k_render_strip* kernel of the translation unit.  It stays a file.)
// Expects in scope: kp, LDS, INTEGRATOR, SOBOL, TEX, LIGHT and tables (that light's sampling tables, null for Light::None).
    const DScene& sc = kp.ks.sc;
    const uint32_t* small_base = stage_scene(sc);
    uint32_t* stack = lane_stack(sc);
    const uint64_t t_start = clock64();
    const uint32_t canon = kp.order ? kp.order[blockIdx.x] : blockIdx.x;     // strip index
    const uint32_t lane = threadIdx.x;
    const uint32_t W = kp.fr.width, H = kp.fr.height;
    // the strip's pixels form one pool: pixel p = lane (p mod block size) of block (p / block size); a lane whose pixel is
    // done takes the next unclaimed one, so no lane waits for "its" pixel of the next block while others still trace
    const uint32_t blk0 = canon * kp.strip;
    const uint32_t bshift = 2u * kp.blk_shift;                               // log2(pixels per block): 6 or 4
    const uint32_t pool_end = (min(blk0 + kp.strip, kp.n_tiles) - blk0) << bshift;
    uint32_t pool_next = 0;                                                  // wave-uniform: next unclaimed pool index

    uint32_t n_rays = 0, n_shaded = 0, n_paths = 0;
    TravCounters cnt;
    counters_zero(cnt);

    PathCtxOf<TEX, LIGHT> cx;
    constexpr bool kHybridStack = !LDS && hybrid_stack(INTEGRATOR);
    uint32_t* const ovf = kHybridStack ? kp.stack_ovf + (size_t)blockIdx.x * sc.stack_ovf_rows * kBlock + lane : nullptr;
    fill_path_ctx<SOBOL, TEX, LIGHT>(cx, kp, sc, small_base, stack, stack, tables);      // (one stack: lvstack = stack; sobol_xy: deal_pixels)
    cx.S.ovf = ovf;

    PathState ps;
    Pcg rng;
    uint4 texel;
    F3 cached = f3(0);
    float u = 0, v = 0;
    uint32_t s = 0, pix = 0;
    uint64_t state_after_cast = 0;
    bool alive = false, want = true;                  // want: this lane needs a (new) pixel

    auto begin_sample = [&]() {                       // castRay, then (SOBOL) the sampler of this frame: Render.metal:527-530
        rng.state = ((uint64_t)texel.z << 32) | texel.w;      // the two words trade roles every frame (B-1)
        rng.inc = ((uint64_t)texel.x << 32) | texel.y;
        path_begin(ps, cast_ray(kp.cam, u, v, rng), kp.max_depth);
        if (SOBOL) {
            state_after_cast = rng.state;
            ps.sobol_index = sobol_interval_to_index(cx, (uint64_t)(kp.frame0 + s));
            ps.sobol_dim = 0;
        }
    };
    // hands pool indices to the lanes that want one (called where the whole wavefront is converged); a lane whose index
    // falls outside the frame (ragged edge blocks) simply asks again in the next round
    auto deal_pixels = [&]() {
        const unsigned long long m = __ballot(want);
        if (m == 0ull) return;
        const uint32_t mine = pool_next + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        pool_next += (uint32_t)__popcll(m);
        if (!want) return;
        if (mine >= pool_end) { want = false; return; }                        // the pool is empty: this lane is done
        const uint32_t tile = kp.tiles[blk0 + (mine >> bshift)];
        const uint32_t l = mine & ((1u << bshift) - 1u), bs = kp.blk_shift;
        const uint32_t px = ((tile & 0xFFFFu) << bs) + (l & ((1u << bs) - 1u));
        const uint32_t py = ((tile >> 16) << bs) + (l >> bs);
        if (px >= W || py >= H) return;                                        // not a pixel: ask again
        pix = py * W + px;
        texel = reinterpret_cast<const uint4*>(kp.fr.rng)[pix];
        const float4 acc = reinterpret_cast<const float4*>(kp.fr.accum)[pix];
        cached = f3(acc.x, acc.y, acc.z);
        u = (float)px / (float)W;                                              // no sub-pixel jitter (B-2)
        v = (float)(py % kp.view_height) / (float)kp.view_height;
        if (SOBOL) { cx.sobol_xy[0] = px; cx.sobol_xy[1] = py % kp.view_height; }
        s = 0;
        want = false;
        alive = true;
        begin_sample();
    };
    auto finish_sample = [&](F3 color) {
        const bool bad = is_inf(color.x) || is_nan(color.x) || is_inf(color.y) || is_nan(color.y) ||
                         is_inf(color.z) || is_nan(color.z);
        if (bad) color = f3(0);                                         // :537-538
        const uint32_t frame = kp.frame0 + s;
        cached = (cached * (float)frame + color) / (float)(frame + 1);  // running mean, :540-541
        if (SOBOL) rng.state = state_after_cast;
        texel.y = (uint32_t)rng.state; texel.x = (uint32_t)(rng.state >> 32);
        texel.w = (uint32_t)rng.inc;   texel.z = (uint32_t)(rng.inc >> 32);
        n_paths++;
        if (++s == kp.spp) {                                            // pixel done: write it back, take the next block's
            float4 out; out.x = cached.x; out.y = cached.y; out.z = cached.z; out.w = 1.0f;
            reinterpret_cast<float4*>(kp.fr.accum)[pix] = out;
            reinterpret_cast<uint4*>(kp.fr.rng)[pix] = texel;
            alive = false;
            want = true;
        } else {
            begin_sample();
        }
    };

    for (;;) {                                        // wave-uniform loop: every lane stays in it until nobody has or wants work
        deal_pixels();
        if (__ballot(alive || want) == 0ull) break;
        if (alive) {
            constexpr bool kVolume = INTEGRATOR == TRC_INTEGRATOR_VOLUME;
            constexpr int kDefer = LDS ? TRC_DEFER_LDS : TRC_DEFER_GLOBAL;
            bool hitted = true;
            if (!(kVolume && TRC_TRACK_SLICE > 0 && ps.tracking)) {       // render_block's loop above
                n_rays++;
                hitted = scene_hit<LDS, false, false, false, kVolume, kHybridStack, kDefer>(cx.S, cx.root_min, cx.root_max, ps.ray, ps.rec, FLT_MAX,
                                                                          cx.stack, cx.lvstack, cnt);
            }
            F3 color;
            const bool finished = (INTEGRATOR == TRC_INTEGRATOR_PATH)
                                      ? path_step<false, SOBOL, TEX>(cx, ps, hitted, rng, cnt, n_shaded, color)
                                      : mis_step<LDS, false, kVolume, SOBOL, kHybridStack, TEX, LIGHT>(cx, ps, hitted, rng, cnt, n_rays, n_shaded, color);
            if (finished) finish_sample(color);
        }
    }
    uint32_t r_paths = wave_sum(n_paths), r_rays = wave_sum(n_rays), r_shaded = wave_sum(n_shaded);
    if (lane == 0) {
        kp.block_cost[canon] = (uint32_t)min((unsigned long long)(clock64() - t_start) / kp.cost_div, 0xFFFFFFull);
        unsigned long long* const stats = stat_row(kp.stats, blockIdx.x);
        atomicAdd(&stats[kStatPaths], (unsigned long long)r_paths);
        atomicAdd(&stats[kStatRays], (unsigned long long)r_rays);
        atomicAdd(&stats[kStatShaded], (unsigned long long)r_shaded);
    }
