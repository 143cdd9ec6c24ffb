// trc_render_pass.hip -- trc_render: one pass of kernelPathTracing (RT_Metal/Metal/Render.metal:495-558) over the caller's share of
// the frame, step by step (render_pass), the kept launches of few samples (trc_flush), the LDS plans and the launch itself.
// The kernels: trc_render_kernels.hpp; the block schedule: trc_schedule.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "trc_launch.hpp"

static size_t dyn_lds_bytes(const DScene& sc, bool stats) {
    size_t dwords = sc.lds_dwords + (size_t)sc.stack_lds * kBlock * (stats ? 2u : 1u);
    return dwords * 4;
}
size_t trc_dyn_lds_bytes(const trc_ctx* ctx, bool stats) { return dyn_lds_bytes(ctx->ks.sc, stats); }

// LDS plan of ONE production render launch on a tree that is read from memory.  A CU holds 4 x W one-wavefront
// workgroups (W = the waves per SIMD the kernel's registers allow) only if each fits 160 KB / (4 W) of LDS: the lane
// stacks plus the staged scene prefix.  plan_lds (upload time) assumes W = 4 and a stack as deep as the tree; here
//  * the stack keeps kStackLdsLevels entries per lane in LDS, deeper entries go to per-workgroup rows in global memory
//    (dev_intersect.hpp::stack_put) -- a ray rarely has more siblings pending, the tree depth is the worst case;
//  * the node prefix takes what is left of the workgroup's share (host trees: any prefix of the BFS order may be staged).
// Measured on the 1 M-triangle scene (depth 27: 6.9 KB of stack): the tracePath kernel (5 waves/SIMD by registers) was
// held at 4 by LDS; 34.9 -> 32.8 ms per 32-spp launch once it fits.
constexpr uint32_t kStackLdsLevels = 16;
// LDS entries of a two-level stack when `levels` are wanted, and the global rows behind them
static void set_hybrid_stack(DScene& sc, uint32_t levels) {
    sc.stack_lds = std::min(sc.stack_depth, std::max(1u, levels));
    sc.stack_ovf_rows = sc.stack_depth - sc.stack_lds;
}
// More than 64 KB of dynamic LDS (the persistent workgroups) has to be asked for once per kernel AND per device (the attribute is set
// on the current device's copy of the function): remembered in the context, which is bound to one device.
static hipError_t grant_lds(trc_ctx* ctx, const void* fn, size_t lds) {
    if (lds <= 64 * 1024 || std::find(ctx->lds_granted.begin(), ctx->lds_granted.end(), fn) != ctx->lds_granted.end()) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024));
    if (e == hipSuccess) ctx->lds_granted.push_back(fn);
    return e;
}

// Workgroups of `block` threads and `lds` bytes of dynamic LDS of kernel `fn` that one CU holds at once: the runtime's answer, which
// knows the kernel's registers and the unit LDS is granted in on this device (a hand formula knew neither: it assumed 512 bytes, and
// the launch plans counted wavefront slots the CU never filled).  Asked once per (kernel, block, lds) and context.
static trc_status resident_workgroups(trc_ctx* ctx, const void* fn, uint32_t block, size_t lds, uint32_t* per_cu) {
    for (const trc_ctx::Residency& e : ctx->residency)
        if (e.fn == fn && e.block == block && e.lds == lds) { *per_cu = e.per_cu; return TRC_OK; }
    HIP_TRY(ctx, grant_lds(ctx, fn, lds));
    if (ctx->residency.size() >= 64u) ctx->residency.clear();      // (a context that has seen many scenes: start over, the answers come back)
    int n = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, (int)block, lds));
    *per_cu = (uint32_t)std::max(n, 0);
    ctx->residency.push_back({fn, block, lds, *per_cu});
    return TRC_OK;
}
// ... and of the same kernel with no dynamic LDS at all: what its registers allow, the most any LDS plan can reach
static trc_status resident_by_registers(trc_ctx* ctx, const void* fn, uint32_t block, uint32_t* per_cu) { return resident_workgroups(ctx, fn, block, 0, per_cu); }

// LDS is planned in steps of 512 bytes; where the runtime then admits fewer workgroups than the plan is for, the plan is made again
// for a share one step smaller, until they fit
constexpr uint32_t kLdsStepDwords = 128;

static trc_status plan_launch_lds(trc_ctx* ctx, DScene& sc, const RenderKernel& kern, bool hybrid) {
    const uint32_t levels = ctx->knobs.stack_lds_levels > 0 ? (uint32_t)ctx->knobs.stack_lds_levels : kStackLdsLevels;
    if (hybrid) set_hybrid_stack(sc, ctx->knobs.no_lds_fit ? std::max(levels, sc.stack_depth) : levels);      // (knob: the whole stack in LDS)
    if (ctx->knobs.no_lds_fit) return TRC_OK;                                          // A/B knobs (trc_debug_set)
    if (!ctx->lds_prefix_ok) return TRC_OK;                                            // all or nothing was decided at upload
    const uint32_t planned = 4u * (uint32_t)kern.waves;                                // workgroups per CU the kernel is compiled for
    uint32_t want = 0;
    TRC_TRY(resident_by_registers(ctx, kern.fn, kBlock, &want));
    want = std::min(want, planned);
    const uint32_t share = ((160u * 1024u / 4u) / planned) & ~(kLdsStepDwords - 1u);   // dwords
    const uint32_t least = sc.off_nodes + kNodeDwords;
    // the node prefix for a share of `per_wg` dwords beside the stack rows
    auto plan_prefix = [&](uint32_t per_wg) {
        const uint32_t stack = sc.stack_lds * kBlock;
        uint32_t room = std::max(per_wg > stack ? per_wg - stack : 0u, least);
        room = std::min(room, kLdsSceneBytes / 4);
        sc.n_lds_nodes = std::min(sc.n_nodes, (room - sc.off_nodes) / kNodeDwords);
        sc.lds_dwords = sc.off_nodes + sc.n_lds_nodes * kNodeDwords;
        return room > least;                                                           // there is prefix left to give back
    };
    plan_prefix(share);
    const DScene first = sc;
    // checked against the runtime: give back node prefix, 512 bytes at a time; then (a stack of two levels, no knob) one stack entry
    // in LDS and the prefix again -- down to the six entries the persistent workgroups stop at too
    for (uint32_t lv = sc.stack_lds;; --lv) {
        if (lv != first.stack_lds) set_hybrid_stack(sc, lv);
        for (uint32_t per_wg = share;; per_wg -= kLdsStepDwords) {
            const bool more = plan_prefix(per_wg);
            uint32_t fit = 0;
            TRC_TRY(resident_workgroups(ctx, kern.fn, kBlock, dyn_lds_bytes(sc, false), &fit));
            if (fit >= want) return TRC_OK;
            if (!more || per_wg < kLdsStepDwords) break;
        }
        if (!hybrid || lv <= 6u || ctx->knobs.stack_lds_levels > 0) break;
    }
    sc = first;                              // nothing the plan can give back lets `want` in: the first plan, as it always ran
    return TRC_OK;
}

// LDS plan of a persistent-workgroup launch (k_render_pwg): `waves` wavefronts share one staged prefix; the workgroup's
// share of the CU's 160 KB minus the wavefronts' stacks is all node prefix.  False when even one node does not fit.
static bool plan_pwg_share(const trc_ctx* ctx, DScene& sc, uint32_t waves, uint32_t per_wg, bool hybrid, uint32_t default_levels, uint32_t park_rows) {
    uint32_t levels = ctx->knobs.stack_lds_levels > 0 ? (uint32_t)ctx->knobs.stack_lds_levels : default_levels;      // trc_render_config.hpp
    for (;; --levels) {
        DScene t = sc;
        if (hybrid) set_hybrid_stack(t, levels);
        const uint32_t stacks = waves * (t.stack_lds + park_rows) * kBlock;       // per wavefront: its stack rows, then its park rows (k_render_pwg)
        if (per_wg >= stacks + t.off_nodes + kNodeDwords) {
            t.n_lds_nodes = std::min(t.n_nodes, (per_wg - stacks - t.off_nodes) / kNodeDwords);
            t.lds_dwords = t.off_nodes + t.n_lds_nodes * kNodeDwords;
            sc = t;
            return true;
        }
        // a scene with many analytic primitives / materials: fewer stack entries in LDS before giving the persistent workgroups up
        if (!hybrid || levels <= 6u || ctx->knobs.stack_lds_levels > 0) return false;
    }
}
static size_t pwg_lds_bytes(const DScene& sc, uint32_t waves, uint32_t park_rows) {
    return ((size_t)sc.lds_dwords + (size_t)waves * (sc.stack_lds + park_rows) * kBlock) * 4;
}
// ... for `per_cu` workgroups per CU.  (Not checked against the runtime as plan_launch_lds is: with that check the full bench ran
// traceVolume 1.4 % slower, outside its spread: profiles/r17/other_configs.txt.)
static bool plan_pwg_lds(const trc_ctx* ctx, DScene& sc, uint32_t waves, uint32_t per_cu, bool hybrid, uint32_t default_levels, uint32_t park_rows) {
    return plan_pwg_share(ctx, sc, waves, ((160u * 1024u / 4u) / per_cu) & ~(kLdsStepDwords - 1u), hybrid, default_levels, park_rows);
}

namespace {

// tables of pbrt::SobolSampler for a 2^m x 2^m pixel grid (include/trc_sobol.h), uploaded once per m
trc_status ensure_sobol_tables(trc_ctx* ctx, uint32_t m) {
    if (!ctx->d_sobol_vdc) {
        std::vector<uint32_t> m32(TRC_SOBOL_DIMS * TRC_SOBOL_MATRIX_SIZE);
        trc_sobol_matrices32(m32.data());
        if (!ctx->d_sobol32) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_sobol32, m32.size() * sizeof(uint32_t)));
        TRC_TRY(trc_copy_to_device(ctx, ctx->d_sobol32, m32.data(), m32.size() * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_sobol_vdc, 2 * TRC_SOBOL_MATRIX_SIZE * sizeof(uint64_t)));
        ctx->sobol_m = ~0u;
    }
    if (ctx->sobol_m != m) {
        uint64_t tb[2 * TRC_SOBOL_MATRIX_SIZE] = {};
        if (m != 0 && trc_sobol_interval_tables(m, tb, tb + TRC_SOBOL_MATRIX_SIZE) != 0)
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "Sobol interval tables");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));            // a launch in flight may still read the old tables
        TRC_TRY(trc_copy_to_device(ctx, ctx->d_sobol_vdc, tb, sizeof(tb), ctx->stream));
        ctx->sobol_m = m;
    }
    return TRC_OK;
}

// The render kernels a scene's launches pick from (trc_render_config.hpp: one table per tree residence and integrator)
// (tri_materials: their twins that read each triangle's material, trc_render_*_tm.hip)
const RenderKernels& render_family(bool lds_scene, uint32_t integrator, bool tri_materials) {
    static const RenderKernels* const lds[3] = {&render_lds_path, &render_lds_mis, &render_lds_volume};
    static const RenderKernels* const mem[3] = {&render_mem_path, &render_mem_mis, &render_mem_volume};
    static const RenderKernels* const lds_tm[3] = {&trimat::render_lds_path, &trimat::render_lds_mis, &trimat::render_lds_volume};
    static const RenderKernels* const mem_tm[3] = {&trimat::render_mem_path, &trimat::render_mem_mis, &trimat::render_mem_volume};
    return *(tri_materials ? (lds_scene ? lds_tm : mem_tm) : (lds_scene ? lds : mem))[integrator];
}

// One render launch (more than 64 KB of dynamic LDS: grant_lds).
hipError_t launch_render(trc_ctx* ctx, const RenderLaunch& r) {
    const void* const fn = r.kern.fn;
    if (const hipError_t e = grant_lds(ctx, fn, r.lds); e != hipSuccess) return e;
    // the parameter block the kernel's RenderArgs asks for: the launch's parameters alone, or with its light's tables behind them
    KRenderEnv kpe;
    KRenderMesh kpm;
    KRenderRays kpr;
    KRenderRaysEnv kpre;
    KRenderParams kpp;
    void* params = const_cast<KRender*>(&r.kp);
    if (r.kern.args == kArgsEnv) { kpe.kp = r.kp; kpe.el = r.el; params = &kpe; }
    if (r.kern.args == kArgsMesh) { kpm.kp = r.kp; kpm.ml = r.ml; params = &kpm; }
    if (r.kern.args == kArgsRays) { kpr.kp = r.kp; kpr.rays = ctx->d_cam_rays; kpr.n_sets = ctx->n_ray_sets; params = &kpr; }
    if (r.kern.args == kArgsRaysEnv) { kpre.kp = r.kp; kpre.el = r.el; kpre.rays = ctx->d_cam_rays; kpre.n_sets = ctx->n_ray_sets; params = &kpre; }
    if (r.kern.args == kArgsParams) { kpp.kp = r.kp; kpp.table = reinterpret_cast<const float4*>(ctx->d_mparams); params = &kpp; }
    void* args[] = {params};
    const hipError_t e = hipLaunchKernel(fn, dim3(r.grid), dim3(r.block), args, r.lds, ctx->stream);
    const hipError_t last = hipGetLastError();          // (and clears what a failed launch left)
    return e != hipSuccess ? e : last;
}

}  // namespace

// One pass of kernelPathTracing over the caller's share of the frame.  `inner`: this pass is one half of a first launch that
// trc_render split in two (below).
static trc_status render_pass(trc_ctx* ctx, const trc_params* p, bool inner);

// First launch of a block list (nothing is known about its blocks: new context, frame size, share, scene, camera or
// integrator): the launch order and the split plan come from the durations of the previous launch, and without them a launch
// runs row-major with every block whole -- config 2 +15 %, the mesh scenes +55-65 % (their heavy blocks start last and the
// launch ends on them; profiles/r04/cold_start.txt).  A pixel's samples are a chain through its RNG texel, so `spp` samples
// in one launch == h samples followed by spp - h (tested: test_spp_fusion_equals_per_frame_launches): the first launch is run
// as a HEAD of kColdHeadSpp samples, cold, and the REST ordered and planned by the head's per-block durations (costs are kept
// per sample, KRender::cost_div, so launches of different lengths speak of the same quantity).  No probe work is thrown
// away, no pixel changes; the only price is the head's own short tail.  Knob no_cold_probe switches it off.
constexpr uint32_t kColdHeadSpp = 8;           // >= 8: the head must run the same kernel and block list as the rest (k_render_strip below)
// `sobol_m` (TRC_FLAG_SOBOL): where the view's log2Resolution goes
static trc_status render_check(trc_ctx* ctx, const trc_params* p, uint32_t* sobol_m = nullptr) {
    if (!ctx || !p) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_render before trc_upload_scene");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_render before trc_resize");
    if (!ctx->has_camera) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render before trc_set_camera");
    const uint32_t nranks = p->tile_nranks ? p->tile_nranks : 1;
    if (p->tile_rank >= nranks) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "tile_rank >= tile_nranks");
    if (p->integrator > TRC_INTEGRATOR_VOLUME) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "unknown integrator");
    if (p->flags & TRC_FLAG_CAMERA_RAYS) {
        if (!ctx->d_cam_rays) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_CAMERA_RAYS: no camera rays in force (trc_upload_camera_rays / trc_generate_camera_rays)");
        if (p->integrator == TRC_INTEGRATOR_VOLUME) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_CAMERA_RAYS: tracePath / traceMIS only");
        // (TRC_FLAG_ENV_LIGHT is let through: its own refusals follow below -- traceMIS, a map -- and k_render_rays_env runs the pair)
        if (p->flags & (TRC_FLAG_SOBOL | TRC_FLAG_COLLECT_STATS | TRC_FLAG_MESH_LIGHTS))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_CAMERA_RAYS: no TRC_FLAG_SOBOL / TRC_FLAG_COLLECT_STATS / TRC_FLAG_MESH_LIGHTS kernels");
        if (p->view_height != 0 && p->view_height < ctx->height) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_CAMERA_RAYS: the ray sets are the frame's, not a stacked view's");
    }
    if (p->flags & TRC_FLAG_MATERIAL_PARAMS) {
        if (!ctx->d_mparams) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MATERIAL_PARAMS: no table in force (trc_upload_material_params)");
        if (p->integrator == TRC_INTEGRATOR_VOLUME) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MATERIAL_PARAMS: tracePath / traceMIS only");
        if (p->flags & (TRC_FLAG_SOBOL | TRC_FLAG_COLLECT_STATS | TRC_FLAG_ENV_LIGHT | TRC_FLAG_MESH_LIGHTS | TRC_FLAG_CAMERA_RAYS))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MATERIAL_PARAMS: no TRC_FLAG_SOBOL / TRC_FLAG_COLLECT_STATS / TRC_FLAG_ENV_LIGHT / TRC_FLAG_MESH_LIGHTS / TRC_FLAG_CAMERA_RAYS kernels");
        if (p->view_height != 0 && p->view_height < ctx->height) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MATERIAL_PARAMS: no stacked views");
    }
    const bool env_light = (p->flags & TRC_FLAG_ENV_LIGHT) != 0;
    if (env_light) {
        if (p->integrator != TRC_INTEGRATOR_MIS) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_ENV_LIGHT: traceMIS only");
        if (p->flags & (TRC_FLAG_SOBOL | TRC_FLAG_COLLECT_STATS))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_ENV_LIGHT: no TRC_FLAG_SOBOL / TRC_FLAG_COLLECT_STATS kernels");
        if (!ctx->d_envmap) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_ENV_LIGHT: no environment map (trc_set_environment_map)");
    }
    const bool mesh_lights = (p->flags & TRC_FLAG_MESH_LIGHTS) != 0;
    if (mesh_lights) {
        if (p->integrator != TRC_INTEGRATOR_MIS) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MESH_LIGHTS: traceMIS only");
        if (p->flags & (TRC_FLAG_SOBOL | TRC_FLAG_COLLECT_STATS | TRC_FLAG_ENV_LIGHT))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_MESH_LIGHTS: no TRC_FLAG_SOBOL / TRC_FLAG_COLLECT_STATS / TRC_FLAG_ENV_LIGHT kernels");
    }
    if (p->integrator != TRC_INTEGRATOR_PATH && ctx->ks.sc.n_squares < 7 && !env_light && !mesh_lights)
        return trc_fail(ctx, TRC_ERR_INVALID_ARG, "traceMIS / traceVolume sample squareList[5] and [6] (Render.metal:320-324,172-176)");
    if (ctx->tex_active() && (p->flags & (TRC_FLAG_SOBOL | TRC_FLAG_COLLECT_STATS)))
        return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "image textures: no TRC_FLAG_SOBOL / TRC_FLAG_COLLECT_STATS kernels (trc_upload_textures)");
    if (p->flags & TRC_FLAG_SOBOL) {
        if (p->integrator == TRC_INTEGRATOR_VOLUME || (p->flags & TRC_FLAG_COLLECT_STATS))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_SOBOL: tracePath / traceMIS, production kernels only");
        if (2ull * p->max_depth > TRC_SOBOL_DIMS)
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_SOBOL: 2 * max_depth exceeds the 40 generated dimensions");
        // resolution = RoundUpPow2(max(wh.x, wh.y)) of the view, log2Resolution = Log2Int(resolution) (SobolSampler.hh:56-58)
        uint32_t m = 0;
        const uint32_t vh = (p->view_height != 0 && p->view_height < ctx->height) ? p->view_height : ctx->height;
        while ((1u << m) < std::max(ctx->width, vh)) ++m;
        if (m > TRC_SOBOL_MAX_LOG2RES) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_SOBOL: frame too large");
        if (sobol_m) *sobol_m = m;
    }
    if (env_light) return trc_env_light_build(ctx);      // the map's sampling tables, once per map (TRC_ERR_OOM: this render does not run)
    if (mesh_lights) return trc_mesh_light_build(ctx);   // the emissive triangles' tables, once per scene and triangle-material array (likewise)
    return TRC_OK;
}

// Launches of few samples, coalesced.  The reference dispatches ONE sample per frame (AAPLRenderer.mm:1195); such a launch
// has no second sample to regenerate finished lanes from and ends on its longest paths: 0.54 ms per sample against 0.31 in
// a fused launch.  A pixel's samples are one chain, so k calls of 1 sample == one call of k samples bit for bit (tested): a
// trc_render of fewer than kCoalesceBelow samples is therefore not launched at once but kept, and extended by the next call
// when that continues it (same parameters, frame0 following on); it is launched when kCoalesceUpTo samples have come
// together, when a call arrives that does not continue it, or when ANY other entry point of the library is entered
// (trc_flush at the top of each: downloads, tonemap, stats, seed, camera ...), so nothing observable changes.  A host that
// displays every frame (one trc_render, one trc_tonemap) gets exactly the launches it asked for; one that renders a run of
// samples before it looks gets them at the fused rate: 64 x 1 spp 34.8 -> 2x.x ms.  Knob no_coalesce switches it off.
constexpr uint32_t kCoalesceBelow = 8, kCoalesceUpTo = 16;
trc_status trc_flush(trc_ctx* ctx) {
    if (!ctx) return TRC_OK;
    TRC_TRY(trc_refit_settle(ctx));      // trc_update_vertices returns before its root box has arrived
    if (!ctx->has_deferred) return TRC_OK;
    ctx->has_deferred = false;
    const trc_params q = ctx->deferred;
    const uint64_t calls = ctx->deferred_calls;
    const trc_status st = render_pass(ctx, &q, false);
    if (st == TRC_OK && calls > 1) ctx->launches += calls - 1;        // trc_stats.launches counts trc_render calls
    if (st != TRC_OK) {
        // the calls that were kept have already returned TRC_OK: the error of their launch surfaces in whatever entry point
        // flushes it, so it says WHICH samples did not run (trc_last_error) -- a host can re-issue exactly those
        ctx->error = "kept launch of " + std::to_string(calls) + " trc_render call(s), frames " + std::to_string(q.frame0) + " .. " +
                     std::to_string(q.frame0 + q.spp - 1) + " (" + std::to_string(q.spp) + " samples per pixel), did not run: " + ctx->error;
    }
    return st;
}
trc_status trc_render_now(trc_ctx* ctx, const trc_params* p) { return render_pass(ctx, p, false); }
extern "C" {
trc_status trc_render(trc_ctx* ctx, const trc_params* p) {
    TRC_TRY(render_check(ctx, p));
    const bool candidate = p->spp > 0 && p->spp < kCoalesceBelow && !(p->flags & TRC_FLAG_COLLECT_STATS) && !ctx->knobs.no_coalesce;
    if (ctx->has_deferred) {
        trc_params& d = ctx->deferred;
        const bool continues = candidate && p->frame0 == d.frame0 + d.spp && p->max_depth == d.max_depth && p->integrator == d.integrator &&
                               p->tile_rank == d.tile_rank && p->tile_nranks == d.tile_nranks && p->flags == d.flags && p->view_height == d.view_height;
        if (continues) {
            d.spp += p->spp;
            ctx->deferred_calls++;
            return d.spp >= kCoalesceUpTo ? trc_flush(ctx) : TRC_OK;
        }
        TRC_TRY(trc_flush(ctx));
    }
    if (candidate) { ctx->deferred = *p; ctx->deferred_calls = 1; ctx->has_deferred = true; return TRC_OK; }
    return render_pass(ctx, p, false);
}

}  // extern "C"

// ----------------------------------------------------------------------- render_pass, step by step
// (what they decide for one launch: RenderLaunch, trc_launch.hpp)
// The kernel's view of the context and of the call
static void launch_params(const trc_ctx* ctx, const trc_params* p, KRender& kp) {
    kp.ks = ctx->ks;
    if (ctx->knobs.descend_min > 0) kp.ks.sc.descend_min = (uint32_t)ctx->knobs.descend_min;      // A/B knob
    kp.cam = ctx->cam;
    kp.ambient[0] = ctx->ambient[0]; kp.ambient[1] = ctx->ambient[1]; kp.ambient[2] = ctx->ambient[2];
    kp.env_rgb = ctx->d_envmap; kp.env_w = ctx->env_w; kp.env_h = ctx->env_h;
    if (ctx->tex_active()) { kp.tex_texels = ctx->d_tex_texels; kp.tex_desc = ctx->d_tex_desc; kp.n_tex = ctx->n_tex; }   // the _tex kernels
    kp.fr.rng = ctx->d_rng; kp.fr.accum = ctx->d_accum; kp.fr.width = ctx->width; kp.fr.height = ctx->height;
    kp.spp = p->spp; kp.max_depth = p->max_depth; kp.frame0 = p->frame0;
    kp.view_height = (p->view_height != 0 && p->view_height < ctx->height) ? p->view_height : ctx->height;
    kp.stats = ctx->d_stats;
    // An instrumented launch (one wavefront per SIMD, counters in every loop) is no measurement of the production kernels'
    // blocks: its durations go to a scratch array, and it neither reads nor changes what the context knows about block costs.
    kp.block_cost = (p->flags & TRC_FLAG_COLLECT_STATS) ? ctx->d_cost_scratch : ctx->d_block_cost;
    kp.cost_div = std::max(1u, 4u * std::min(p->spp, 1u << 28));
    kp.density = ctx->d_density;
    kp.dinfo = ctx->dinfo;
    kp.occupancy = ctx->d_occupancy;
}

// Launch geometry.  One 8x8 block per wavefront fills the GPU when there are many more blocks than wavefront slots
// (32 400 blocks for 4 096 slots at 1080p).  A rank that owns 1/N of the frame (strong scaling) has about one block
// per slot: the launch then lasts as long as its slowest wavefront, and a wavefront is as slow as the union of its
// 64 pixels' branches.  4x4 blocks on 16 lanes give 4x the wavefronts, each with a quarter of the pixels to wait
// for -- the same pixels, the same arithmetic per pixel (TRC_FLAG_SMALL_BLOCKS forces it, _LARGE_BLOCKS forbids it).
static trc_status launch_geometry(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    const uint32_t nranks = p->tile_nranks ? p->tile_nranks : 1;
    uint32_t blk_shift = 3;
    r.fits = ctx->width <= 65535u * 4u && ctx->height <= 65535u * 4u;
    if ((p->flags & TRC_FLAG_SMALL_BLOCKS) && r.fits) blk_shift = 2;
    if (ctx->knobs.force_blk_shift > 0) blk_shift = std::min(3u, (uint32_t)ctx->knobs.force_blk_shift - 1u);   // measurement knob: 2^k x 2^k pixel blocks
    TRC_TRY(trc_ensure_tiles(ctx, nranks, p->tile_rank, p->view_height, blk_shift, true));
    r.blocks8 = blk_shift == 3 ? ctx->n_tiles : ctx->n_tiles >> (2u * (3u - blk_shift));      // of the list as it is: a tile mask may have shortened it
    KRender& kp = r.kp;
    kp.tiles = ctx->d_tiles;
    kp.blk_shift = blk_shift;
    // launches of few samples per pixel give every wavefront a strip of consecutive blocks (k_render_strip); the unit of the
    // adaptive order is then the strip, and durations recorded for another strip length say nothing
    kp.n_tiles = ctx->n_tiles;
    kp.strip = 1;
    if (!r.stats) {
        // blocks per wavefront, measured at 1920x1080 (wall ms for 64 samples in launches of 1 / 4 spp) with the pooled
        // pixels of k_render_strip: strip 2: 37.6 / 28.4, 3: 36.6 / 29.7, 4: 37.5 / 31.5, >= 5: 38.8 / 35.6 -- longer strips
        // leave too few workgroups (the frame has 32 400 blocks for 4 096 wavefront slots); one block per wavefront: 80.8 / 33.0
        uint32_t want = p->spp <= 2 ? 3u : p->spp < 8 ? 2u : 1u;
        if (ctx->knobs.strip_len > 0) want = (uint32_t)ctx->knobs.strip_len;   // A/B knob: blocks per wavefront, any spp
        const uint32_t slots = (uint32_t)ctx->cu_count * 16u;
        const uint32_t room = ctx->n_tiles / (slots + slots / 2u);          // keep >= 1.5 workgroups per slot
        kp.strip = std::max(1u, std::min(want, room));
        // test knob: exactly this many blocks per wavefront whatever the room (a frame of a few blocks runs the strip kernels: the
        // cap above is a matter of speed, the kernels bound every strip by the block list themselves)
        if (ctx->knobs.strip_force > 0) kp.strip = std::min((uint32_t)ctx->knobs.strip_force, std::max(1u, ctx->n_tiles));
        if (r.rays || r.params) kp.strip = 1;       // TRC_FLAG_CAMERA_RAYS, TRC_FLAG_MATERIAL_PARAMS: one block per one-wavefront workgroup is the only shape (choose_kernel)
    }
    r.quarters_ok = kp.strip == 1 && blk_shift == 3;
    kp.cost_stride = r.quarters_ok ? kCostSlots : 1u;
    return TRC_OK;
}

// Samples of the cold head this pass is split into (see kColdHeadSpp), or 0: the pass runs as one launch
static uint32_t cold_head_spp(const trc_ctx* ctx, const trc_params* p, const RenderLaunch& r, bool inner) {
    const uint32_t head = std::max(kColdHeadSpp, (uint32_t)ctx->knobs.probe_spp);
    const bool cold = !inner && !ctx->cost_valid && !r.stats && !ctx->knobs.no_cold_probe && !(p->flags & TRC_FLAG_FIXED_ORDER) && r.kp.strip == 1 &&
                      p->spp >= 2u * head;
    return cold ? head : 0u;
}
// Stages: the cold head, then -- where plenty of samples remain (four times the stage's) -- up to two more passes of
// doubling length, each ordered and planned by its predecessor, then the rest.  A 64-sample launch is head + rest
// (a third pass costs its drain: 21.8 -> 22.1 ms); a 256-sample launch is 8 + 16 + 32 + 200, which lets the split
// plan's K ramp 16 -> 40 -> 76 INSIDE the first launch: config 3 431 -> 362 ms (and 331 at the second launch
// instead of 368), config 4 220 -> 210, an eighth of config 3 290 -> 221 (knob head_stages = n caps the passes)
static trc_status render_cold_head(trc_ctx* ctx, const trc_params* p, uint32_t head) {
    trc_params r = *p;
    uint32_t stage = head, done = 0;
    const uint32_t max_stages = ctx->knobs.head_stages > 0 ? (uint32_t)ctx->knobs.head_stages : 3u;
    for (uint32_t k = 0; k < max_stages && p->spp - done >= (k == 0 ? 2u : 4u) * stage; ++k, stage *= 2u) {
        trc_params h = *p;
        h.spp = stage; h.frame0 = p->frame0 + done;
        TRC_TRY(render_pass(ctx, &h, true));
        ctx->launches--;                   // one trc_render call = one launch in trc_stats
        if (k == 0) ctx->cost_head_age = 1;
        done += stage;
    }
    r.spp = p->spp - done; r.frame0 = p->frame0 + done;
    return render_pass(ctx, &r, true);
}

// ... of a launch under TRC_FLAG_CAMERA_RAYS: the entry of the ray kernels' own tables (trc_render_rays.hpp) by tree residence, integrator,
// active image textures and per-triangle materials.  One block per one-wavefront workgroup (launch_geometry: strip 1): no dense kernel, no
// persistent workgroups; the LDS of a tree read from memory is planned as for any such kernel.
static trc_status choose_rays_kernel(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    KRender& kp = r.kp;
    const int integrator = (int)p->integrator;
    const bool tex = ctx->tex_active();
    const RenderRaysKernels& table = ctx->tri_materials ? (ctx->lds_scene ? trimat::render_rays_lds : trimat::render_rays_mem)
                                                        : (ctx->lds_scene ? render_rays_lds : render_rays_mem);
    r.dense = r.pwg = false;
    const bool env = r.light == Light::Env;                      // TRC_FLAG_ENV_LIGHT besides (render_check: traceMIS, a map set)
    r.kern = env ? table.env[tex ? 1 : 0] : table.one[integrator == TRC_INTEGRATOR_MIS ? 1 : 0][tex ? 1 : 0];
    if (!r.kern.fn) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "no camera-ray kernel for this integrator");
    ctx->last_kernel.shape = 0u;                                 // trc_debug_last_kernel, trc_debug_last_camera_rays
    ctx->last_kernel.variant = (uint32_t)(env ? (tex ? kVariantEnvTex : kVariantEnv) : tex ? kVariantTex : kVariantPlain);
    ctx->last_kernel.lds_resident = ctx->lds_scene ? 1u : 0u;
    ctx->last_kernel.tri_materials = ctx->tri_materials ? 1u : 0u;
    ctx->last_kernel.strip = kp.strip;
    ctx->last_kernel.camera_rays = 1u;
    ctx->last_kernel.material_params = 0u;
    ctx->last_kernel.count++;
    if (!ctx->lds_scene) TRC_TRY(plan_launch_lds(ctx, kp.ks.sc, r.kern, hybrid_stack(integrator)));
    r.lds = dyn_lds_bytes(kp.ks.sc, false);
    r.wave_slots = (uint32_t)ctx->cu_count * 4u * (uint32_t)r.kern.waves;
    trc_ctx::LastFit& fit = ctx->last_fit;
    fit.fn = r.kern.fn; fit.block = kBlock; fit.waves = (uint32_t)r.kern.waves; fit.lds = r.lds;
    fit.planned_per_cu = 4u * fit.waves;
    TRC_TRY(resident_workgroups(ctx, fit.fn, fit.block, fit.lds, &fit.per_cu));
    return TRC_OK;
}

// ... of a launch under TRC_FLAG_MATERIAL_PARAMS: the entry of the parameter kernels' own tables (trc_render_params.hpp), chosen and planned
// as choose_rays_kernel does it
static trc_status choose_params_kernel(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    KRender& kp = r.kp;
    const int integrator = (int)p->integrator;
    const bool tex = ctx->tex_active();
    const RenderParamsKernels& table = ctx->tri_materials ? (ctx->lds_scene ? trimat::render_params_lds : trimat::render_params_mem)
                                                          : (ctx->lds_scene ? render_params_lds : render_params_mem);
    r.dense = r.pwg = false;
    r.kern = table.one[integrator == TRC_INTEGRATOR_MIS ? 1 : 0][tex ? 1 : 0];
    if (!r.kern.fn) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "no material-parameter kernel for this integrator");
    ctx->last_kernel.shape = 0u;                                 // trc_debug_last_kernel, trc_debug_last_material_params
    ctx->last_kernel.variant = (uint32_t)(tex ? kVariantTex : kVariantPlain);
    ctx->last_kernel.lds_resident = ctx->lds_scene ? 1u : 0u;
    ctx->last_kernel.tri_materials = ctx->tri_materials ? 1u : 0u;
    ctx->last_kernel.strip = kp.strip;
    ctx->last_kernel.camera_rays = 0u;
    ctx->last_kernel.material_params = 1u;
    ctx->last_kernel.count++;
    if (!ctx->lds_scene) TRC_TRY(plan_launch_lds(ctx, kp.ks.sc, r.kern, hybrid_stack(integrator)));
    r.lds = dyn_lds_bytes(kp.ks.sc, false);
    r.wave_slots = (uint32_t)ctx->cu_count * 4u * (uint32_t)r.kern.waves;
    trc_ctx::LastFit& fit = ctx->last_fit;
    fit.fn = r.kern.fn; fit.block = kBlock; fit.waves = (uint32_t)r.kern.waves; fit.lds = r.lds;
    fit.planned_per_cu = 4u * fit.waves;
    TRC_TRY(resident_workgroups(ctx, fit.fn, fit.block, fit.lds, &fit.per_cu));
    return TRC_OK;
}

// Kernel choice: k_render_dense, persistent workgroups, strips or one block per one-wavefront workgroup; the entry of the kernel
// table that runs it; its LDS (the plan of a tree read from memory, the rows of parked per-pixel state, the bytes per workgroup).
static trc_status choose_kernel(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    KRender& kp = r.kp;
    const int integrator = (int)p->integrator;
    const RenderKernels& family = render_family(ctx->lds_scene, p->integrator, ctx->tri_materials);
    const RenderKernel& render_dense = ctx->tri_materials ? trimat::render_dense : ::render_dense;
    const bool tex = ctx->tex_active();
    if (r.rays) return choose_rays_kernel(ctx, p, r);
    if (r.params) return choose_params_kernel(ctx, p, r);
    const RenderVariant variant = r.light == Light::Mesh ? (tex ? kVariantMeshTex : kVariantMesh) : r.light == Light::Env ? (tex ? kVariantEnvTex : kVariantEnv)
                                : tex ? kVariantTex : r.sobol ? kVariantSobol : r.stats ? kVariantStats : kVariantPlain;
    // a whole frame's worth of blocks per wavefront slot: the LDS-resident tracePath kernel at one more wavefront per SIMD -- where the
    // CU holds (the runtime's answer) the workgroups the kernel is compiled for, with their memo rows
    r.dense = ctx->lds_scene && integrator == TRC_INTEGRATOR_PATH && !r.stats && !r.sobol && !ctx->tex_active() && kp.strip == 1 && !ctx->knobs.no_dense &&
              ctx->n_tiles >= (uint32_t)TRC_DENSE_MIN_BLOCKS_PER_SLOT * (uint32_t)ctx->cu_count * 4u * render_dense.waves;
    uint32_t dense_per_cu = 0;
    if (r.dense) {
        TRC_TRY(resident_workgroups(ctx, render_dense.fn, kBlock, dyn_lds_bytes(kp.ks.sc, false) + (size_t)dense_lds_rows() * kBlock * 4u, &dense_per_cu));
        r.dense = dense_per_cu >= 4u * (uint32_t)render_dense.waves;
    }
    uint32_t park_rows = r.dense ? dense_lds_rows() : 0u;      // LDS rows of parked per-pixel state and of the primary-replay memo (render_block)
    const bool mem_plan = !r.stats && !ctx->lds_scene;                   // trees read from memory: the LDS is planned per launch
    if (mem_plan && !ctx->knobs.no_pwg && kp.strip == 1 && ctx->lds_prefix_ok) {       // no_pwg: A/B knob
        r.pwg_waves = (uint32_t)pwg_waves(integrator);
        park_rows = pwg_park_rows(integrator);
        r.pwg = plan_pwg_lds(ctx, kp.ks.sc, r.pwg_waves, (uint32_t)pwg_per_cu(integrator), hybrid_stack(integrator), pwg_stack_lds_levels(integrator), park_rows);
        if (!r.pwg) park_rows = 0u;
    }
    r.kern = r.dense ? render_dense : (r.pwg ? family.pwg : kp.strip > 1 ? family.strip : family.one)[variant];
    if (!r.kern.fn) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "no render kernel for this integrator, flags and launch shape");
    ctx->last_kernel.shape = r.dense ? 3u : r.pwg ? 2u : kp.strip > 1 ? 1u : 0u;                 // trc_debug_last_kernel
    ctx->last_kernel.variant = r.dense ? (uint32_t)kVariantPlain : (uint32_t)variant;
    ctx->last_kernel.lds_resident = ctx->lds_scene ? 1u : 0u;
    ctx->last_kernel.tri_materials = ctx->tri_materials ? 1u : 0u;
    ctx->last_kernel.strip = kp.strip;
    ctx->last_kernel.camera_rays = 0u;
    ctx->last_kernel.material_params = 0u;
    ctx->last_kernel.count++;
    if (mem_plan && !r.pwg) TRC_TRY(plan_launch_lds(ctx, kp.ks.sc, r.kern, hybrid_stack(integrator)));
    r.lds = r.pwg ? pwg_lds_bytes(kp.ks.sc, r.pwg_waves, park_rows)
                  : dyn_lds_bytes(kp.ks.sc, r.stats) + (r.dense ? (size_t)park_rows * kBlock * 4 : 0u);
    // wavefront slots of the kernel this launch runs (the split plan's model, trc_debug_launch_shape): k_render_dense's are the workgroups
    // the runtime says a CU holds of it; the other kernels count the waves they are compiled for, strip and persistent-workgroup
    // launches the one-wavefront kernel's, as they always have (a strip launch plans nothing; the persistent ones' default is the same).
    const uint32_t per_cu = r.dense ? dense_per_cu : 4u * (uint32_t)family.one[kVariantPlain].waves;
    r.wave_slots = (uint32_t)ctx->cu_count * per_cu;
    trc_ctx::LastFit& fit = ctx->last_fit;
    fit.fn = r.kern.fn; fit.block = r.pwg ? 64u * r.pwg_waves : kBlock; fit.waves = (uint32_t)r.kern.waves; fit.lds = r.lds;
    fit.planned_per_cu = r.pwg ? (uint32_t)pwg_per_cu(integrator) : 4u * fit.waves;
    TRC_TRY(resident_workgroups(ctx, fit.fn, fit.block, fit.lds, &fit.per_cu));
    return TRC_OK;
}

// Per-launch buffers and the grid: the Sobol' tables, the traversal-stack rows of a tree read from memory (per wavefront), the
// persistent workgroups' block queue
static trc_status launch_buffers(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    KRender& kp = r.kp;
    if (r.sobol) {
        TRC_TRY(ensure_sobol_tables(ctx, kp.sobol_m));
        kp.sobol32 = ctx->d_sobol32;
        kp.sobol_vdc = ctx->d_sobol_vdc;
    }
    if (r.pwg) {                    // workgroups the GPU holds at once, of the workgroup's wavefronts
        r.block = 64u * r.pwg_waves;
        r.grid = std::min((uint32_t)ctx->cu_count * (uint32_t)pwg_per_cu((int)p->integrator), (r.grid_cap + r.pwg_waves - 1) / r.pwg_waves);   // small frames: no idle workgroups
    } else r.grid = kp.strip > 1 ? (ctx->n_tiles + kp.strip - 1) / kp.strip : r.grid_cap;
    if (!r.stats && !ctx->lds_scene) {
        const size_t rows = kp.ks.sc.stack_ovf_rows;
        const size_t need = rows * kBlock * sizeof(uint32_t) * (r.pwg ? (size_t)r.grid * r.pwg_waves : (size_t)r.grid_cap);   // rows per wavefront
        TRC_TRY(trc_grow_buffer(ctx, ctx->d_stack_ovf, ctx->stack_ovf_bytes, need, "hipMalloc traversal-stack overflow rows"));
        kp.stack_ovf = ctx->d_stack_ovf;
    }
    // the primary-replay memo rows of the kernels that keep them in global memory (trc_render_config.hpp), per wavefront as above
    const size_t memo_rows = r.stats || r.sobol || r.light != Light::None ? 0u : r.pwg ? pwg_memo_rows((int)p->integrator) : (r.dense && TRC_REPLAY_DENSE_GLOBAL) ? (size_t)TRC_REPLAY_DENSE : 0u;
    if (memo_rows) {
        const size_t need = memo_rows * kBlock * sizeof(uint32_t) * (r.pwg ? (size_t)r.grid * r.pwg_waves : (size_t)r.grid_cap);
        TRC_TRY(trc_grow_buffer(ctx, ctx->d_memo, ctx->memo_bytes, need, "hipMalloc primary-replay memo rows"));
        kp.memo = ctx->d_memo;
    }
    kp.replay = ctx->knobs.no_primary_replay ? 0u : (uint32_t)(ctx->knobs.replay_min_lanes > 0 ? ctx->knobs.replay_min_lanes : TRC_REPLAY_MIN_LANES);
    kp.replay_chain = (uint32_t)(ctx->knobs.replay_chain > 0 ? ctx->knobs.replay_chain : TRC_REPLAY_CHAIN);
    if (r.pwg) {
        if (!ctx->d_queue && hipMalloc((void**)&ctx->d_queue, sizeof(uint32_t)) != hipSuccess) return trc_fail(ctx, TRC_ERR_OOM, "hipMalloc block queue");
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_queue, 0, sizeof(uint32_t), ctx->stream));
        kp.queue = ctx->d_queue;
    }
    return TRC_OK;
}

// The launch, between two events (its duration: trc_stats.kernel_ms, and the block costs' clock)
static trc_status timed_launch(trc_ctx* ctx, const RenderLaunch& r) {
    HIP_TRY(ctx, hipGetLastError());     // the order / sort / memset launches above
    hipEvent_t e0 = trc_get_event(ctx), e1 = trc_get_event(ctx);
    auto give_back = [&]() { if (e0) ctx->event_pool.push_back(e0); if (e1) ctx->event_pool.push_back(e1); };
    if (!e0 || !e1) { give_back(); return trc_fail(ctx, TRC_ERR_HIP, "hipEventCreate failed"); }
    hipError_t le = hipEventRecord(e0, ctx->stream);
    if (le == hipSuccess) le = launch_render(ctx, r);
    if (le == hipSuccess) le = hipEventRecord(e1, ctx->stream);
    if (le != hipSuccess) { give_back(); return trc_fail(ctx, TRC_ERR_HIP, std::string("k_render launch: ") + hipGetErrorString(le)); }
    ctx->pending.emplace_back(e0, e1);
    ctx->launches++;
    return TRC_OK;
}

static trc_status render_pass(trc_ctx* ctx, const trc_params* p, bool inner) {
    RenderLaunch r;
    TRC_TRY(render_check(ctx, p, &r.kp.sobol_m));
    if (p->spp == 0) return TRC_OK;
    TRC_TRY(trc_refit_settle(ctx));      // ks.root_box of a trc_update_vertices just before
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    trc_collect_finished_events(ctx);        // before any launch of this call: it may consume a "not ready" sticky error
    r.stats = (p->flags & TRC_FLAG_COLLECT_STATS) != 0;
    r.sobol = (p->flags & TRC_FLAG_SOBOL) != 0;
    r.rays = (p->flags & TRC_FLAG_CAMERA_RAYS) != 0;
    r.params = (p->flags & TRC_FLAG_MATERIAL_PARAMS) != 0;
    r.light = (p->flags & TRC_FLAG_MESH_LIGHTS) ? Light::Mesh : (p->flags & TRC_FLAG_ENV_LIGHT) ? Light::Env : Light::None;      // (render_check: never both)
    if (r.light == Light::Env) r.el = trc_env_light_view(ctx);
    if (r.light == Light::Mesh) r.ml = trc_mesh_light_view(ctx);
    TRC_TRY(launch_geometry(ctx, p, r));
    if (ctx->n_tiles == 0) return TRC_OK;
    if (trc_dyn_lds_bytes(ctx, r.stats) > 160 * 1024) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "traversal stack exceeds the 160 KB LDS of a CU");
    launch_params(ctx, p, r.kp);
    drop_stale_costs(ctx, p, r);
    if (const uint32_t head = cold_head_spp(ctx, p, r, inner)) return render_cold_head(ctx, p, head);
    TRC_TRY(choose_kernel(ctx, p, r));
    TRC_TRY(schedule_blocks(ctx, p, r));
    TRC_TRY(launch_buffers(ctx, p, r));
    return timed_launch(ctx, r);
}

extern "C" {
// developer diagnostic: camera rays answered from the primary-replay memo since the last trc_reset_stats (tracer_abi.h)
trc_status trc_debug_primary_replays(trc_ctx* ctx, uint64_t* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long h[kStatCount];
    TRC_TRY(trc_read_stats_sum(ctx, h, kStatCount));
    *out = h[kStatReplays];
    return TRC_OK;
}

// developer diagnostic: the chain bound and the work bound of the last launch (tracer_abi.h)
trc_status trc_debug_launch_shape(trc_ctx* ctx, trc_launch_shape* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, ctx->device) != hipSuccess || khz <= 0) khz = 2400000;
    out->clock_mhz = khz / 1000.0;
    out->wave_slots = ctx->last_wave_slots;
    const uint32_t n = ctx->cost_strip > 1 ? (ctx->n_tiles + ctx->cost_strip - 1) / ctx->cost_strip : ctx->n_tiles;
    if (n == 0 || !ctx->d_block_cost || !ctx->last_cost_div) return TRC_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t stride = ctx->cost_quarters ? kCostSlots : 1u;
    std::vector<uint32_t> c((size_t)n * stride), sp(n, 0u), qs((size_t)n * 4u, 0u);
    TRC_TRY(trc_copy_to_host(ctx, c.data(), ctx->d_block_cost, c.size() * 4, ctx->stream));
    if (stride != 1u && ctx->split_live) {
        TRC_TRY(trc_copy_to_host(ctx, sp.data(), ctx->d_split, (size_t)n * 4, ctx->stream));
        TRC_TRY(trc_copy_to_host(ctx, qs.data(), ctx->d_qsplit, (size_t)n * 16, ctx->stream));
    }
    uint64_t sum = 0, longest = 0;
    uint32_t entries = 0;
    auto item = [&](uint32_t v) { sum += v; longest = std::max<uint64_t>(longest, v); entries++; };
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t* q = &c[(size_t)i * stride];
        if (!sp[i]) { item(q[0]); continue; }
        for_each_part(qs.data(), i, [&](uint32_t slot) { item(q[slot]); });
    }
    const double to_ms = (double)ctx->last_cost_div / ((double)khz);      // cost units -> shader clocks -> ms
    out->entries = entries;
    out->longest_entry_ms = (double)longest * to_ms;
    out->sum_entries_ms = (double)sum * to_ms;
    out->work_over_slots_ms = out->wave_slots ? out->sum_entries_ms / out->wave_slots : 0.0;
    return TRC_OK;
}

}  // extern "C"
