// trc_render_config.hpp -- compile-time shape of the render kernels (launch bounds, persistent-workgroup geometry, stack and
// record policy per integrator), shared by the translation units that DEFINE the kernels (trc_render_lds.hip, trc_render_mem.hip)
// and the ones that plan and launch them (trc_render_pass.hip, trc_schedule.hip).  Every value is an A/B macro: make variant NAME=x DEFS=-D...
#pragma once

#include "trc_ctx.hpp"
#include "trc_lds_fit.hpp"

// "test now, build the record for the winner afterwards" (dev_intersect.hpp: trav_test_leaf<DEFER>), per tree residence
// two-level traversal stack (first entries in LDS, deeper ones in global rows: dev_intersect.hpp stack_put) per integrator, on
// trees read from memory: it is what lets LDS admit the occupancy the registers allow
#ifndef TRC_MIS_HYBRID
#define TRC_MIS_HYBRID 1
#endif
#ifndef TRC_VOLUME_HYBRID
#define TRC_VOLUME_HYBRID 0
#endif
constexpr bool hybrid_stack(int integrator) {
    return integrator == TRC_INTEGRATOR_PATH || (integrator == TRC_INTEGRATOR_MIS ? TRC_MIS_HYBRID != 0 : TRC_VOLUME_HYBRID != 0);
}
#ifndef TRC_DEFER_LDS
#define TRC_DEFER_LDS 0
#endif
#ifndef TRC_DEFER_GLOBAL
#define TRC_DEFER_GLOBAL 1
#endif

// kernelPathTracing, Render.metal:495-558.  One lane per pixel, one one-wavefront workgroup per 8x8 pixel block
// (DESIGN.md 4.1), all `spp` samples fused: RNG texel and accumulator are read and
// written ONCE per pixel instead of once per sample (64 B/pixel/sample in the reference).
// wavefronts per SIMD the register allocation aims at (launch bounds), each measured (profiles/r02/
// compiler_flags_and_occupancy.txt, lds_plan_and_stack.txt): tracePath on an LDS-resident tree fits 96 VGPRs with 2
// spilled dwords (5 waves: 21.5 -> 20.8 ms on config 2; 6 waves / 80 VGPRs: 21.3-21.6); on a tree read from memory the
// sixth wave hides more latency than its spills cost (1 M triangles: 32.8 -> 31.8 ms; 7 waves: 33.4) -- provided LDS
// lets it in (plan_launch_lds); traceMIS needs 128 (5 waves: 63.2 -> 63.7 ms on config 3), traceVolume 128 (5: 55 -> 84 ms)
#ifndef TRC_PATH_WAVES
#define TRC_PATH_WAVES 5
#endif
// ... and at 6 when the launch list is many times the wavefront slots (a whole 1080p frame: 19.85 -> 19.63 ms; its 25-52 spilled
// dwords lengthen a lone block's chain, so shares of a frame -- which end on their slowest block -- keep the 5-wave kernel:
// an eighth of config 2 5.6 against 5.9 ms).  k_render_dense: tracePath, LDS-resident tree, production, no Sobol'.
// Measured again with the primary replay in place (profiles/r17/ab_lds_fit.txt; 80 registers + 112 B of scratch per lane, 1.6 % of the
// kernel's instructions scratch accesses, against 96 + 36 B and 0.5 % at 5): 5 waves 15.20 ms where 6 with 8 memo rows run 15.73 -- but 6
// with SEVEN rows 15.10, at 0.92 of its wavefront slots busy under the counters where 8 rows had 0.82 (profiles/r17/occupancy.txt): the
// sixth wave was short of LDS more than of registers (TRC_REPLAY_DENSE below).  6 stays.
#ifndef TRC_PATH_WAVES_DENSE
#define TRC_PATH_WAVES_DENSE 6
#endif
#ifndef TRC_DENSE_MIN_BLOCKS_PER_SLOT
#define TRC_DENSE_MIN_BLOCKS_PER_SLOT 4
#endif
// tracePath on a tree read from memory: SEVEN waves per SIMD (72 registers: 90 spilled values and 160 B of scratch per lane where 64
// registers spill 116 / 200 B).  Round 4 had found seven slower than eight because a workgroup of 14 wavefronts does not pack -- the
// dispatcher deals a workgroup's wavefronts to the SIMDs from SIMD 0 on, 14 = 4 + 4 + 3 + 3, and the second workgroup would put an eighth
// wavefront on a SIMD whose registers hold seven, so only ONE was resident (41.6 ms).  Four-wavefront workgroups, seven per CU, pack
// (1 + 1 + 1 + 1 each).  Round 5, alternating builds (profiles/r05/ab_shapes_config*.txt, shapes_validate.txt): config 4 23.25 -> 22.87 ms
// per 32-spp launch, teapot x 1 / x 16 / x 256 16.80 / 22.38 / 20.68 -> 16.33 / 22.04 / 18.92 ms (the scene beyond the Infinity Cache
// gains most: -8.5 %), 168.5 against 169.6 ms as named; 4 x 8, 8 x 4 at eight waves and 4 x 6 at six are slower (23.66 / 23.36 / 26.73).
#ifndef TRC_PATH_WAVES_GLOBAL
#define TRC_PATH_WAVES_GLOBAL 7
#endif
#ifndef TRC_MIS_WAVES
#define TRC_MIS_WAVES 8              // traceMIS on a tree read from memory (latency-bound: occupancy pays, round 4)
#endif
#ifndef TRC_MIS_WAVES_LDS
#define TRC_MIS_WAVES_LDS 8          // ... and on an LDS-resident one (Cornell + spheres, 32 spp: 16.7 ms at 4 waves and 128 registers, 15.9 at 5, 15.6 at 8 with 64)
#endif
#ifndef TRC_VOLUME_WAVES
#define TRC_VOLUME_WAVES 4
#endif
// persistent workgroups (k_render_pwg): wavefronts per workgroup x workgroups per CU = the waves per CU above
#ifndef TRC_PWG_WAVES_PATH
#define TRC_PWG_WAVES_PATH 4
#endif
#ifndef TRC_PWG_PER_CU_PATH
#define TRC_PWG_PER_CU_PATH 7
#endif
#ifndef TRC_PWG_WAVES_MIS
#define TRC_PWG_WAVES_MIS 16
#endif
#ifndef TRC_PWG_PER_CU_MIS
#define TRC_PWG_PER_CU_MIS 2
#endif
#ifndef TRC_PWG_WAVES_VOLUME
#define TRC_PWG_WAVES_VOLUME 16
#endif
#ifndef TRC_PWG_PER_CU_VOLUME
#define TRC_PWG_PER_CU_VOLUME 1
#endif
#ifndef TRC_STRIP_PATH_WAVES
#define TRC_STRIP_PATH_WAVES 4
#endif
constexpr int pwg_waves(int integrator) { return integrator == TRC_INTEGRATOR_PATH ? TRC_PWG_WAVES_PATH : (integrator == TRC_INTEGRATOR_MIS ? TRC_PWG_WAVES_MIS : TRC_PWG_WAVES_VOLUME); }
// entries of a lane's traversal stack that live in LDS in a persistent-workgroup launch (deeper ones: global rows, dev_intersect.hpp
// stack_push); what the stacks leave of the workgroup's LDS share is node prefix.  tracePath 10 beside its park rows (round 6: 6 / 8 / 10:
// 23.2 / 22.1 / 21.9 ms per 32-spp launch of config 4; 16 without park rows: 22.6); traceMIS 8 (6 / 8 / 10 / 12 / 16: 41.7 / 40.1 / 40.2 / 40.4 / 41.0 ms per 32-spp launch of config 3, 294.4
// against 300.5 ms as named: its shadow rays walk with one entry per level and its 16 x 2 workgroups get 48 KB of prefix instead of 16)
// PARK (round 6, trc_render_kernels.hpp::render_block): words of a lane's LDS column hold the values that are touched only where a sample
// begins or ends (running mean, (u, v), sample counter) and the two work counters, so that they are not carried -- and spilled to scratch
// -- through the walk and the shading code of every iteration.  8 rows, or 10 with the pixel's coordinates (with 8 they are worked out
// again at the end from the launch entry, read once more).  Paid for with stack entries / node prefix; per kernel family, each measured
// (profiles/r06/ab_park_*.txt): 0 = off.
enum : uint32_t { kParkCachedX = 0, kParkCachedY, kParkCachedZ, kParkU, kParkV, kParkSample, kParkRays, kParkShaded, kParkPx, kParkPy };
#ifndef TRC_PARK_PATH
#define TRC_PARK_PATH 8          // 8 rows + 12 stack entries against 10 + 10: -0.6 % on config 4 and on the 4 M-triangle scene (ab_park_rows_config4.txt)
#endif
#ifndef TRC_PARK_MIS
#define TRC_PARK_MIS 0
#endif
#ifndef TRC_PARK_VOLUME
#define TRC_PARK_VOLUME 10       // (8: +3 %, ab_park_rows_volume.txt)
#endif
#ifndef TRC_PARK_DENSE
#define TRC_PARK_DENSE 0         // k_render_dense (the headline kernel: tracePath, whole tree in LDS): 8 rows are what six waves per SIMD leave, and they
#endif                           // take its scratch from 88 to 32 bytes per lane -- and its time from 16.57 to 17.19 ms (ab_park_dense_config2.txt):
                                 // the kernel is bound by issue, and an LDS access is an issued instruction + a wait where the spill was one too.  Off.
constexpr uint32_t pwg_park_rows(int integrator) { return integrator == TRC_INTEGRATOR_PATH ? TRC_PARK_PATH : (integrator == TRC_INTEGRATOR_MIS ? TRC_PARK_MIS : TRC_PARK_VOLUME); }
static_assert((TRC_PARK_PATH == 0 || TRC_PARK_PATH == 8 || TRC_PARK_PATH == 10) && (TRC_PARK_MIS == 0 || TRC_PARK_MIS == 8 || TRC_PARK_MIS == 10) &&
              (TRC_PARK_VOLUME == 0 || TRC_PARK_VOLUME == 8 || TRC_PARK_VOLUME == 10) && (TRC_PARK_DENSE == 0 || TRC_PARK_DENSE == 8 || TRC_PARK_DENSE == 10), "park rows: 0, 8 or 10");
// PRIMARY REPLAY (round 8, trc_render_kernels.hpp::render_block): the reference's camera has no sub-pixel jitter and its default lens has
// radius 0, so every sample of a pixel casts the same camera ray, bit for bit, and Scene::hit of it is a pure function of (scene, ray).
// A lane keeps what the integrator reads of that hit -- p, gn, tag, material | the side sn took, with 10 rows uv -- in MEMO words of a
// column of its own (row r at memo[r * kBlock]) after the first walk of a block, and a later sample whose origin has the eye's bits takes
// the record from there instead of walking.  Per kernel family, 0 = compiled out:
//   k_render_dense       7 rows of LDS behind the stack rows: tag, material, side and the replay count of a column that lost its record
//                        share ONE word (trc_lds_fit.hpp).  The headline scene's workgroup is then 3008 B of scene + 6 stack rows + 7 memo
//                        rows = 6336 B, and 24 of them -- six waves per SIMD -- fit a CU's 160 KB whether LDS is granted in 512-byte or
//                        in 1280-byte blocks; with 8 rows (6592 B) the runtime still answers 24, but the counters show 0.82 of 6144
//                        wavefront slots busy (= 0.93 of the 5376 that 21 per CU make) against 0.92 with 7, and the launch 4 % slower:
//                        15.73 -> 15.10 ms (profiles/r17/occupancy.txt, ab_lds_fit.txt; 5 waves with 8 / 10 / 7 rows: 15.20 / 15.23 / 15.23).  uv has no row: a hit whose
//                        colour reads rec.uv (a checker texture on a cube or a triangle) is not kept, and that pixel walks every sample;
//                        nor is a hit whose material or primitive index does not fit the word's 8 / 20 bits
//   k_render_pwg<path>   10 rows per wavefront in global memory, sized per launch like the overflow rows of the stack (coalesced 256 B)
// TRC_REPLAY_DENSE_GLOBAL 1 puts the dense kernel's rows in global memory too (the storage A/B).  Scheduling (knobs replay_min_lanes /
// replay_chain): where at least TRC_REPLAY_MIN_LANES lanes of a wavefront hold a replayed hit, a trip of the loop shades those lanes alone, at
// most TRC_REPLAY_CHAIN such trips between two walks; 65 lanes = the plain variant, a replayed lane sits out the next walk and nothing else.
// Config 2, ms per 64-spp launch (profiles/r08/ab_primary_replay.txt): replay off 17.5; 1 lane x 1 trip 15.6; 8 / 16 / 24 / 32 / 48 lanes 15.6 /
// 15.7 / 15.7 / 16.2 / 17.4; plain 17.6; 1 lane, trips unbounded 21.0 (pixels that replay 63 times in a row starve the walkers).
// traceMIS / traceVolume, Sobol', k_render, the strip and the instrumented kernels always walk.
enum : uint32_t { kMemoPx = 0, kMemoPy, kMemoPz, kMemoNx, kMemoNy, kMemoNz, kMemoTag, kMemoMat, kMemoU, kMemoV };
constexpr uint32_t kMemoWord = kMemoTag;           // 7 rows: tag, material, side and replay count packed into this one (trc_lds_fit.hpp)
constexpr uint32_t kMemoNone = 0xFFFFFFFFu;        // the material word of a column that holds no record (its tag word: replays so far)
constexpr uint32_t kMemoSameSide = 0x80000000u;    // material word: sn == gn (else sn == -gn: check_face)
#ifndef TRC_REPLAY_DENSE
#define TRC_REPLAY_DENSE 7
#endif
#ifndef TRC_REPLAY_DENSE_GLOBAL
#define TRC_REPLAY_DENSE_GLOBAL 0
#endif
#ifndef TRC_REPLAY_PWG_PATH
#define TRC_REPLAY_PWG_PATH 10
#endif
#ifndef TRC_REPLAY_MIN_LANES
#define TRC_REPLAY_MIN_LANES 1
#endif
#ifndef TRC_REPLAY_CHAIN
#define TRC_REPLAY_CHAIN 1
#endif
static_assert((TRC_REPLAY_DENSE == 0 || TRC_REPLAY_DENSE == 7 || TRC_REPLAY_DENSE == 8 || TRC_REPLAY_DENSE == 10) && (TRC_REPLAY_PWG_PATH == 0 || TRC_REPLAY_PWG_PATH == 10), "memo rows: 0, 7 (dense), 8 or 10 (10 wherever image textures may be live)");
constexpr uint32_t dense_lds_rows() { return (uint32_t)TRC_PARK_DENSE + (TRC_REPLAY_DENSE_GLOBAL ? 0u : (uint32_t)TRC_REPLAY_DENSE); }      // LDS rows of k_render_dense behind its stack
constexpr uint32_t pwg_memo_rows(int integrator) { return integrator == TRC_INTEGRATOR_PATH ? (uint32_t)TRC_REPLAY_PWG_PATH : 0u; }
#ifndef TRC_PWG_STACK_LDS_PATH
#define TRC_PWG_STACK_LDS_PATH (TRC_PARK_PATH == 10 ? 10 : (TRC_PARK_PATH == 8 ? 12 : 16))
#endif
#ifndef TRC_PWG_STACK_LDS_MIS
#define TRC_PWG_STACK_LDS_MIS 8
#endif
#ifndef TRC_PWG_STACK_LDS_VOLUME
#define TRC_PWG_STACK_LDS_VOLUME 16
#endif
constexpr uint32_t pwg_stack_lds_levels(int integrator) { return integrator == TRC_INTEGRATOR_MIS ? TRC_PWG_STACK_LDS_MIS : (integrator == TRC_INTEGRATOR_PATH ? TRC_PWG_STACK_LDS_PATH : TRC_PWG_STACK_LDS_VOLUME); }
constexpr int pwg_per_cu(int integrator) { return integrator == TRC_INTEGRATOR_PATH ? TRC_PWG_PER_CU_PATH : (integrator == TRC_INTEGRATOR_MIS ? TRC_PWG_PER_CU_MIS : TRC_PWG_PER_CU_VOLUME); }

// wavefronts per SIMD each kernel kind is compiled for: its __launch_bounds__ (trc_render_kernels.hpp) and what the host plans
// with (trc_render_pass.hip: the LDS plan; trc_schedule.hip: the split plan's wavefront slots) -- one value, read from the kernel table
constexpr int render_waves(bool lds, bool stats, int integrator) {      // k_render, k_render_tex (statistics: one wavefront)
    return stats ? 1 : integrator == TRC_INTEGRATOR_VOLUME ? TRC_VOLUME_WAVES
                     : integrator == TRC_INTEGRATOR_MIS ? (lds ? TRC_MIS_WAVES_LDS : TRC_MIS_WAVES) : (lds ? TRC_PATH_WAVES : TRC_PATH_WAVES_GLOBAL);
}
constexpr int strip_waves(int integrator) { return integrator == TRC_INTEGRATOR_VOLUME ? 3 : (integrator == TRC_INTEGRATOR_PATH ? TRC_STRIP_PATH_WAVES : 4); }
constexpr int pwg_simd_waves(int integrator) { return pwg_waves(integrator) * pwg_per_cu(integrator) / 4; }      // k_render_pwg

// The kernels themselves (trc_render_kernels.hpp) are instantiated in five translation units -- by tree residence and integrator family,
// so that each can be compiled with the backend options that pay for it (Makefile: EXTRA_*), and in parallel:
//   trc_render_lds.hip        tracePath, whole tree staged in LDS (Cornell scenes; the bench's kernel)       -amdgpu-use-amdgpu-trackers
//   trc_render_lds_mis.hip    traceMIS / traceVolume, whole tree staged in LDS
//   trc_render_mem_path.hip   tracePath, trees read from memory (mesh scenes)                                 -disable-machine-sink
//   trc_render_mem.hip        traceMIS, trees read from memory
//   trc_render_mem_volume.hip traceVolume, trees read from memory                                             -disable-machine-sink
// Each exports the kernel table of its families (render_kernels<LDS, INTEGRATOR>), which instantiates exactly the kernels in it;
// trc_render_pass.hip launches whatever entry a launch picks.  A null entry is a variant that does not exist.
// the kernel's parameter block: KRender, KRenderEnv (TRC_FLAG_ENV_LIGHT), KRenderMesh (TRC_FLAG_MESH_LIGHTS), KRenderRays (TRC_FLAG_CAMERA_RAYS),
// KRenderRaysEnv (TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT), KRenderParams (TRC_FLAG_MATERIAL_PARAMS)
enum RenderArgs { kArgsPlain, kArgsEnv, kArgsMesh, kArgsRays, kArgsRaysEnv, kArgsParams };
struct RenderKernel {
    const void* fn;                     // the kernel (null: no such variant)
    int waves;                          // wavefronts per SIMD of its launch bounds
    RenderArgs args;                    // ... and which parameter block launch_render hands it
};
// A table entry is made from the kernel itself, so the parameter block is checked by the compiler where the kernel is named.
// (Not constexpr: a function pointer becomes a data pointer by reinterpret_cast only.  The tables are filled when the library loads.)
inline RenderKernel render_kernel(void (*fn)(KRender), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsPlain}; }
inline RenderKernel render_kernel(void (*fn)(KRenderEnv), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsEnv}; }
inline RenderKernel render_kernel(void (*fn)(KRenderMesh), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsMesh}; }
inline RenderKernel render_kernel(void (*fn)(KRenderRays), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsRays}; }
inline RenderKernel render_kernel(void (*fn)(KRenderRaysEnv), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsRaysEnv}; }
inline RenderKernel render_kernel(void (*fn)(KRenderParams), int waves) { return {reinterpret_cast<const void*>(fn), waves, kArgsParams}; }
// TRC_FLAG_COLLECT_STATS, TRC_FLAG_SOBOL, image textures, TRC_FLAG_ENV_LIGHT (traceMIS only) without and with image textures,
// TRC_FLAG_MESH_LIGHTS (traceMIS only) without and with image textures
enum RenderVariant { kVariantPlain, kVariantStats, kVariantSobol, kVariantTex, kVariantEnv, kVariantEnvTex, kVariantMesh, kVariantMeshTex, kVariants };
struct RenderKernels {
    RenderKernel one[kVariants];        // one pixel block per one-wavefront workgroup: k_render<.., STATS, .., SOBOL>, k_render_tex
    RenderKernel strip[kVariants];      // a strip of blocks per wavefront: k_render_strip<.., SOBOL>, k_render_strip_tex (no statistics)
    RenderKernel pwg[kVariants];        // persistent workgroups, trees read from memory: k_render_pwg<.., SOBOL>, k_render_pwg_tex (no statistics)
};
extern const RenderKernels render_lds_path, render_lds_mis, render_lds_volume, render_mem_path, render_mem_mis, render_mem_volume;
extern const RenderKernel render_dense;      // k_render_dense (trc_render_lds.hip): tracePath, LDS-resident tree, production, PCG
// the same tables over the twins that read each triangle's material (trc_render_*_tm.hip; dev_intersect.hpp TRC_TRIANGLE_MATERIALS)
namespace trimat {
extern const RenderKernels render_lds_path, render_lds_mis, render_lds_volume, render_mem_path, render_mem_mis, render_mem_volume;
extern const RenderKernel render_dense;
}
// TRC_FLAG_CAMERA_RAYS: tables of their own, beside the tables above and not in them -- k_render_rays<LDS, INTEGRATOR, TEX>
// (trc_render_rays.hpp) at [tracePath 0 / traceMIS 1][image textures], one table per tree residence: trc_render_rays.hip (whole tree
// staged in LDS) and trc_render_rays_mem.hip (trees read from memory), each with the options of the units it shadows, and their twins.
// With TRC_FLAG_ENV_LIGHT besides (traceMIS only): k_render_rays_env<LDS, TEX> at env[image textures]
struct RenderRaysKernels {
    RenderKernel one[2][2];
    RenderKernel env[2];
};
extern const RenderRaysKernels render_rays_lds, render_rays_mem;
namespace trimat {
extern const RenderRaysKernels render_rays_lds, render_rays_mem;
}
// TRC_FLAG_MATERIAL_PARAMS: the same again -- k_render_params<LDS, INTEGRATOR, TEX> (trc_render_params.hpp) at [tracePath 0 / traceMIS 1]
// [image textures], one table per tree residence: trc_render_params.hip (whole tree staged in LDS) and trc_render_params_mem.hip (trees
// read from memory), each with the options of the units it shadows, and their twins
struct RenderParamsKernels {
    RenderKernel one[2][2];
};
extern const RenderParamsKernels render_params_lds, render_params_mem;
namespace trimat {
extern const RenderParamsKernels render_params_lds, render_params_mem;
}
