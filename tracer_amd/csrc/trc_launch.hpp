// trc_launch.hpp -- what the render pass (trc_render_pass.hip) and the launch schedule (trc_schedule.hip) share: the
// decisions of one launch, the walk over the parts a block ran as, and the schedule's two steps of render_pass.
#pragma once

#include "trc_ctx.hpp"
#include "trc_render_config.hpp"

// qsplit[4 i + q]: bit 0 = quarter q of block i ran as four sixteenths in the last launch, bits 4..7 = sixteenth s of it ran as four
// single pixels (round 6).  for_each_part visits the cost slot of every part block i ran as (trc_ctx.hpp: slot = launch code - 1).
constexpr uint32_t kPixelBit = 4u;
template <class F>
__host__ __device__ __forceinline__ void for_each_part(const uint32_t* qsplit, uint32_t i, F&& f) {
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t m = qsplit[4u * i + q];
        if (!(m & 1u)) { f(q); continue; }
        for (uint32_t s4 = 0; s4 < 4u; ++s4) {
            if ((m >> (kPixelBit + s4)) & 1u) { for (uint32_t p4 = 0; p4 < 4u; ++p4) f(20u + 16u * q + 4u * s4 + p4); }
            else f(4u + 4u * q + s4);
        }
    }
}

// What render_pass decides for one launch.  Each step reads what the steps before it decided.
struct RenderLaunch {
    KRender kp{};                       // the kernel's parameters
    bool stats = false, sobol = false;  // TRC_FLAG_COLLECT_STATS, TRC_FLAG_SOBOL
    bool rays = false;                  // TRC_FLAG_CAMERA_RAYS: the kernels of trc_render_rays.hpp, which read a sample's camera ray from the context's ray sets
    bool params = false;                // TRC_FLAG_MATERIAL_PARAMS: the kernels of trc_render_params.hpp, which read a lobe's parameters from the context's table
    Light light = Light::None;          // TRC_FLAG_ENV_LIGHT / TRC_FLAG_MESH_LIGHTS: the light the kernels sample besides the squares ...
    EnvLight el{};                      // ... Light::Env: the map's sampling tables (the k_render*_env kernels' second half of KRenderEnv)
    MeshLight ml{};                     // ... Light::Mesh: the emissive triangles' (the k_render*_mesh kernels' second half of KRenderMesh)
    bool fits = false;                  // launch_geometry: the frame's edges allow 4x4 blocks ...
    uint64_t blocks8 = 0;               // ... 8x8 blocks in this rank's share
    bool quarters_ok = false;           // ... the list's blocks are 8x8: costs live in kCostSlots slots per block
    bool dense = false, pwg = false;    // choose_kernel: k_render_dense, persistent workgroups ...
    RenderKernel kern{};                // ... the entry of the kernel table that runs
    uint32_t wave_slots = 0;            // ... wavefront slots of the split plan's model
    uint32_t pwg_waves = 0;             // ... wavefronts per persistent workgroup
    size_t lds = 0;                     // ... dynamic LDS per workgroup
    uint32_t grid_cap = 0;              // schedule_blocks: workgroups of a one-block-per-workgroup launch
    bool planned = false;               // ... the split plan (or every block as quarters) makes this launch's list
    uint32_t grid = 0, block = kBlock;  // launch_buffers
};

// trc_schedule.hip: the steps of render_pass that own the block costs
void drop_stale_costs(trc_ctx* ctx, const trc_params* p, const RenderLaunch& r);
trc_status schedule_blocks(trc_ctx* ctx, const trc_params* p, RenderLaunch& r);
