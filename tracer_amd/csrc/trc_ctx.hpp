// trc_ctx.hpp -- pieces shared by the translation units of libtracer_amd.so (trc_abi.hip, trc_render_pass.hip, trc_schedule.hip,
// trc_group.hip, trc_sppm.hip ...): kernel-side scene staging helpers, the context struct, the error helpers and what one unit
// calls of another.
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "tracer_abi.h"
#ifdef TRC_TEST_HOOKS
#include "tracer_test_hooks.h"      // libtracer_amd_hooks.so: the product's sources + the test hooks
#endif
#include "dev_integrator.hpp"

using namespace trcdev;

// ======================================================================= kernels
extern __shared__ __attribute__((aligned(16))) uint32_t trc_smem[];

// launch-list entries (KRender::order): index into the block list | part code << 25.  Code 0: the whole block; 1..4: its 4x4
// quarter code - 1 (x fastest) on 16 lanes; 5..20: the 2x2 sixteenth (code - 5) & 3 of quarter (code - 5) >> 2 on 4 lanes;
// 21..84 (round 6): ONE pixel on one lane -- pixel (code - 21) & 3 of sixteenth ((code - 21) >> 2) & 3 of quarter (code - 21) >> 4:
// the floor of a pixel's sample chain, for the shares of a frame that end on a single 4-lane wavefront.
constexpr uint32_t kLaunchCodeShift = 25u;
constexpr uint32_t kLaunchIndexMask = (1u << kLaunchCodeShift) - 1u;
// duration slots per 8x8 block of a list that may be split (KRender::cost_stride): 0..3 the quarters (0 also the whole
// block), 4..19 the sixteenths, 20..83 the pixels -- slot = code - 1
constexpr uint32_t kCostSlots = 84u;
constexpr uint32_t kPlanWords = 12u;          // trc_schedule.hip k_plan_split

struct KScene {
    DScene sc;
    float root_box[6];
};

struct KRender {
    KScene ks;
    DCamera cam;
    float ambient[3];
    const float* env_rgb; uint32_t env_w, env_h;      // environment map (null: constant `ambient`)
    DFrame fr;
    uint32_t spp, max_depth, frame0;
    uint32_t view_height;               // rows per view of a stacked frame (= frame height for a single view)
    const uint32_t* tiles;              // tx | ty << 16, one per workgroup
    const float* density;               // traceVolume: GridDensity medium grid (null when absent)
    trc_GridDensityInfo dinfo;
    const uint8_t* occupancy;           // ... and its 4x4x4-brick occupancy (dev_integrator.hpp::grid_sample)
    unsigned long long* stats;          // kStatCount counters
    uint32_t* stack_ovf;                // (stack_depth - stack_lds) rows of 64 entries per wavefront (null: the stack is all LDS)
    uint32_t* queue;                    // k_render_pwg: next position of the launch order to hand out
    uint32_t blk_shift;                 // log2 of the pixel-block edge of one wavefront: 3 (8x8, 64 lanes) or 2 (4x4, 16 lanes)
    uint32_t n_tiles, strip;            // k_render_strip: blocks in `tiles`, consecutive blocks per wavefront (1: k_render)
    const uint32_t* order;              // launch list: order[slot] = index into `tiles` | part code << kLaunchCodeShift (null: identity; codes
                                        // above: cost-adaptive block size, k_plan_split).  k_render_strip: strip indices, no codes.
    const uint32_t* n_launch;           // device word: entries of `order` in this launch (null: n_tiles); workgroups past it exit
    uint32_t cost_div;                  // a block's cost = its wavefront's duration in shader clocks / cost_div (= 4 x spp: per sample)
    uint32_t* block_cost;               // duration of each block in this launch (the next launch's sort key): slot kCostSlots * tile +
                                        // max(code - 1, 0) when the list may be split (cost_stride = kCostSlots), else slot `tile`
    uint32_t cost_stride;
    const uint32_t* sobol32;            // TRC_FLAG_SOBOL: [40][52] generator matrices (null otherwise)
    const uint64_t* sobol_vdc;          // ... [52] VdCSobolMatrices[m - 1] + [52] VdCSobolMatricesInv[m - 1]
    uint32_t sobol_m;                   // ... log2Resolution
    const float* tex_texels;            // image textures (k_render*_tex only): texel pool, RGB float, rows bottom-up ...
    const uint4* tex_desc;              // ... {first texel, w, h, 0} per image
    uint32_t n_tex;                     // ... images uploaded
    uint32_t* memo;                     // primary replay (trc_render_config.hpp): the memo rows per wavefront of the kernels that keep them in global memory
    uint32_t replay;                    // ... 0: every camera ray walks (knob no_primary_replay); n: a trip of the loop shades replayed hits alone where >= n lanes hold one
    uint32_t replay_chain;              // ... and at most this many such trips in a row
};

// the kernels of TRC_FLAG_ENV_LIGHT (k_render*_env) take the environment map's sampling tables besides: a struct of their own, so
// that every other kernel keeps its parameter block
struct KRenderEnv {
    KRender kp;
    EnvLight el;
};

// ... and the kernels of TRC_FLAG_MESH_LIGHTS (k_render*_mesh) the emissive triangles' sampling tables
struct KRenderMesh {
    KRender kp;
    MeshLight ml;
};

// ... and the kernels of TRC_FLAG_CAMERA_RAYS (k_render_rays, trc_render_rays.hpp) the ray sets a sample's camera ray is read from
struct KRenderRays {
    KRender kp;
    const trc_ray* rays;                // n_sets sets of W x H records: pixel (x, y) of set k at (k * H + y) * W + x
    uint32_t n_sets;
};

// ... and the kernels of TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT (k_render_rays_env) both: the map's tables as in KRenderEnv, then the ray sets
struct KRenderRaysEnv {
    KRender kp;
    EnvLight el;
    const trc_ray* rays;
    uint32_t n_sets;
};

// ... and the kernels of TRC_FLAG_MATERIAL_PARAMS (k_render_params, trc_render_params.hpp) the table of trc_material_params
struct KRenderParams {
    KRender kp;
    const float4* table;                // three float4 per material, in the order of the scene's material list
};

struct KTrace {
    KScene ks;
    const trc_ray* rays;
    trc_hit* hits;
    uint32_t n;
};

// cooperative copy of the blob prefix (prims, materials, top fat nodes) into LDS
__device__ __forceinline__ const uint32_t* stage_scene(const DScene& sc) {
    const uint4* src = reinterpret_cast<const uint4*>(sc.blob);
    uint4* dst = reinterpret_cast<uint4*>(trc_smem);
    const uint32_t n16 = sc.lds_dwords >> 2;
    for (uint32_t i = threadIdx.x; i < n16; i += kBlock) dst[i] = src[i];
    __syncthreads();
    return trc_smem;
}

// this lane's column of the traversal stack (one row per entry); the instrumented kernels keep a second region of the
// same size for the levels
__device__ __forceinline__ uint32_t* lane_stack(const DScene& sc) { return trc_smem + sc.lds_dwords + threadIdx.x; }
__device__ __forceinline__ uint32_t* lane_lvstack(const DScene& sc) { return trc_smem + sc.lds_dwords + sc.stack_lds * kBlock + threadIdx.x; }

__device__ __forceinline__ SceneRef make_scene_ref(const DScene& sc, const uint32_t* small_base) {
    SceneRef S;
    S.small_base = small_base;
    S.blob = sc.blob;
    S.off_nodes = sc.off_nodes; S.off_spheres = sc.off_spheres; S.off_squares = sc.off_squares;
    S.off_cubes = sc.off_cubes; S.off_materials = sc.off_materials;
    S.off_tripos = sc.off_tripos; S.off_triattr = sc.off_triattr;
    S.n_lds_nodes = sc.n_lds_nodes;
    S.stack_lds = sc.stack_lds;
    S.stack_cap = sc.stack_depth;
    S.ovf = nullptr;
    S.descend_min = sc.descend_min;
    return S;
}

// Work counters live in kStatRows copies of one row; a wavefront adds to row (its index mod kStatRows) and the reader
// sums the rows.  One row for everybody meant one 64-bit atomic per wavefront and counter on ONE address: device-scope
// atomics on a line are served one after the other (~12 ns each, measured), and 32 400 wavefronts x 3 counters held a
// 1-spp frame at 1.2 ms and the SPPM camera pass at 0.4 ms -- whatever the kernels did.
constexpr uint32_t kStatRows = 1024;
constexpr uint32_t kStatRowStride = ((kStatCount + 3 * kProfCount + 15) / 16) * 16;      // 64-bit words; rows start on 128-byte lines
static_assert(kStatRowStride <= 64, "k_stats_sum sums a row with one 64-thread workgroup");
__device__ __forceinline__ unsigned long long* stat_row(unsigned long long* stats, uint32_t wave_index) {
    return stats + (size_t)(wave_index & (kStatRows - 1u)) * kStatRowStride;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}


// ======================================================================= context
struct SppmState;   // trc_sppm.hip
struct DenoiseState;   // trc_denoise.hip

// What the calls that move a scene's vertices keep between them (trc_refit.hip, trc_deform.hip, trc_normals.hip; trc_refit.hpp is what
// the three share).  Made on demand by the first call that needs it, freed with the scene (trc_refit_free); a rebuild drops `maps` alone
struct RefitState {
    struct Maps {                           // follow the tree's topology and numbering (trc_refit_free_maps)
        uint32_t* d_parent = nullptr;       // [n_nodes] fat node that holds this fat node's box (root: itself)
        uint32_t* d_refnode = nullptr;      // [n_nodes] device-built trees: this fat node's record in d_bvh_ref
        uint32_t* d_arrive = nullptr;       // [n_nodes] arrival counters of the single-launch climb (zero between updates)
        float* d_root = nullptr;            // [12] the refitted root box in words 0..5 (the root's store zeroes 6 and 7); word kPoseCountWord:
                                            // the overflows of every pose, skin and morph so far, never put back to zero
        uint32_t* d_primslot = nullptr;     // [n_spheres + n_squares + n_cubes] in that order: 2 * fat node + slot of the leaf that names the primitive, kTagNone: no leaf does
        std::vector<uint32_t> levels;       // first fat node of every depth, and n_nodes behind them (the fat nodes are numbered by depth)
        uint32_t count_seen = 0;            // the counter word as last read back: a call's count is the difference to it
    } maps;
    // ev[0], ev[1]: around the kernels of the family's last call, whichever it was; ev[2]: behind the root box's copy to h_readback.
    // ONE pair serves every call because every entry point opens with trc_flush: the flush settles a pending refit, and with it reads
    // that refit's time (trc_refit_read_time), before the pair is recorded again.  A trc_recompute_normals leaves nothing pending, so
    // its time is read when it is asked for, or never
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms = 0.0f; bool timed = false;    // device time of those kernels (trc_debug_refit_ms); timed: still to be read from ev[0], ev[1]
    bool pending = false, posed = false;    // ks.root_box still waits for ev[2] (trc_refit_settle); the counter word travels with it
    uint32_t overflows = 0;                 // of the last pose, skin or morph (trc_debug_pose_overflows)
    trc_TriangleVertex* d_rest = nullptr;   // the rest copy of d_verts, made by the first pose, skin or morph of a scene
    trc_pose* d_pose_table = nullptr; size_t pose_table_bytes = 0;      // of the last trc_pose_vertices
    // trc_skin_bind: vertex first + i has d_influences[i] (null: no binding); trc_morph_bind: target k, vertex first + i has d_deltas[k * count + i]
    struct Skin { trc_skin_influence* d_influences = nullptr; uint32_t first = 0, count = 0, max_bone = 0; } skin;
    struct Morph { trc_morph_delta* d_deltas = nullptr; uint32_t first = 0, count = 0, n_targets = 0; } morph;
    trc_skin_bone* d_palette = nullptr; size_t palette_bytes = 0;       // of the last skin, alone or on top of a morph
    void* d_morph_active = nullptr; size_t morph_active_bytes = 0;      // the active list of the last morph (morph_check.hpp)
    void* d_prim_stage = nullptr; size_t prim_stage_bytes = 0;          // the caller's records of the last trc_update_primitives: spheres, squares, cubes
    // trc_recompute_normals: d_adj_corners[d_adj_offsets[v] .. d_adj_offsets[v + 1]) are the k with d_idx[k] == v, ascending
    uint32_t* d_adj_offsets = nullptr; uint32_t* d_adj_corners = nullptr;      // [n_vertex + 1], [n_index]
};

struct trc_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::string error;

    // scene
    bool has_scene = false;
    KScene ks{};
    uint32_t* d_blob = nullptr;
    size_t blob_bytes = 0;
    bool lds_scene = false;
    bool lds_prefix_ok = false;         // the fat nodes are in top-of-tree-first order: any prefix may be staged
    uint32_t* d_stack_ovf = nullptr;    // traversal-stack overflow rows of the render launches (deep trees only)
    size_t stack_ovf_bytes = 0;
    uint32_t* d_memo = nullptr;         // primary-replay memo rows of the render launches that keep them in global memory
    size_t memo_bytes = 0;
    uint32_t* d_queue = nullptr;        // block queue head of the persistent-workgroup launches
    trc_BVH* d_bvh_ref = nullptr;    // tree built by trc_upload_scene_lbvh / _sah / _device or trc_rebuild_tree, reference array layout (trc_download_bvh)
    uint32_t n_bvh_ref = 0, lbvh_height = 0;
    float lbvh_build_ms = 0.0f;
    // trc_set_triangle_visibility (trc_visibility.hpp): one byte per triangle, 1 = visible, padded to 16 bytes; null until the first call of a
    // scene makes the mask explicit (a triangle is visible iff a leaf of the tree names it).  Freed with the scene (trc_release_scene)
    uint8_t* d_vis = nullptr;
    float vis_leaf_ms = 0.0f;        // device time of the last call's leaf-list stage: mask, partition, leaf records (trc_debug_visibility_ms)
    // the scene's vertex and index arrays, kept beside the blob by every upload (trc_repack_triangles), and what the calls that move
    // them keep (RefitState); all freed with the blob (trc_refit_free)
    trc_TriangleVertex* d_verts = nullptr; uint32_t* d_idx = nullptr; uint32_t n_vertex = 0;
    RefitState refit;
    float* d_density = nullptr;      // GridDensity medium (trc_upload_density)
    uint8_t* d_occupancy = nullptr;
    trc_GridDensityInfo dinfo{};

    bool has_camera = false;
    DCamera cam{};
    float ambient[3] = {0, 0, 0};
    float* d_envmap = nullptr; uint32_t env_w = 0, env_h = 0;
    uint32_t* d_sobol32 = nullptr; uint64_t* d_sobol_vdc = nullptr; uint32_t sobol_m = ~0u;   // TRC_FLAG_SOBOL tables
    // image textures (trc_upload_textures): texel pool + descriptors, and the smallest textureIndex of the scene's Image
    // materials (~0u: none) -- an image is active, and the _tex kernels launched, when it is below n_tex
    float* d_tex_texels = nullptr; uint4* d_tex_desc = nullptr; uint32_t n_tex = 0; uint32_t scene_min_image = ~0u;
    bool tex_active() const { return scene_min_image < n_tex; }
    bool tri_materials = false;         // trc_upload_triangle_materials holds an array: launch the render kernels' trimat twins
    // TRC_FLAG_ENV_LIGHT: the map's sampling tables (trc_envlight.hip), built at the first flagged render after trc_set_environment_map
    uint8_t* d_envl = nullptr; double envl_total = 0.0; float envl_build_ms = 0.0f;
    Light cost_light = Light::None;     // the light variant of the launches whose block costs are recorded (drop_stale_costs)
    // TRC_FLAG_MESH_LIGHTS: the emissive triangles' sampling tables (trc_meshlight.hip), built at the first flagged render after a scene
    // or triangle-material upload.  mesh_built with d_meshl null: a scene without a light triangle (or without a triangle)
    uint8_t* d_meshl = nullptr; bool mesh_built = false; uint32_t mesh_n_lights = 0; double mesh_total = 0.0;

    // frame
    uint32_t width = 0, height = 0;
    uint32_t* d_rng = nullptr;
    float* d_accum = nullptr;
    // TRC_FLAG_CAMERA_RAYS (trc_camera_rays.hip): n_ray_sets sets of W x H trc_ray records, set-major then row-major (null: no rays in
    // force).  Sized by the frame: trc_release_frame.  cost_rays: the recorded block costs are a flagged launch's (drop_stale_costs)
    trc_ray* d_cam_rays = nullptr; uint32_t n_ray_sets = 0;
    bool cost_rays = false;
    // TRC_FLAG_MATERIAL_PARAMS (trc_material_params.hip): n_mparams records of trc_material_params, one per material of the scene (null: no
    // table in force).  Belongs to the scene: trc_release_scene.  cost_params: the recorded block costs are a flagged launch's
    trc_material_params* d_mparams = nullptr; uint32_t n_mparams = 0;
    bool cost_params = false;
    // ... ray_gen: which rays these are -- the next number whenever they are replaced or dropped (trc_camera_rays_release: trc_upload_camera_rays,
    // trc_generate_camera_rays, trc_clear_camera_rays, trc_resize), whatever the new ones' bits: the denoiser under trc_denoise_guide_rays compares it
    uint64_t ray_gen = 0;

    // tiles for (nranks, rank)
    uint32_t* d_tiles = nullptr;
    // adaptive launch order: duration of every block in the previous launch -> most expensive blocks first in the next
    uint32_t* d_block_cost = nullptr;
    uint32_t* d_order_keys[2] = {nullptr, nullptr};
    uint32_t* d_order_vals[2] = {nullptr, nullptr};
    uint32_t* d_order_hist = nullptr;
    // cost-adaptive block size (trc_schedule.hip: k_plan_split): which 8x8 blocks the last launch ran as four 4x4 quarters, the
    // launch list with the quarters spliced in, and the plan {quarters' parents K, entries}
    uint32_t* d_split = nullptr;
    uint32_t* d_whole = nullptr;        // cost of a block when it last ran whole (while it runs as quarters)
    uint32_t* d_cost_est = nullptr;     // per cost slot: the shortest duration seen lately (k_filter_costs)
    uint32_t* d_qsplit = nullptr;       // [4 n] quarter q of block i ran as four sixteenths in the last launch ...
    uint32_t* d_qwhole = nullptr;       // [4 n] ... and what it cost when it last ran as one quarter
    uint32_t* d_swhole = nullptr;       // [16 n] what a sixteenth cost when it last ran as one (while it runs as four pixels: bits 4..7 of qsplit)
    uint32_t* d_launch = nullptr;
    uint32_t* d_plan = nullptr;
    uint32_t* d_cost_scratch = nullptr;  // durations of instrumented launches (never read)
    uint32_t* d_plan_gather = nullptr;  // k_plan_gather's dense per-rank arrays (6 words per block)
    uint32_t plan_streak = 0, plan_reused = 0, plan_n = 0, plan_wave_slots = 0, plan_grid_cap = 0; bool plan_split_mode = false;   // plan reuse (trc_render)
    uint32_t launch_cap = 0;            // entries d_launch holds = the grid of a launch that may split
    bool split_live = false;            // d_split holds flags of the last launch's plan (else all zero)
    bool cost_quarters = false;         // d_block_cost / d_split describe a launch made with cost_stride 4
    bool cost_valid = false; uint32_t cost_strip = 1;
    uint32_t last_cost_div = 0, last_wave_slots = 0;     // of the last render launch (trc_debug_launch_shape)
    // what choose_kernel (trc_render_pass.hip) decided for the last render launch (trc_debug_last_kernel, tracer_test_hooks.h): the
    // launch shape (0 one block per one-wavefront workgroup, 1 strips, 2 persistent workgroups, 3 k_render_dense), the RenderVariant,
    // whether the whole tree was staged in LDS, whether the per-triangle-material twins ran, and the strip length; launches counted
    // camera_rays: it was a kernel of TRC_FLAG_CAMERA_RAYS (trc_debug_last_camera_rays)
    // material_params: it was a kernel of TRC_FLAG_MATERIAL_PARAMS (trc_debug_last_material_params)
    struct LastKernel { uint32_t shape = 0, variant = 0, lds_resident = 0, tri_materials = 0, strip = 0, count = 0, camera_rays = 0, material_params = 0; } last_kernel;
    // ... and how that launch sits on a CU (trc_debug_last_residency): the kernel, its workgroup size and dynamic LDS, the workgroups per
    // CU its plan is for (4 x the waves of its launch bounds; the persistent workgroups' per-CU count) and the runtime's answer
    struct LastFit { const void* fn = nullptr; uint32_t block = 0, waves = 0, planned_per_cu = 0, per_cu = 0; size_t lds = 0; } last_fit;
    trc_params deferred{}; bool has_deferred = false; uint64_t deferred_calls = 0;   // a launch of few samples kept for coalescing (trc_render)
    int cost_head_age = 0;                    // 1: the costs are a cold head's (trc_render), 2: the launch after it ran on them
    bool cost_fresh_next = false;             // the next ordered launch takes the last launch's raw durations as its costs (trc_set_camera, policy 2)
    uint32_t cost_integrator = 0xFFFFFFFFu;   // integrator the recorded costs belong to
    const uint32_t* d_stale_order = nullptr;     // the launch order of the view before the camera moved: the next cold pass's prior
    const uint32_t* d_last_order = nullptr; uint32_t order_age = 0;     // most recent sorted order (short launches reuse it)
    int cu_count = 0;
    uint32_t n_tiles = 0, tiles_nranks = 0, tiles_rank = 0, tiles_view_height = 0, tiles_blk_shift = 3;
    // trc_set_tile_mask / trc_render_adaptive (trc_adaptive.hip): the TRC_TILE x TRC_TILE tiles of the frame that trc_render's block list
    // keeps, one byte per tile, row-major (empty: every tile).  mask_gen names the mask in the block list's cache key (0: no mask; every
    // trc_set_tile_mask takes the next number), tiles_mask_gen is the list's.  d_mask mirrors tile_mask on the device once a kernel needs it
    // (all ones without a mask; mask_on_device: it holds the current one).  Everything here is sized by the frame: trc_release_frame
    struct Adaptive {
        std::vector<uint8_t> tile_mask;
        uint64_t mask_gen = 0, next_gen = 0;
        uint64_t shrinks_from = ~0ull;      // the mask_gen (0: no mask) whose tiles this mask is a subset of: trc_ensure_tiles may carry that list's costs over
        uint8_t* d_mask = nullptr; bool mask_on_device = false;
        float* d_snapshot = nullptr;        // A of trc_tile_snapshot: the accumulator plane as it was (16 B per pixel, made at first use)
        float* d_error = nullptr;           // E_t of trc_tile_error (zero until a tile's first estimate)
        uint32_t* d_samples = nullptr; bool has_samples = false;      // n_t of the last trc_render_adaptive (k_tile_decide)
        uint32_t* d_decide = nullptr;       // k_tile_decide's two words: tiles still active, the largest E_t's bits
    } adaptive;
    uint64_t tiles_mask_gen = 0;

    // stats
    unsigned long long* d_stats = nullptr;       // kStatRows rows of kStatRowStride counters (stat_row)
    unsigned long long* d_stats_sum = nullptr;   // their sum, made by trc_get_stats / trc_debug_profile
    uint64_t launches = 0;
    double kernel_ms = 0.0;
    double schedule_ms = 0.0;                                   // launch-list kernels (order, sort, plan) of those launches
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_sched;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // per-launch event pairs not yet read
    std::vector<hipEvent_t> event_pool;

    // RCCL
    void* comm = nullptr;
    int nranks = 1, rank = 0;
    float* d_reduce_recv = nullptr;
    // pipelined compose (trc_group_reduce_accum_async): second accumulator, communication stream, and per-buffer
    // "reduce finished" events (ev_busy belongs to d_accum, ev_busy_alt to d_accum_alt; they swap with the buffers)
    float* d_accum_alt = nullptr;
    float* d_composed = nullptr;        // buffer holding the most recently composed frame (one of the two)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_rendered = nullptr, ev_busy = nullptr, ev_busy_alt = nullptr;
    bool busy = false, busy_alt = false;
    // sample-sharded compose (trc_group_compose_samples): the slices received from the ranks, and the composed slices
    float* d_shard_in = nullptr; float* d_shard_out = nullptr; size_t shard_px = 0; int shard_nranks = 0;
    // ... and the pipelined form's snapshot of the accumulator (trc_group_compose_samples_async), free again at ev_snapshot_free
    float* d_shard_src = nullptr; hipEvent_t ev_snapshot_free = nullptr; bool snapshot_busy = false;

    SppmState* sppm = nullptr;       // trc_sppm.hip
    DenoiseState* denoise = nullptr; // trc_denoise.hip (allocated by the first trc_denoise after trc_resize)
    bool track_motion = false;       // trc_denoise_track_motion: context state like the textures -- survives scene uploads and trc_resize; what it owns lives in `denoise`
    bool guide_rays = false;         // trc_denoise_guide_rays: the same kind of state -- the G-buffer is walked along set 0 of the ray sets (d_cam_rays), not along the camera's ray

    // caller-supplied collectives (trc_group_set_collectives) instead of an RCCL communicator
    trc_collectives coll{};
    bool coll_active = false;
    void* h_stage = nullptr;            // pinned staging buffer of host-staged collectives
    size_t h_stage_bytes = 0;
    // 1 KB of pinned host memory (trc_readback_alloc) for the two read-backs that are ASYNCHRONOUS on purpose: the per-level counter block of
    // trc_upload_scene_sah (sah_build_topology) and the refitted root box of trc_update_vertices (trc_refit_tail).  The root box's copy is still
    // in flight when trc_update_vertices returns; that is safe only because every entry point calls trc_flush first, which settles it
    // (trc_refit_settle) before anything else writes or reads the buffer -- and why every synchronous read-back goes through h_xfer instead
    uint32_t* h_readback = nullptr;
    char* h_xfer = nullptr;             // 2 x kXferChunk bytes of pinned host memory, synchronous users only: trc_copy_*, trc_read_to_host
    hipEvent_t ev_xfer[2] = {nullptr, nullptr};

    // A/B and test knobs, per context: defaults from the environment at trc_create (TRC_NO_LDS_FIT, TRC_STACK_LDS_LEVELS,
    // TRC_STRIP_LEN, TRC_NO_PWG, TRC_SPPM_SERIAL_CAMERA), changed through trc_debug_set
    // (trc_abi.hip: kKnobs names each once, for both)
    struct Knobs {
        int no_lds_fit = 0;             // the whole traversal stack in LDS, no node prefix fitted to the launch (plan_launch_lds)
        int stack_lds_levels = 0;       // entries of a lane's stack kept in LDS (0: the kernel family's default)
        int strip_len = 0;              // blocks per wavefront of a strip launch, any spp, capped by the room (launch_geometry)
        int no_pwg = 0;                 // no persistent workgroups on trees read from memory
        int sppm_serial_camera = 0;     // SPPM: the camera pass on the context's stream, not beside the photon pass
        int sppm_timing = 0;            // SPPM: event pairs around a frame's photon, hash / table and refine passes, added to kernel_ms
        int force_blk_shift = 0;        // k + 1: 2^k x 2^k pixel blocks whatever the flags say
        int no_split = 0;               // every block whole: no cost-adaptive block size
        int no_cost_filter = 0;         // order and plan by the last launch's raw durations
        int no_cold_probe = 0;          // a first launch runs as one pass, no cold head
        int probe_spp = 0;              // samples of the cold head (at least kColdHeadSpp)
        int no_plan_reuse = 0;          // a settled list is planned again at every launch
        int no_coalesce = 0;            // launches of few samples go at once
        int no_dense = 0;               // never k_render_dense
        int head_stages = 0;            // passes of a staged cold head (0: 3)
        int descend_min = 0;            // DScene::descend_min of the launches (0: the upload's)
        int camera_policy = 0;          // trc_set_camera: 0 keep the costs under a small move, 1 always forget, 2 / 3 always keep (filtered / raw)
        int no_primary_replay = 0;      // every camera ray walks
        int replay_min_lanes = 0;       // lanes that must hold a replayed hit for a replay trip (0: TRC_REPLAY_MIN_LANES)
        int replay_chain = 0;           // replay trips in a row (0: TRC_REPLAY_CHAIN)
        int mesh_light_pick = 1;        // TRC_FLAG_MESH_LIGHTS: 0 never picks the mesh's light sample (the BSDF-only estimator)
        int refit_single = 0;           // trc_update_vertices: refit in a single launch (trc_refit.hip)
        int skin_no_lds = 0;            // trc_skin_vertices: the bones gathered from memory whatever the palette's size (trc_deform.hip)
        int strip_force = 0;            // tests: exactly this many blocks per wavefront (launch_geometry)
        int mask_forgets_costs = 0;     // a tile mask that only clears tiles forgets the block costs like any new list (trc_ensure_tiles)
    } knobs;
    // render kernels that were granted > 64 KB of dynamic LDS on THIS context's device (trc_render_pass.hip: launch_render):
    // hipFuncSetAttribute applies to the current device only, so the grant is per context, not per process
    std::vector<const void*> lds_granted;
    // workgroups of a render kernel that one CU holds at once, as the runtime answers for (kernel, workgroup size, dynamic LDS) on this
    // context's device (trc_render_pass.hip: resident_workgroups); asked once per combination
    struct Residency { const void* fn; uint32_t block; size_t lds; uint32_t per_cu; };
    std::vector<Residency> residency;

    bool grouped() const { return comm != nullptr || coll_active; }
};


inline trc_status trc_fail(trc_ctx* ctx, trc_status s, const std::string& msg) {
    if (ctx) ctx->error = msg;
    return s;
}
#define HIP_TRY(ctx, expr)                                                                 \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return trc_fail(ctx, e_ == hipErrorOutOfMemory ? TRC_ERR_OOM : TRC_ERR_HIP,     \
                            std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

// ... and the same for the library's own status: evaluates `expr` once and returns it from the enclosing function unless it is TRC_OK
#define TRC_TRY(expr)                                                                      \
    do {                                                                                   \
        const trc_status s_ = (expr);                                                      \
        if (s_ != TRC_OK) return s_;                                                       \
    } while (0)

// A device allocation that lives no longer than the function that makes it: freed on every path out.  release() hands the
// pointer to a longer-lived owner.  A failed hipMalloc leaves no sticky error behind for a later, unrelated call to report.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p); }
    trc_status alloc(trc_ctx* ctx, size_t bytes, const char* what) {
        if (hipMalloc(&p, bytes) == hipSuccess) return TRC_OK;
        p = nullptr;
        (void)hipGetLastError();
        return trc_fail(ctx, TRC_ERR_OOM, std::string("hipMalloc ") + what);
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void* release() { void* q = p; p = nullptr; return q; }
};

// The many temporary device arrays of one function (the tree builds), each a DevBuf: freed on every path out, failing as DevBuf::alloc does.
// reserve() first makes ONE allocation that the arrays are then carved from, 256 bytes apart at least; an array that no longer fits, or
// every array when the reservation itself found no room, gets a buffer of its own as before.  Why: hipFree waits for the device and
// unmaps, 0.18 ms apiece on an MI355X -- the thirty-odd arrays of a tree build over 1 M leaves took 5.5 ms to free, a single one of their
// total size (203 MB) 0.23 ms (profiles/r19/rebuild_tree.txt)
struct DevBufs {
    std::vector<DevBuf> bufs;
    char* arena = nullptr; size_t arena_bytes = 0, arena_used = 0;
    void reserve(size_t bytes) {
        bufs.emplace_back();
        if (hipMalloc(&bufs.back().p, bytes) != hipSuccess) { bufs.back().p = nullptr; (void)hipGetLastError(); return; }
        arena = bufs.back().as<char>(); arena_bytes = bytes; arena_used = 0;
    }
    template <class T> trc_status alloc(trc_ctx* ctx, T** out, size_t count, const char* what) {      // `count` elements, at least one
        const size_t bytes = (count ? count : 1) * sizeof(T), padded = (bytes + 255u) & ~(size_t)255u;
        if (padded <= arena_bytes - arena_used) { *out = reinterpret_cast<T*>(arena + arena_used); arena_used += padded; return TRC_OK; }
        bufs.emplace_back();
        TRC_TRY(bufs.back().alloc(ctx, bytes, what));
        *out = bufs.back().as<T>();
        return TRC_OK;
    }
};

// A buffer of the context that must hold at least `need` bytes (`have`: what it holds): a launch in flight may still use the old
// one, so the stream is synchronised before it goes.  `msg`: the error text of a failed allocation (TRC_ERR_OOM, nothing kept)
template <class T>
inline trc_status trc_grow_buffer(trc_ctx* ctx, T*& buf, size_t& have, size_t need, const char* msg) {
    if (need <= have) return TRC_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(buf); buf = nullptr;
    have = 0;
    if (hipMalloc((void**)&buf, need) != hipSuccess) return trc_fail(ctx, TRC_ERR_OOM, msg);
    have = need;
    return TRC_OK;
}

// RCCL entry points, resolved at run time (dlopen) so the library loads where RCCL is absent
struct IdBlob { char internal[TRC_UNIQUE_ID_BYTES]; };   // ncclUniqueId, passed by value
struct Rccl {
    void* handle = nullptr;
    bool ready = false;              // every entry point below resolved
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, IdBlob, int) = nullptr;
    int (*Reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    // point-to-point (the sample-sharded compose): optional, a library without them still composes tiles
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
extern Rccl g_rccl;
bool trc_load_rccl(std::string& err);
// ncclDataType_t / ncclRedOp_t ordinals (rccl.h:448-466)
constexpr int kNcclUint8 = 1, kNcclUint32 = 3, kNcclFloat = 7, kNcclSum = 0, kNcclMax = 2, kNcclMin = 3;

// The three collectives the group calls need, in place on device buffers, through RCCL (ctx->comm) or the caller's table
// (ctx->coll; host-staged tables get the data in pinned host memory).  `what` names the call in error messages.
trc_status trc_coll_reduce(trc_ctx* ctx, void* buf, size_t count, int dtype, int op, int root, hipStream_t st, const char* what);
trc_status trc_coll_allreduce(trc_ctx* ctx, void* buf, size_t count, int dtype, int op, hipStream_t st, const char* what);
trc_status trc_coll_allgather(trc_ctx* ctx, void* buf, size_t bytes_per_rank, hipStream_t st, const char* what);

// Transfers between device memory and memory the CALLER (or a std::vector of ours) owns.  They do not hand the host pointer to the HIP
// runtime: a copy to / from pageable memory makes the runtime pin the caller's pages in place, and under many processes sharing the GPU a
// D2H copy into freshly mapped pages was seen to leave whole ranges of the destination untouched -- zeros where the device buffer,
// downloaded again, had the data (round 6: tests/campaigns/sppm_stress.py reproduced round 5's "unwritten photon records" 380 times in
// 9 000 scenes, every one of them a transfer, none a kernel).  So the bytes go through the context's own pinned
// buffer, two chunks of kXferChunk in flight, and are copied to / from the caller's memory by the CPU.  Synchronous: on return the
// transfer is complete (`st` is synchronised up to it): no caller synchronises again.
constexpr size_t kXferChunk = 4u << 20;
trc_status trc_copy_to_host(trc_ctx* ctx, void* host, const void* dev, size_t bytes, hipStream_t st);
trc_status trc_copy_to_device(trc_ctx* ctx, void* dev, const void* host, size_t bytes, hipStream_t st);
// ... and the library's own small read-backs (flags, counters, a root box): a few device ranges into host variables through the same buffer with
// ONE synchronisation of `st`, kXferChunk bytes in all.  Reports a launch that failed before it too: TRC_ERR_HIP, "<what>: <hipGetErrorString>"
struct trc_read_item { void* host; const void* dev; size_t bytes; };
trc_status trc_read_to_host(trc_ctx* ctx, hipStream_t st, const char* what, std::initializer_list<trc_read_item> items);

// tiles owned by `rank` of `nranks` (XCD-aware order) uploaded into ctx->d_tiles; shared by render and SPPM
// `masked`: of those, the blocks of tiles that trc_set_tile_mask kept (trc_render); SPPM's list is keyed without the mask
trc_status trc_ensure_tiles(trc_ctx* ctx, uint32_t nranks, uint32_t rank, uint32_t view_height = 0, uint32_t blk_shift = 3, bool masked = false);
// trc_render_pass.hip: one pass of trc_render, launched at once (never kept for coalescing): the passes of trc_render_adaptive
trc_status trc_render_now(trc_ctx* ctx, const trc_params* p);
// trc_adaptive.hip: the tile mask (null: every tile) becomes the context's; frees what trc_set_tile_mask and the estimate own (trc_release_frame)
trc_status trc_adopt_tile_mask(trc_ctx* ctx, const uint8_t* mask, bool on_device = false);      // `mask`: trc_tile_count bytes; on_device: d_mask already holds it
void trc_adaptive_release(trc_ctx* ctx);
void trc_material_params_release(trc_ctx* ctx);  // trc_material_params.hip: frees the table of TRC_FLAG_MATERIAL_PARAMS (trc_release_scene); the block costs of a flagged launch go with it
void trc_camera_rays_release(trc_ctx* ctx);      // trc_camera_rays.hip: frees the ray sets of TRC_FLAG_CAMERA_RAYS (trc_release_frame); the block costs of a flagged launch go with them
inline uint32_t trc_tiles_x(const trc_ctx* ctx) { return (ctx->width + TRC_TILE - 1) / TRC_TILE; }
inline uint32_t trc_tile_count(const trc_ctx* ctx) { return trc_tiles_x(ctx) * ((ctx->height + TRC_TILE - 1) / TRC_TILE); }
size_t trc_dyn_lds_bytes(const trc_ctx* ctx, bool stats);
// trc_lbvh.hip: stable radix sort of (key, value) pairs on the 24 low key bits, three of the tree builds' 8-bit passes; *result: the buffer that holds it
void trc_sort_pairs24(hipStream_t st, uint32_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* digit_base, uint32_t n, int* result);
// ... and on the `bits` low key bits (rounded up to whole passes), for keys known to be small: trc_recompute_normals' vertex indices
void trc_sort_pairs(hipStream_t st, uint32_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* digit_base, uint32_t n, uint32_t bits, int* result);
uint32_t trc_sort_hist_words(uint32_t n);
// trc_tonemap's output stage on any W*H RGBA32F plane of the context (the accumulator, the denoised frame); synchronous
trc_status trc_tonemap_plane(trc_ctx* ctx, const float* plane, uint8_t* rgba8, float* exposure_out);
// launches what trc_render kept back, and settles what trc_update_vertices left for later.  Every other entry point opens with
// TRC_TRY(trc_flush(ctx)), before it looks at its arguments: a kept launch of few samples goes first (trc_render), and its status is the
// entry point's.  trc_flush(nullptr) is TRC_OK: the null-context check that follows answers
trc_status trc_flush(trc_ctx* ctx);
hipEvent_t trc_get_event(trc_ctx* ctx);   // from the context's pool (null on failure); pairs go to ctx->pending
// A timed section of a stream between two events of the context's pool, which get them back on every path out.  stop() closes it; ms() is its
// device time once the stream has been synchronised.  No event to be had: nothing fails, the section took 0 ms (lbvh_build_ms, envl_build_ms: diagnostics)
struct TimedSection {
    trc_ctx* ctx; hipStream_t st; hipEvent_t e0, e1;
    TimedSection(trc_ctx* c, hipStream_t s) : ctx(c), st(s), e0(trc_get_event(c)), e1(trc_get_event(c)) { if (e0 && e1) (void)hipEventRecord(e0, st); }
    ~TimedSection() { if (e0) ctx->event_pool.push_back(e0); if (e1) ctx->event_pool.push_back(e1); }
    void stop() { if (e0 && e1) (void)hipEventRecord(e1, st); }
    float ms() const { float v = 0.0f; return e0 && e1 && hipEventElapsedTime(&v, e0, e1) == hipSuccess ? v : 0.0f; }
};
void trc_sppm_release(trc_ctx* ctx);   // frees ctx->sppm (no-op when absent)
void trc_denoise_release(trc_ctx* ctx);      // frees ctx->denoise: its G-buffers, planes and history (no-op when absent)
// smallest textureIndex of the scene's Image materials (~0u: none); recorded by every scene upload (trc_ctx::scene_min_image)
inline uint32_t trc_scene_min_image(const trc_scene* s) {
    uint32_t m = ~0u;
    for (uint32_t i = 0; i < s->n_material; ++i)
        if (s->materials[i].textureInfo.type == TRC_TEX_IMAGE && s->materials[i].textureInfo.textureIndex < m) m = s->materials[i].textureInfo.textureIndex;
    return m;
}
void trc_denoise_invalidate(trc_ctx* ctx);   // trc_picture_changed: the G-buffer is stale and the history dropped
// trc_scene_changed, the kinds that leave every surface where the history can follow it: with tracking on (trc_denoise_track_motion) the
// G-buffer is stale and the history STAYS, and where `geometry` (vertices or analytic primitives) is about to move and no call has moved any
// since the last trc_denoise, the vertex positions and the blob's primitive section are copied into the snapshot on the context's stream
// first.  Tracking off: trc_denoise_invalidate
void trc_denoise_moved(trc_ctx* ctx, bool geometry);
void trc_denoise_scene_released(trc_ctx* ctx);      // trc_release_scene: the snapshot is sized by the scene that goes
// TRC_FLAG_ENV_LIGHT (trc_envlight.hip): build the current map's sampling tables if they are not built (TRC_ERR_OOM: nothing kept), free
// them, and the kernels' view of them
trc_status trc_env_light_build(trc_ctx* ctx);
void trc_env_light_free(trc_ctx* ctx);
EnvLight trc_env_light_view(const trc_ctx* ctx);
// TRC_FLAG_MESH_LIGHTS (trc_meshlight.hip): the same three for the scene's emissive triangles
trc_status trc_mesh_light_build(trc_ctx* ctx);
void trc_mesh_light_free(trc_ctx* ctx);
MeshLight trc_mesh_light_view(const trc_ctx* ctx);
constexpr size_t kReadbackBytes = 1024;
inline trc_status trc_readback_alloc(trc_ctx* ctx) {    // ctx->h_readback, once per context; freed by trc_destroy
    if (!ctx->h_readback) HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_readback, kReadbackBytes, hipHostMallocDefault));
    return TRC_OK;
}
trc_status trc_refit_settle_pending(trc_ctx* ctx); // trc_refit.hip: what the last trc_update_vertices / trc_pose_vertices / trc_skin_vertices / trc_morph_vertices / trc_update_primitives left for later (ks.root_box, the overflow count)
inline trc_status trc_refit_settle(trc_ctx* ctx) { return ctx->refit.pending ? trc_refit_settle_pending(ctx) : TRC_OK; }
void trc_refit_free(trc_ctx* ctx);                 // trc_refit.hip: the kept vertex / index arrays, rest copy, skin and morph bindings, the normals' adjacency and the refit maps (no-op when absent)
void trc_refit_free_maps(trc_ctx* ctx);            // trc_refit.hip: the refit maps alone (parent, level table, record map): the tree's topology changed (trc_rebuild_tree)
void trc_sppm_order_after_camera(trc_ctx* ctx);   // context stream waits for a camera pass running ahead (no-op when none)

// ----------------------------------------------------------------------- what is stale now
// Every entry point that changes what the context's caches were derived from says so through one of these three.
// trc_forget_costs: the recorded block costs and the launch orders sorted from them are another picture's -- the next launch
// measures afresh (its cold head).  Called by trc_scene_changed, by the scheduler where a launch's list is not the one the costs
// were recorded for (trc_ensure_tiles, drop_stale_costs) and by trc_debug_set.  trc_set_camera keeps a rule of its own: it carries
// the old order over as the next cold pass's prior.
inline void trc_forget_costs(trc_ctx* ctx) { ctx->cost_valid = false; ctx->d_last_order = nullptr; ctx->d_stale_order = nullptr; }
// trc_picture_changed: what a pixel shows changed -- the denoiser's G-buffer is stale and its history dropped.  Called by
// trc_scene_changed and by the entry points that change the lighting or the colours alone: trc_set_environment,
// trc_set_environment_map, trc_upload_textures.
inline void trc_picture_changed(trc_ctx* ctx) { trc_denoise_invalidate(ctx); }
// trc_scene_changed (trc_abi.hip): the geometry or its materials changed.  Every kind drops the picture (trc_picture_changed; but see
// the last three kinds below) and the
// emissive triangles' sampling tables (TRC_FLAG_MESH_LIGHTS: rebuilt when a launch asks).
//   kSceneReplaced      trc_upload_scene, upload_device_tree (trc_upload_scene_lbvh / _sah / _device), BEFORE they allocate the new
//                       scene: also forgets the block costs and releases the old scene (trc_release_scene: blob, reference-layout
//                       tree, kept vertex / index arrays and refit maps; has_scene false, every triangle material 19 again)
//                       A device tree upload that fails after that releases what it allocated of the NEW scene too, before it returns
//   kSceneMaterials     trc_upload_triangle_materials: also forgets the block costs
//   kSceneVerticesMoved trc_update_vertices, trc_pose_vertices, trc_skin_vertices, trc_morph_vertices, BEFORE anything of theirs that writes a
//                       vertex is queued: the block costs stay (the picture changed a little, as under a camera that moves a little)
//   kSceneNormalsChanged trc_recompute_normals: as kSceneVerticesMoved, but no position changes
//   kSceneTreeRebuilt   trc_rebuild_tree, once the new tree is on its way into the blob: no vertex moved, but a tie in t may now resolve to
//                       another primitive.  The block costs stay; the refit maps go (trc_refit_free_maps: the next update, pose or skin makes
//                       them for the new topology); vertex and index arrays, rest copy, bindings and triangle materials stay
//   kScenePrimitivesMoved trc_update_primitives, BEFORE its kernel is queued: in place like kSceneVerticesMoved -- the block costs stay, the
//                       mesh-light tables go
// The last four keep the denoiser's history while trc_denoise_track_motion is on (trc_denoise_moved: "moved" of either kind, "normals changed",
// "rebuilt" reach the denoiser here and nowhere else); with it off they drop the picture like every other kind.
enum SceneChange { kSceneReplaced, kSceneMaterials, kSceneVerticesMoved, kSceneNormalsChanged, kSceneTreeRebuilt, kScenePrimitivesMoved };
void trc_scene_changed(trc_ctx* ctx, SceneChange kind);
// Each device buffer is freed and nulled in one place, for the entry point that replaces it and for trc_destroy alike:
void trc_release_scene(trc_ctx* ctx);    // trc_abi.hip: what a scene upload allocates
void trc_adopt_scene(trc_ctx* ctx, KScene ks, const trc_scene* s);      // trc_abi.hip: the last step of every scene upload -- `ks` becomes the context's scene
void trc_release_frame(trc_ctx* ctx);    // trc_abi.hip: what depends on the frame size (trc_resize): frame, block list, compose buffers, SPPM, denoiser
void trc_release_tiles(trc_ctx* ctx);    // trc_schedule.hip: the block list and the arrays sized by it (trc_ensure_tiles)
void trc_collect_finished_events(trc_ctx* ctx);   // trc_abi.hip: completed event pairs into kernel_ms / schedule_ms without waiting (render_pass)
// trc_abi.hip: the first `count` words of the counters' rows summed into one (k_stats_sum of d_stats into d_stats_sum), on the host; synchronises the stream
trc_status trc_read_stats_sum(trc_ctx* ctx, unsigned long long* h, size_t count);
