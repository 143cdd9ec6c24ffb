/*
 * tracer_abi.h -- the drop-in boundary of the MI355X path-tracing hot path.
 *
 * Plain C ABI: extern "C", plain pointers and sizes, no C++/torch types.
 *
 * The reference (iaomw/Tracer, RT_Metal) has no FFI; its de-facto boundary is
 * "flat buffers of POD structs shared by host and shader + one dispatch"
 * (RT_Metal/Metal/Render.metal:495-509 kernel arguments; host side
 * RT_Metal/Tracer/AAPLRenderer.mm:702-720,1167-1196).  This header restates
 * those PODs byte-for-byte (Apple simd rules: float3 = 16 B / align 16,
 * float2 = 8 / 8, float4x4 = 64 / 16 column-major, packed_float3 = 12 / 4)
 * and declares the entry points a host would call in place of
 * `-[AAPLRenderer render:]`.  Every struct cites the reference definition
 * it mirrors; sizes/offsets are locked by static asserts below.
 *
 * Two shared libraries implement it:
 *   libtracer_amd.so  (HIP, gfx950)  -- trc_*        device path (the product)
 *   libtrc_host.so    (C++17, CPU)   -- trc_host_*   scene prep + SAH BVH builder
 */
#ifndef TRACER_ABI_H
#define TRACER_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gcc / clang / hipcc, C and C++ alike */
#define TRC_ALIGN(n) __attribute__((aligned(n)))

/* 2: trc_trace_rays' last argument became a bit set (TRC_TRACE_*: 2 now means the production closest-hit walk, it used
 *    to mean any-hit); trc_build_flavor, trc_sppm_hash_cells, trc_host_scene_load_pbrt, trc_host_mesh_from_arrays added
 * 3: trc_group_set_collectives, trc_debug_set, trc_debug_block_costs; trc_pbrt_info / trc_pbrt_shape grew (textures,
 *    plymesh / disk / cylinder); trc_host_mesh_load_ply, trc_host_load_hdr, trc_div_by_test
 * 4: trc_debug_launch_shape, trc_unary_test; grouped trc_sppm_download of the photon records is collective; trc_stats.schedule_ms; knob no_plan_reuse; trc_debug_block_costs reports durations per SAMPLE (shader clocks / (4 spp)); knobs
 *    no_cold_probe / probe_spp (the first launch of a block list runs as an 8-sample head + the rest, trc_render)
 * 5: sample sharding with a bit-level definition: trc_shard_seed, trc_group_compose_samples[_async]; trc_collectives grew
 *    (alltoall, gather); trc_group_allreduce_mean_accum is that compose delivered to every rank (rank-ordered sum, no longer an
 *    all-reduce); trc_device_pci_bus_id; the test hooks moved to include/tracer_test_hooks.h and libtracer_amd_hooks.so
 * 6: launch lists may hold single-pixel parts (trc_debug_block_costs: bit 29; trc_launch_shape counts them as items); knob
 *    camera_policy; trc_download_composed on a non-root rank of a sample-sharded compose returns TRC_ERR_NO_FRAME (it used to
 *    hand out that rank's partial slices)
 * 7: SVGF denoiser stage: trc_gbuffer_texel, trc_denoise_params, trc_denoise_default_params, trc_denoise, trc_download_denoised,
 *    trc_tonemap_denoised, trc_download_gbuffer, trc_denoise_reset (nothing existing changed)
 * 8: image textures: trc_image, trc_upload_textures, trc_host_load_png (nothing existing changed)
 * 9: TRC_FLAG_ENV_LIGHT: the environment map as an importance-sampled light of traceMIS (nothing existing changed)
 * 10: per-triangle materials: trc_upload_triangle_materials, trc_host_scene_load_pbrt_flags (TRC_PBRT_TRIANGLE_MATERIALS),
 *    trc_host_scene_triangle_materials (nothing existing changed)
 * 11: primary replay: trc_debug_primary_replays, knob no_primary_replay; trc_stats.rays keeps counting every Scene::hit of the
 *    algorithm, the camera rays answered from the memo included (nothing existing changed)
 * 12: TRC_FLAG_MESH_LIGHTS: the emissive triangles of a mesh as sampled lights of traceMIS, knob mesh_light_pick (nothing existing
 *    changed)
 * 13: moving geometry: trc_update_vertices, trc_debug_refit_ms, knob refit_single (nothing existing changed)
 *     added under 13, the number stays: trc_pose, trc_pose_vertices, trc_download_vertices, trc_debug_pose_overflows (posing vertex
 *     ranges by matrices on the device; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_skin_influence, trc_skin_bone, TRC_SKIN_MAX_BONES, trc_skin_bind, trc_skin_vertices, knob
 *     skin_no_lds (linear blend skinning on the device; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_rebuild_tree, trc_tree_cost_t, trc_tree_cost (a fresh tree for a moved mesh from what the
 *     device holds, and a surface-area measure that tells a host when to ask for one; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_morph_delta, TRC_MORPH_MAX_TARGETS, trc_morph_bind, trc_morph_vertices (blend shapes on the
 *     device, alone or under the skin of trc_skin_bind in one call; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_recompute_normals (smooth vertex normals re-derived on the device from the mesh as it now
 *     stands; an addition only, nothing existing changed)
 *     added under 13, the number stays: trc_motion_texel, trc_denoise_track_motion, trc_download_motion, trc_download_history_length (the SVGF history follows
 *     surfaces that the calls above move; opt-in, off by default; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_primitive_ranges, trc_update_primitives, trc_host_make_sphere, trc_host_make_square,
 *     trc_host_make_cube (spheres, squares and cubes moved on the device; with tracking on the history follows them too: the motion
 *     texel of an analytic hit may now be non-zero; additions only, nothing existing changed)
 *     added under 13, the number stays: TRC_TREE_SAH3, trc_host_build_tree_flags (a three-axis, 32-bin SAH split as an option of the
 *     SAH builds on the host and on the device; opt-in, nothing defaults to it; additions only, nothing existing changed)
 *     added under 13, the number stays: trc_triangle_range, trc_set_triangle_visibility, trc_download_triangle_visibility,
 *     trc_debug_visibility_ms (mesh triangles shown and hidden on the device: a tree over the visible leaves from what the device holds;
 *     additions only, nothing existing changed)
 *     added under 13, the number stays: trc_set_tile_mask, trc_download_tile_mask, trc_tile_snapshot, trc_tile_error, trc_download_tile_error,
 *     trc_adaptive_params, trc_adaptive_report, trc_adaptive_default_params, trc_render_adaptive, trc_download_tile_samples, knob
 *     mask_forgets_costs (trc_render over a subset of the frame's tiles, a per-tile error estimate and a driver that stops sampling the
 *     tiles that have settled; with no mask set and no adaptive call made nothing changes; additions only)
 *     added under 13, the number stays: TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT is accepted (traceMIS: the map as a light under camera-ray
 *     sets; it returned TRC_ERR_UNSUPPORTED before) and trc_denoise_guide_rays (the SVGF G-buffer walked along the ray sets; opt-in, off by
 *     default); no unflagged launch and no unguided trc_denoise changes
 *     added under 13, the number stays: TRC_FLAG_MATERIAL_PARAMS, trc_material_params, trc_upload_material_params,
 *     trc_download_material_params, trc_host_default_material_params (per-material roughness, dielectric index and conductor eta / k read
 *     from a table of the context by kernels of their own; without the flag nothing changes; additions only) */
#define TRC_ABI_VERSION 13

/* ------------------------------------------------------------------ */
/* vector / matrix PODs (Apple simd layout)                            */
/* ------------------------------------------------------------------ */

/* simd_float2: 8 bytes, align 8 (RT_Metal/Metal/Common.hh:30) */
typedef struct TRC_ALIGN(8) trc_float2 { float x, y; } trc_float2;
/* simd_float3: 16 bytes, align 16; 4th lane is padding (Common.hh:29) */
typedef struct TRC_ALIGN(16) trc_float3 { float x, y, z, _pad; } trc_float3;
/* simd_float4 (Common.hh:28) */
typedef struct TRC_ALIGN(16) trc_float4 { float x, y, z, w; } trc_float4;
/* simd_float4x4: 4 columns, column-major (Common.hh:25) */
typedef struct TRC_ALIGN(16) trc_float4x4 { trc_float4 columns[4]; } trc_float4x4;

/* ------------------------------------------------------------------ */
/* enums, with the reference's ordinals                                */
/* ------------------------------------------------------------------ */

/* RT_Metal/Metal/BVH.hh:6-8 */
enum trc_PrimitiveType {
    TRC_PRIM_SPHERE = 0, TRC_PRIM_SQUARE = 1, TRC_PRIM_CUBE = 2,
    TRC_PRIM_TRIANGLE = 3, TRC_PRIM_BVH = 4, TRC_PRIM_UNKNOW = 5
};
/* RT_Metal/Metal/Material.hh:18-20 */
enum trc_MaterialType {
    TRC_MAT_DIFFUSE = 0, TRC_MAT_LAMBERT = 1, TRC_MAT_ORENNAYAR = 2,
    TRC_MAT_PLASTIC = 3, TRC_MAT_METAL = 4, TRC_MAT_GLASS = 5,
    TRC_MAT_ISOTROPIC = 6, TRC_MAT_DIELECTRIC = 7, TRC_MAT_DEMOFOX = 8,
    TRC_MAT_PBR = 9, TRC_MAT_NIL = 10
};
/* RT_Metal/Metal/Ray.hh:6 */
enum trc_MediumType { TRC_MEDIUM_NIL = 0, TRC_MEDIUM_HOMOGENEOUS = 1, TRC_MEDIUM_GRIDDENSITY = 2 };
/* RT_Metal/Metal/Texture.hh:6 */
enum trc_TextureType { TRC_TEX_CONSTANT = 0, TRC_TEX_CHECKER = 1, TRC_TEX_NOISE = 2, TRC_TEX_IMAGE = 3 };

/* ------------------------------------------------------------------ */
/* scene PODs                                                          */
/* ------------------------------------------------------------------ */

/* RT_Metal/Metal/AABB.hh:7-9 -- 32 bytes; empty box = (+FLT_MAX, -FLT_MAX) */
typedef struct trc_AABB { trc_float3 mini, maxi; } trc_AABB;

/* RT_Metal/Metal/BVH.hh:15-22 -- 64 bytes. Array form: root at index 0,
 * leaves carry pType in {Sphere,Square,Cube,Triangle} + pIndex, interior
 * nodes pType == BVH with left/right/parent indices into the same array. */
typedef struct trc_BVH {
    uint32_t parent, left, right;
    uint32_t axis;
    int32_t  pType;              /* enum trc_PrimitiveType */
    uint32_t pIndex;
    uint32_t _pad[2];
    trc_AABB bBOX;
} trc_BVH;

/* RT_Metal/Metal/Sphere.hh:6-15 -- 272 bytes */
typedef struct trc_Sphere {
    float        radius;
    uint32_t     _pad0[3];
    trc_float3   center;
    trc_float4x4 model_matrix, normal_matrix, inverse_matrix;
    uint32_t     material;
    uint32_t     _pad1[3];
    trc_AABB     boundingBOX;
} trc_Sphere;

/* RT_Metal/Metal/Square.hh:12-27 -- 272 bytes; axis-aligned rectangle
 * spanning range_i x range_j on axes (axis_i, axis_j) at axis_k = value_k */
typedef struct trc_Square {
    uint8_t      axis_i, axis_j;
    uint8_t      _pad0[6];
    trc_float2   range_i, range_j;
    uint8_t      axis_k;
    uint8_t      _pad1[3];
    float        value_k;
    trc_float4x4 model_matrix, normal_matrix, inverse_matrix;
    uint32_t     material;
    uint32_t     _pad2[3];
    trc_AABB     boundingBOX;
} trc_Square;

/* RT_Metal/Metal/Cube.hh:6-13 -- 240 bytes; unit box under model_matrix */
typedef struct trc_Cube {
    trc_float4x4 model_matrix, normal_matrix, inverse_matrix;
    trc_AABB     box;
    uint32_t     material;
    uint32_t     _pad[3];
} trc_Cube;

/* RT_Metal/Metal/Triangle.hh:12-18 (device) == Common.hh:32-36 MeshElement
 * (host) -- 32 bytes, packed */
typedef struct trc_TriangleVertex {
    float v[3];
    float n[3];
    float uv[2];
} trc_TriangleVertex;

/* RT_Metal/Metal/Texture.hh:8-13 -- 32 bytes */
typedef struct trc_TextureInfo {
    int32_t    type;             /* enum trc_TextureType */
    uint32_t   textureIndex;
    uint32_t   _pad[2];
    trc_float3 albedo;
} trc_TextureInfo;

/* RT_Metal/Metal/Material.hh:22-40 -- 64 bytes. NOTE (reference behaviour):
 * BSDF parameters are hard-coded in MicrofacetBXDF.h create*() functions;
 * eta / roughness are carried but not read by the shading path. */
typedef struct trc_Material {
    int32_t  type;               /* enum trc_MaterialType */
    int32_t  medium;             /* enum trc_MediumType */
    uint8_t  specular;
    uint8_t  _pad0[3];
    float    eta;
    float    roughness;
    uint32_t _pad1[3];
    trc_TextureInfo textureInfo;
} trc_Material;

/* RT_Metal/Metal/Camera.hh:8-21 -- 176 bytes */
typedef struct trc_Camera {
    trc_float3 lookFrom, lookAt, viewUp;
    float vfov, aspect, aperture, lenRadius;
    float focus_dist;
    uint32_t _pad[3];
    trc_float3 u, v, w;
    trc_float3 vertical, horizontal, cornerLowLeft;
} trc_Camera;

/* RT_Metal/Metal/Camera.hh:27-55 -- 96 bytes (per-frame uniforms) */
typedef struct trc_Complex {
    trc_float2 tex_size, view_size;
    float      running_time;
    uint32_t   frame_count;
    uint32_t   _pad0[2];
    trc_AABB   photonBox;
    trc_float3 photonBoxSize;
    float      photonInitialRadius;
    float      photonHashScale;
    float      totalPhotonSum;
    uint32_t   framePhotonSum;
} trc_Complex;

/* RT_Metal/Metal/Photon.hh:12-28 -- 80 bytes (SPPM photon, persists across frames up to 8 steps) */
typedef struct trc_PhotonRecord {
    trc_float3 flux, normal, position, direction;
    uint8_t    step;
    uint8_t    active;
    uint8_t    _pad[14];
} trc_PhotonRecord;

/* RT_Metal/Metal/Photon.hh:30-53 -- 112 bytes (SPPM visible point of one pixel) */
typedef struct trc_CameraRecord {
    trc_float3 ratio, position, direction;
    uint8_t    valid;
    uint8_t    _pad0[15];
    trc_float3 alternative, flux;
    float      radius;
    uint32_t   photonCount;
    uint32_t   _pad1[2];
} trc_CameraRecord;

/* RT_Metal/Metal/Medium.hh:83-109 -- 32 bytes; describes the density grid of the GridDensity medium
 * (bound at PackageEnv ids 3/4, Render.hh:30-31) */
typedef struct trc_GridDensityInfo {
    float    sigma_a, sigma_s;
    float    sigma_t, g;
    float    invMaxDensity;
    uint32_t nx, ny, nz;
} trc_GridDensityInfo;

#define TRC_PHOTON_HASHN 512      /* PHOTON_HASHN, RT_Metal/Metal/Common.hh:4: 512x512 photons and hash cells */

/* Primitive argument table of the kernel (Render.hh:122-130) + materials of
 * PackageEnv (Render.hh:24-32), as pointers + counts.  All pointers are HOST
 * pointers; trc_upload_scene copies, the caller keeps ownership. */
typedef struct trc_scene {
    const trc_BVH*            bvhList;     uint32_t n_bvh;        /* 2*leaves-1, root at 0 */
    const trc_Sphere*         sphereList;  uint32_t n_sphere;
    const trc_Square*         squareList;  uint32_t n_square;
    const trc_Cube*           cubeList;    uint32_t n_cube;
    const trc_TriangleVertex* triList;     uint32_t n_vertex;
    const uint32_t*           idxList;     uint32_t n_index;      /* 3 per triangle */
    const trc_Material*       materials;   uint32_t n_material;
} trc_scene;

/* ------------------------------------------------------------------ */
/* status codes                                                        */
/* ------------------------------------------------------------------ */
typedef int32_t trc_status;
#define TRC_OK                  0
#define TRC_ERR_INVALID_ARG    -1
#define TRC_ERR_NO_DEVICE      -2   /* no HIP device / extension unusable: fail loudly */
#define TRC_ERR_HIP            -3
#define TRC_ERR_NO_SCENE       -4
#define TRC_ERR_NO_FRAME       -5   /* trc_resize not called */
#define TRC_ERR_BVH_INVALID    -6   /* malformed tree (bad index, depth > TRC_MAX_BVH_DEPTH, ...) */
#define TRC_ERR_UNSUPPORTED    -7
#define TRC_ERR_RCCL           -8
#define TRC_ERR_OOM            -9

#define TRC_MAX_BVH_DEPTH      64   /* reference: 32-bit stack_mark (Render.hh:140) */

/* ------------------------------------------------------------------ */
/* render parameters                                                   */
/* ------------------------------------------------------------------ */
enum trc_integrator {
    TRC_INTEGRATOR_PATH = 0,     /* tracePath, Render.metal:411-492 (the active one, :532) */
    TRC_INTEGRATOR_MIS  = 1,     /* traceMIS,  Render.metal:277-409 */
    TRC_INTEGRATOR_VOLUME = 2    /* traceVolume, Render.metal:78-275: traceMIS + participating media
                                    (Medium.hh:25-199, HitRecord.hh:37-79); SURVEY 8f-3 */
};

/* flags */
#define TRC_FLAG_FIXED_ORDER    2u  /* launch the pixel blocks in list order instead of "most expensive block of the
                                       previous launch first" (a scheduling choice only: pixels are independent) */
#define TRC_FLAG_SOBOL          4u  /* XSampler = pbrt::SobolSampler, wired as the reference's commented-out lines do
                                       (Render.metal:529-530): castRay still draws from the pixel's PCG stream; the
                                       sampler is built afterwards from a COPY of that stream, the frame number and
                                       the pixel; sample2D() (the BSDF sample of every bounce) takes successive Sobol
                                       dimensions of the pixel's sample, random() (light pick, Russian roulette)
                                       draws from the copy, and the texel keeps the stream as castRay left it.
                                       TRC_INTEGRATOR_PATH / _MIS only, 2 * max_depth <= 40 dimensions; with
                                       view_height the sampler sees the pixel and size of its own view.  Not with an
                                       active image texture (trc_upload_textures): TRC_ERR_UNSUPPORTED. */
#define TRC_FLAG_SMALL_BLOCKS    8u  /* one 4x4 pixel block on 16 lanes per wavefront instead of 8x8 on 64 (a scheduling
                                       choice only: pixels are independent).  Pays when a launch has about as many
                                       blocks as the GPU has wavefront slots, i.e. a rank's share of a strong-scaled
                                       frame; chosen automatically there unless TRC_FLAG_LARGE_BLOCKS is set */
#define TRC_FLAG_LARGE_BLOCKS   16u
#define TRC_FLAG_ENV_LIGHT      32u /* traceMIS treats the environment map as a light, sampled by importance and combined with
                                       BSDF sampling by MIS (an extension beyond the reference, which lights with the map only
                                       where a BSDF-sampled ray escapes).  Without the flag nothing changes.
   - Accepted with TRC_INTEGRATOR_MIS and a map set (trc_set_environment_map; the constant of trc_set_environment is not
     sampled), with or without active image textures.  With tracePath / traceVolume, TRC_FLAG_SOBOL, TRC_FLAG_COLLECT_STATS or
     without a map, trc_render returns TRC_ERR_UNSUPPORTED and renders nothing.  Scenes without squareList[5] / [6] are accepted.
   - Distribution over the map's W x H cells (row j at w in [j/H, (j+1)/H), rows bottom-up like the map's): cell weight = the
     largest rgb_to_y among the texels the bilinear lookup can read inside the cell (3 x 3, clamped at the edges; negative or
     non-finite texels count 0) times cos(latitude of the cell centre).  Direction of (u, w): phi = 2 pi (u - 1/2),
     latitude = pi (w - 1/2), d = (cos lat cos phi, sin lat, cos lat sin phi); solid-angle pdf = p_uw / (2 pi^2 cos lat).
     The radiance lookup keeps the reference's SampleSphericalMap constants (0.1591 / 0.3183).
   - Light pick: the reference's one pcg_float draw.  p_env = 1/2 with square lights, 1 without, 0 when every weight is 0.  A
     draw below p_env picks the map, else square 5 below p_env + (1 - p_env) / 2 and square 6 above; a square's contribution
     is divided by 1 - p_env (the reference's expectation, its missing 1/2 pick factor included).
   - The map's sample: a two-level alias table (rows, then the picked row's cells), six extra PCG draws taken only when the
     map is picked: a multiply-shift index and a 32-bit alias decision per level, two floats inside the cell.  Its shadow ray
     is an any-hit walk to infinity from where a BSDF ray of that direction would start.  Contribution: ratio * F * L_env *
     w / (p_env pdf), w = power heuristic(p_env pdf, bsdf pdf).  The map's sample counts only where the BSDF sample is a
     cosine lobe (Lambert, or the Lambert lobe of Plastic, picked by the vertex's sample2D) and has support (wo.z > 0,
     wi.z > 0).  Beckmann, Metal and Glass lobes report per-lobe pdfs with the reference's lobe-pick conventions
     (Material.hh), not the density to weigh against: at such a vertex a pick of the map takes no sample and the escape keeps
     weight 1, so the flag reduces no variance there.  No map sample at a vertex whose BSDF ray would not be counted if it
     escaped (max_depth), so the flag changes no expectation at any max_depth.
   - A BSDF-sampled ray from a cosine lobe that escapes is weighted by power heuristic(bsdf pdf, p_env pdf(d)), exactly 1
     where pdf(d) = 0; any other escape (a camera ray, a ray from another material) is not weighted.  Without square lights a BSDF-sampled emitter hit has weight 1.
   - The tables are built at the first flagged render after trc_set_environment_map (TRC_ERR_OOM if they cannot be
     allocated; flag-off renders keep working) and freed when the map changes or is cleared, and by trc_destroy.  A change
     of the flag, like one of the integrator, drops the recorded block costs of the launch planner. */
#define TRC_FLAG_MESH_LIGHTS    64u /* traceMIS treats the emissive triangles of the mesh as lights, sampled by area and combined
                                       with BSDF sampling by MIS (an extension beyond the reference, whose traceMIS samples
                                       squareList[5] / [6] only).  Without the flag nothing changes.
   - Accepted with TRC_INTEGRATOR_MIS, with or without active image textures, with or without trc_upload_triangle_materials
     (without it every triangle has material 19), with or without squareList[5] / [6].  With tracePath / traceVolume,
     TRC_FLAG_SOBOL, TRC_FLAG_COLLECT_STATS or TRC_FLAG_ENV_LIGHT, trc_render returns TRC_ERR_UNSUPPORTED and renders nothing.
   - Light set: triangle t is a light when its material has type TRC_MAT_DIFFUSE (the emitter), y = rgb_to_y(albedo) is finite
     and > 0, and its area A is finite and > 0; binary32 on the vertices as uploaded, in this order: e1 = v1 - v0, e2 = v2 - v0,
     c = cross(e1, e2), A = sqrt(c.x c.x + c.y c.y + c.z c.z) / 2.  Its weight is y * A (the exact float64 product); the total is
     the float64 sum over the lights by ascending triangle index.  A one-level alias table over the lights in triangle order
     (entries {threshold, alias}: a 32-bit draw below the threshold keeps the entry; Vose's method in the order stated for
     TRC_FLAG_ENV_LIGHT's tables) and, per triangle, pdfA[t] = weight / (total * A) rounded once to binary32, 0 for a triangle
     that is no light.
   - Light pick: the reference's one pcg_float draw.  p_mesh = 1/2 with square lights, 1 without, 0 without a light triangle.
     A draw below p_mesh picks the mesh, else square 5 below p_mesh + (1 - p_mesh) / 2 and square 6 above; a square's
     contribution is divided by 1 - p_mesh.  With p_mesh = 0 every operation and draw is the flag-off kernel's: the frame and
     the RNG texture are the flag-off ones bit for bit.
   - The mesh's sample: four extra PCG draws, taken only when the mesh is picked: r0, r1 pick the light (multiply-shift index,
     alias decision), floats f0, f1 the point: s = sqrt(f0), b0 = 1 - s, b1 = f1 s, p = (v0 b0 + v1 b1) + v2 ((1 - b0) - b1).
     n = the normalised geometric normal cross(e1, e2) on the shading point's side; the shadow ray is the any-hit walk to
     offset_ray(p, n), as for a square.  cosL = |dot(n, -dir)|, liPDF = p_mesh pdfA dist^2 / cosL, contribution = ratio * F *
     (albedo cosL) * w / liPDF with w = power heuristic(liPDF, bsdf pdf): radiance keeps the reference's Le * cos convention,
     so squares and triangles emit alike.  As for TRC_FLAG_ENV_LIGHT the sample counts only where the BSDF sample is a cosine
     lobe (Lambert, or the Lambert lobe of Plastic) with wo.z > 0 and wi.z > 0; at any other vertex a pick of the mesh takes no
     sample and draws nothing more.
   - A BSDF-sampled hit on a TRIANGLE emitter, while the scene has a light triangle, is ratio * (albedo cosOnLight) * w with
     cosOnLight = |dot(geometric normal, -d)| and w = power heuristic(bsdf pdf, p_mesh pdfA[t] dist^2 / cosOnLight) where the
     previous vertex sampled a cosine lobe and that density is > 0, else 1.  This is a DEFINED DIFFERENCE from flag-off for
     triangle emitters: the reference's formula multiplies the emitter hit by scat_attenuation / scat_bxPDF a second time (the
     path throughput holds it already) and weighs it against hitRecord.PDF, which only a square writes -- on a triangle it is
     whatever the last accepted square left there; neither describes the integrand the mesh's light sample estimates.  A
     square emitter hit keeps the reference's formula, and camera-ray hits on emitters are unchanged.
   - Knob mesh_light_pick (trc_debug_set; default 1): 0 forces p_mesh = 0 while the triangle-emitter formula above is kept
     (w = 1): the BSDF-only estimator of the same integrand.  Measurement and tests only.
   - The tables are built on the device at the first flagged render after a scene or triangle-material upload (TRC_ERR_OOM
     if they cannot be allocated; flag-off renders keep working) and freed by every trc_upload_scene*, by
     trc_upload_triangle_materials and by trc_destroy.  A change of the flag drops the recorded block costs of the launch
     planner. */
#define TRC_FLAG_CAMERA_RAYS   128u /* a sample's camera ray is read from the context's camera-ray sets ("Camera-ray sets" below:
                                       trc_upload_camera_rays, trc_generate_camera_rays) instead of being cast by the camera: the way
                                       to anti-aliasing (sets of sub-pixel offsets) and to other projections (orthographic, 360 degree
                                       panorama, a host's own lens).  Without the flag nothing changes.
   - Which ray: with n_sets sets in force, sample s of a call with frame0 takes, for pixel (x, y), the record of set
     (frame0 + s) % n_sets at (set * H + y) * W + x.  The ray is made as trc_trace_rays makes one: the direction is normalised on
     entry like Ray::Ray; tmax and _pad are ignored.  Rays are not validated: a non-finite ray misses the scene, as the walk has it.
   - Everything else of the sample is the unflagged trc_render's: the pixel's RNG texel is read and written the same way; the stream
     is advanced by castRay's lens draws (the rejection loop of Camera.hh:59-69) exactly as before -- the draws are taken and their
     ray dropped --, then the same tracePath / traceMIS step by step, the running mean weighted by frame0 + s, the NaN / Inf clamp
     and the work counters.
   - So, with the rays the camera itself would cast (a camera of lens radius 0 and no zero component in lookFrom; TRC_RAYS_PINHOLE,
     one set, no offsets), the frame, the RNG texture and trc_stats.rays / paths / shaded are the unflagged call's, bit for bit.
   - And k calls of 1 sample equal one call of k samples, so launches of few samples are coalesced as without the flag (the flag
     is part of what "continues" a kept launch).
   - Accepted with TRC_INTEGRATOR_PATH and TRC_INTEGRATOR_MIS, with or without active image textures, with or without
     trc_upload_triangle_materials, on trees staged in LDS or read from memory, with tile_rank / tile_nranks, under a tile mask and in
     trc_render_adaptive.  TRC_ERR_UNSUPPORTED, nothing rendered: no rays in force; TRC_INTEGRATOR_VOLUME; TRC_FLAG_SOBOL,
     TRC_FLAG_COLLECT_STATS or TRC_FLAG_MESH_LIGHTS; a view_height that names a stack (non-zero and below H).
   - With TRC_FLAG_ENV_LIGHT besides (TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT, traceMIS): the sample takes its camera ray from the
     sets exactly as above (the lens draws are taken and dropped), and everything after that is the TRC_FLAG_ENV_LIGHT sample step by
     step: the light pick, the six extra draws when the map is picked, the any-hit shadow walk, the MIS weights, the weighting of
     escapes from cosine lobes.  So with the rays the camera itself would cast (as above) the frame, the RNG texture and
     trc_stats.rays / paths / shaded are the unflagged TRC_FLAG_ENV_LIGHT call's, bit for bit; and k calls of 1 sample equal one call of
     k samples.  Accepted with TRC_INTEGRATOR_MIS and a map set, with or without active image textures, trc_upload_triangle_materials
     and square lights, on trees staged in LDS or read from memory, with tile ranks, under a tile mask and in trc_render_adaptive.
     The refusals are the union of the two flags' own (TRC_ERR_UNSUPPORTED, nothing rendered): no rays in force, no map, another
     integrator, TRC_FLAG_SOBOL, TRC_FLAG_COLLECT_STATS, TRC_FLAG_MESH_LIGHTS, a stacked view.  The natural pair of
     TRC_RAYS_EQUIRECT: a panorama of a scene lit by the map, in the map's own parametrisation.
   - A flagged launch runs kernels of its own, one pixel block per one-wavefront workgroup: no strips, persistent workgroups or
     dense kernel, and no primary replay.  A change of the flag, or new rays in force, drops the recorded block costs of the
     launch planner, as a change of the integrator does (and so does a change of TRC_FLAG_ENV_LIGHT under the flag).
   - trc_denoise follows the rays where trc_denoise_guide_rays is on ("A denoiser that follows the rays" below); with it off its
     G-buffer is the camera's: right for TRC_RAYS_PINHOLE sets, up to the sub-pixel offset, and wrong for any other rays.
   - LIMIT: the SPPM camera pass knows nothing of the rays; TRC_FLAG_MESH_LIGHTS is refused under the flag. */
#define TRC_FLAG_MATERIAL_PARAMS 256u /* the lobe parameters the reference writes as literals -- the roughness pair, the dielectric
                                       index, the conductor's eta and k -- are read per material from the context's table ("Material
                                       parameters" below: trc_upload_material_params).  Without the flag nothing changes: frames, RNG
                                       texture, stats, timing and memory are the unflagged library's.
   - A flagged sample is the unflagged sample step by step with those literals replaced by entry rec.material of the table: the same
     draws in the same order, the reference's expressions on the same operands in the same order.  Replaced: the roughness pair of the
     material's microfacet distribution (Plastic's specular lobe and both Glass lobes: Beckmann; Metal: Trowbridge-Reitz), each used
     as max(0.001f, a); the 1.5 of Plastic's and Glass's reflection Fresnel term and Glass's etaB (etaA stays 1, and the transmission
     lobe's own Fresnel term stays FresnelDielectric(etaA)); Metal's eta and k.  Kept as literals: Plastic's kd / ks weights, Glass's
     kr / kt = 0.98, the lobe-pick ratios.  A Lambert vertex, an emitter and the diffuse half of Plastic read nothing of the table.
   - Where the unflagged kernels use a form that holds for the literals only, the flagged kernels use the general form, correctly
     rounded: a quotient by alpha * alpha is the division x / (alpha * alpha); the conductor Fresnel term is the general one; the
     index is the table's.  So with a table of trc_host_default_material_params per material the frame, the RNG texture and
     trc_stats.rays / paths / shaded are the unflagged call's, bit for bit (exact build).
   - And k calls of 1 sample equal one call of k samples, so launches of few samples are coalesced as without the flag (the flag
     is part of what "continues" a kept launch).
   - Accepted with TRC_INTEGRATOR_PATH and TRC_INTEGRATOR_MIS, with or without active image textures, with or without
     trc_upload_triangle_materials, on trees staged in LDS or read from memory, with tile_rank / tile_nranks, under a tile mask and in
     trc_render_adaptive.  TRC_ERR_UNSUPPORTED, nothing rendered: no table in force; TRC_INTEGRATOR_VOLUME; TRC_FLAG_SOBOL,
     TRC_FLAG_COLLECT_STATS, TRC_FLAG_ENV_LIGHT, TRC_FLAG_MESH_LIGHTS or TRC_FLAG_CAMERA_RAYS; a view_height that names a stack
     (non-zero and below H).
   - A flagged launch runs kernels of its own, one pixel block per one-wavefront workgroup: no strips, persistent workgroups or
     dense kernel, and no primary replay.  A change of the flag, or a new table, drops the recorded block costs of the launch planner.
   - LIMIT: SPPM and trc_denoise do not know the table; the pbrt reader does not fill one. */
#define TRC_FLAG_COLLECT_STATS  1u  /* run the instrumented kernel variant: exact
                                       N_descend / N_return / leaf-test counters.  Not with an active image texture
                                       (trc_upload_textures): TRC_ERR_UNSUPPORTED. */

typedef struct trc_params {
    uint32_t spp;                /* samples per pixel this call; the reference does 1 per launch */
    uint32_t max_depth;          /* 8 (Render.metal:532) */
    uint32_t integrator;         /* enum trc_integrator */
    uint32_t frame0;             /* Complex.frame_count of the first sample (running-mean weight) */
    uint32_t tile_rank;          /* this call renders tiles t with trc_tile_owner(t) == tile_rank ... */
    uint32_t tile_nranks;        /* ... of tile_nranks (1 => whole frame) */
    uint32_t flags;
    uint32_t view_height;        /* 0: the frame is one view.  Otherwise the frame is a vertical stack of views of
                                    this many rows: pixel (x, y) sees the camera ray of (x, y % view_height) of a
                                    W x view_height image -- a batch of views rendered as one frame (each pixel of
                                    the stack has its own RNG texel); bench.py's multi-GPU workload */
} trc_params;

/* Pixel tiles: TRC_TILE x TRC_TILE pixels, row-major tile grid, owner of
 * tile (tx,ty) among n ranks = (tx + ty) % n. */
#define TRC_TILE 16

/* One ray / one hit of the Scene::hit test hook (Render.hh:135-252). */
typedef struct trc_ray {
    float origin[3];
    float tmax;                  /* test_t: FLT_MAX for closest hit, distance for shadow rays */
    float direction[3];          /* normalised on entry like Ray::Ray (Ray.hh:21-23) */
    uint32_t _pad;
} trc_ray;

typedef struct trc_hit {
    int32_t  hit;                /* return value of Scene::hit */
    int32_t  pType;              /* primitive type of the closest hit, -1 on miss */
    uint32_t pIndex;             /* index into its primitive list */
    float    t;
    float    p[3];
    float    gn[3];
    float    sn[3];
    float    uv[2];
    uint32_t material;
    float    PDF;
    uint32_t n_descend;          /* traversal iterations entered from the parent (Render.hh:155-187) */
    uint32_t n_return;           /* iterations entered from a child (Render.hh:189-209) */
    uint32_t n_leaf;             /* primitive hit_test calls */
} trc_hit;

/* Exact work counters of the render kernels since the last trc_reset_stats.
 * rays / paths are always counted; the n_* traversal counters only when
 * TRC_FLAG_COLLECT_STATS was set for the call. */
typedef struct trc_stats {
    uint64_t paths;              /* W*H*spp of the tiles rendered */
    uint64_t rays;               /* Scene::hit invocations of the reference's algorithm (primary + bounce + shadow).  The tracePath
                                  * production kernels answer a pixel's repeated camera ray from a memo of its first walk instead of
                                  * walking again (trc_debug_primary_replays counts those); such a ray is counted here all the same */
    uint64_t shaded;             /* material lookups (S_F / F evaluations' hits) */
    uint64_t n_descend, n_return;
    uint64_t n_leaf_sphere, n_leaf_square, n_leaf_cube, n_leaf_triangle;
    uint64_t n_hit_triangle;     /* triangle tests that hit (+60 B normal/uv fetch) */
    uint64_t n_hit_cube;         /* cube tests that reach the world transform (228 B vs 100 B) */
    uint64_t launches;           /* render kernel launches */
    double   kernel_ms;          /* sum of hipEvent durations of those launches, on the ctx stream */
    double   schedule_ms;        /* ... and of the launch-list kernels in front of them (order, sort, split plan); not part of kernel_ms */
} trc_stats;

/* Threading contract.  A context owns its device buffers, one render stream (+ a communication stream and the SPPM
 * camera stream) and all per-launch state; nothing is shared between contexts except the process-wide RCCL symbol table,
 * which is resolved once under a lock.  Therefore:
 *   - calls on ONE context must not overlap: a context is used by one thread at a time (any thread -- the reference's
 *     completion handlers arrive off the main thread, AAPLRenderer.mm:1148-1150 -- every entry point selects the
 *     context's device itself);
 *   - DIFFERENT contexts, on the same GPU or on different GPUs, may be driven from different threads concurrently;
 *   - trc_* calls are asynchronous on the context's stream unless they hand host memory back (downloads, trc_get_stats,
 *     trc_trace_rays, trc_tonemap, trc_synchronize), which wait for the stream.
 * tests/test_gpu_multicontext.py drives two contexts interleaved and from two threads. */
typedef struct trc_ctx trc_ctx;

/* ------------------------------------------------------------------ */
/* device path: libtracer_amd.so                                       */
/* ------------------------------------------------------------------ */

uint32_t    trc_abi_version(void);
/* "exact" = libtracer_amd.so: IEEE division / sqrt, no FMA contraction -- the build every parity statement is about;
 * "fast-math" = libtracer_amd_fast.so: the same sources under fast-math rules, as the reference compiles its shaders
 * (MTL_FAST_MATH): approximate division / sqrt, FMA contraction, denormals flushed; results agree with the exact build
 * statistically, not bit for bit */
const char* trc_build_flavor(void);
/* 1 in libtracer_amd_hooks.so -- the same sources compiled with -DTRC_TEST_HOOKS, which additionally exports the
 * entry points of include/tracer_test_hooks.h (exhaustive arithmetic checks, the SPPM hash, the per-site cycle profile) for
 * tests/ and tools/; 0 in the product libraries, which do not carry them */
int         trc_has_test_hooks(void);
const char* trc_status_string(trc_status s);
/* last error text of this context (HIP error string etc.), never NULL */
const char* trc_last_error(const trc_ctx* ctx);

/* replaces device/queue/pipeline creation, AAPLRenderer.mm:129-181 */
trc_status trc_create(int device, trc_ctx** out);
void       trc_destroy(trc_ctx* ctx);

/* replaces buffer creation + heap copy, AAPLRenderer.mm:213-246,610-720,1233-1355 */
trc_status trc_upload_scene(trc_ctx* ctx, const trc_scene* scene);

/* On-device LBVH build + node repack.  The reference builds its BVH on the host
 * (BVH::buildTree, RT_Metal/Metal/BVH.hh:35-269) and lists "LBVHs, Morton Encoding" as a to-do
 * (RT_Metal/README.md:42); this entry point replaces BVH::buildTree for scenes where the host SAH build is the
 * bottleneck.  `scene->bvhList` holds ONLY the n_bvh LEAF records as BVH::buildNode writes them
 * (BVH.hh:273-314: bBOX, pType, pIndex); the hierarchy is built on the GPU (30-bit Morton codes of the box
 * centroids, stable radix sort, Karras' binary radix tree, bottom-up boxes) and used by every later
 * trc_render / trc_trace_rays exactly like an uploaded tree. */
trc_status trc_upload_scene_lbvh(trc_ctx* ctx, const trc_scene* scene);
/* BVH::buildTree itself on the device (RT_Metal/Metal/BVH.hh:35-269; the host builder of this package is
 * trc_host_build_tree): same input as trc_upload_scene_lbvh -- the n_bvh LEAF records -- and the tree the reference's
 * 10-bucket SAH recursion builds from them, record for record (post-order interior numbering, the partition's own leaf
 * order, median split of identical centroids, pairs ordered by centroid): rendering through it is rendering through the
 * host-built tree.  Leaf boxes must be finite with |coordinates| <= 1e37 (TRC_ERR_BVH_INVALID otherwise).
 * trc_download_bvh / trc_lbvh_info report on it like on an LBVH tree. */
trc_status trc_upload_scene_sah(trc_ctx* ctx, const trc_scene* scene);
/* Both device builds behind one call.  flags: TRC_TREE_SAH (else the LBVH); TRC_TREE_TRIANGLE_LEAVES: `scene->bvhList` holds the leaf
 * records of the analytic primitives only (n_bvh of them, possibly none) and one leaf per triangle of (idxList, triList) follows them
 * in index order, written on the device exactly as the reference's loop writes it (AAPLRenderer.mm:575-589: the box of the three
 * vertices through BVH::buildNode under the identity matrix) -- a host with a mesh of a million triangles neither loops over them
 * nor uploads 64 bytes per triangle.  The tree is the one trc_host_build_tree builds from the same leaves. */
#define TRC_TREE_SAH              1u
#define TRC_TREE_TRIANGLE_LEAVES  2u
/* TRC_TREE_SAH3, a modifier of TRC_TREE_SAH: a tree of lower surface-area cost from the same leaves -- every axis is priced, with 32
 * bins, in place of the reference's widest axis and 10 buckets.  An option: nothing defaults to it, and the tree is no longer the
 * reference's.  Accepted: trc_upload_scene_device(TRC_TREE_SAH | TRC_TREE_SAH3 [| TRC_TREE_TRIANGLE_LEAVES]),
 * trc_rebuild_tree(TRC_TREE_SAH | TRC_TREE_SAH3) and trc_host_build_tree_flags(TRC_TREE_SAH | TRC_TREE_SAH3): the three build the same
 * tree from the same leaves, record for record.  TRC_TREE_SAH3 without TRC_TREE_SAH is TRC_ERR_INVALID_ARG, nothing changed.
 *  - As for TRC_TREE_SAH: the root at 0, the leaves at 1..n in input order, the interiors in serial post-order; a record's centroid is
 *    mn + (mx - mn) / 2 per component; a node of two leaves puts the one with the smaller centroid on the widest axis of the two
 *    centroids' box to the left (the first to the right unless it compares <); every box is the union of its children's; leaf boxes
 *    must be finite with |coordinates| <= 1e37; the depth limit is TRC_MAX_BVH_DEPTH.  Only the split of a node of three or more
 *    leaves differs:
 *  - cb = the bounds of the node's records' centroids.  The axes a = 0, 1, 2 are considered in that order; an axis is skipped unless
 *    e = cb.max[a] - cb.min[a] compares > 0.  The bin of a record on a considered axis: rel = (c[a] - cb.min[a]) / e, fb = 32 * rel,
 *    b = fb >= 0 ? (uint)fb : 0, clamped to 31.
 *  - For each considered axis and each i = 0..30 ascending: side 0 holds the records with bin <= i, side 1 the rest; n0, n1 their
 *    counts, B0, B1 the unions of their leaf boxes; A(B) = 2 * ((dx * dy + dx * dz) + dy * dz) with d = max - min;
 *    cost = (float)n0 * A(B0) + (float)n1 * A(B1).  Every operation is one binary32 operation in the order written, none contracted.
 *    A candidate with an empty side is skipped (on an axis of positive extent bins 0 and 31 are never empty, so none is).
 *  - The first candidate in this order initialises best; a later one replaces it only when cost < best: ties go to the lower axis,
 *    then to the lower i, and an infinite or NaN cost behaves as < says.  There is no division by the area of cb, which is 0 for
 *    collinear or coplanar centroids.
 *  - The records whose bin on the winning axis is <= the winning i go left, in the order the two-ended swap loop of BVH.hh:154-168
 *    leaves them (the k-th misplaced record from the left changes places with the k-th from the right).  The node's axis is the
 *    winning axis.
 *  - No axis of positive extent: all centroids are identical.  axis 2, the split at first + span / 2, the order kept. */
#define TRC_TREE_SAH3             16u
trc_status trc_upload_scene_device(trc_ctx* ctx, const trc_scene* scene, uint32_t flags);
/* the device-built tree in the reference's array layout (BVH.hh:246-269): [root, leaf 0..n-1, interior
 * 1..n-2], 2n-1 records.  out == NULL: only *n_nodes is written. */
trc_status trc_download_bvh(trc_ctx* ctx, trc_BVH* out, uint32_t capacity, uint32_t* n_nodes);
/* node count, depth of the deepest leaf and GPU time of the last trc_upload_scene_lbvh (bounds -> emit) */
trc_status trc_lbvh_info(trc_ctx* ctx, uint32_t* n_nodes, uint32_t* height, float* device_build_ms);
/* replaces memcpy(_camera_buffer.contents, ...), AAPLRenderer.mm:1183 */
/* replaces _densityInfoBuffer / _densityDataBuffer (AAPLRenderer.mm:629-643, bound at :716-720): the
 * nx*ny*nz density grid of the GridDensity medium, x fastest (Medium.hh:121).  Consulted by
 * TRC_INTEGRATOR_VOLUME when a ray travels in a medium of type TRC_MEDIUM_GRIDDENSITY; both pointers
 * NULL clear it. */
trc_status trc_upload_density(trc_ctx* ctx, const trc_GridDensityInfo* info, const float* density);
trc_status trc_set_camera(trc_ctx* ctx, const trc_Camera* camera);
/* constant environment radiance used on a miss; stands in for
 * packageEnv.texHDR.sample (Render.metal:434-439; the HDR blob is missing) */
trc_status trc_set_environment(trc_ctx* ctx, const float rgb[3]);

/* (re)allocates accum A (RGBA32F) + RNG (RGBA32Uint) for a W x H frame and
 * zeroes them; replaces texture creation, AAPLRenderer.mm:260-288 */
/* texHDR (Render.hh:25; the reference's HDR blob is missing from its repository): equirectangular RGB float image,
 * 3*w*h floats, row 0 at v = 0.  A ray that leaves the scene returns SampleSphericalMap (Render.hh:42-48) + a bilinear,
 * clamp-to-edge lookup (Common.hh:11) instead of the constant of trc_set_environment; rgb == NULL clears the map. */
trc_status trc_set_environment_map(trc_ctx* ctx, uint32_t w, uint32_t h, const float* rgb);

/* Image textures (TextureInfo::value, Texture.hh:29-35, over texture2d's of PackageEnv, Render.hh:26; the reference's host
 * loads them with MTKTextureLoader, sRGB off, origin flipped vertically: AAPLRenderer.mm:349-447).  An image is 3*w*h
 * float RGB, rows bottom-up (row 0 at v = 0: what trc_host_load_png returns).
 *  - A material with textureInfo.type == TRC_TEX_IMAGE and textureIndex < n (an ACTIVE image) takes sample.rgb of image
 *    textureIndex as its colour, NOT multiplied by albedo (Texture.hh:33-34).  textureIndex >= n, or nothing uploaded: the
 *    colour is the albedo, as without textures (the reference's nullptr branch).
 *  - uv: where Checker's comes from -- spheres and squares derive theirs from the hit (Sphere.hh:19-31, Square.hh), cubes
 *    and triangles take the hit record's.  A non-finite component is replaced by 0 before the lookup, and a finite one is
 *    clamped to [-1, 2] (so that u*w stays finite for any vt of a mesh).
 *  - Lookup (trc_set_environment_map's, level 0, clamp to edge, float32, no contraction): x = u*w - 0.5, y = v*h - 0.5,
 *    x0 = floor(x), fx = x - x0, column indices x0 and x0 + 1 clamped to [0, w-1] (y likewise);
 *    top = (1 - fx) * t(x0, y0) + fx * t(x1, y0), bottom likewise on row y1, result (1 - fy) * top + fy * bottom.
 *    No mip chain, no wrap modes, no sRGB decoding.
 *  - Emitters keep Le = textureInfo.albedo (Render.metal:109): a texture on a light material changes nothing.
 *  - Textures are context state like the environment map: they survive trc_upload_scene* and do not depend on the order
 *    of the two uploads.  Every call replaces the whole set; n == 0 clears it.  The call drops the denoiser history and
 *    the G-buffer (its albedo plane depends on the textures).
 *  - TRC_ERR_INVALID_ARG: images == NULL with n > 0, a zero size, a NULL rgb or a non-finite texel; TRC_ERR_OOM when the
 *    device allocation fails (the previous set is then cleared).  While an image is active, trc_render refuses
 *    TRC_FLAG_SOBOL and TRC_FLAG_COLLECT_STATS with TRC_ERR_UNSUPPORTED. */
typedef struct trc_image {
    uint32_t     width, height;
    const float* rgb;            /* 3 * width * height floats, rows bottom-up */
} trc_image;
trc_status trc_upload_textures(trc_ctx* ctx, const trc_image* images, uint32_t n);

/* Per-triangle materials.  The reference hard-codes material 19 for every triangle (Triangle.hh:82), and so does every scene
 * upload here; this call gives triangle t (the t-th of idxList, the pIndex of its leaf) the material material[t] instead.
 *  - Everything that reads a hit's material follows: tracePath, traceMIS, traceVolume (the medium of a material), the SPPM
 *    camera and photon passes, the G-buffer's id and albedo planes, trc_trace_rays' hit.material, the work counters.
 *  - n_triangles must equal the scene's n_index / 3 and every index must be below its n_material: TRC_ERR_INVALID_ARG
 *    otherwise, and nothing changes.  TRC_ERR_NO_SCENE before any trc_upload_scene*.
 *  - material == NULL with n_triangles == 0 restores 19 everywhere; every trc_upload_scene* restores it too.
 *  - Launches kept back for coalescing run first; the G-buffer and the denoiser history are dropped, as are the recorded block
 *    costs of the launch planner.  trc_sppm_frames sees the new materials at its next call: a consistent SPPM pass restarts
 *    with trc_sppm_init.  Image textures stay active as before (the whole material table decides that).
 *  - Without TRC_FLAG_MESH_LIGHTS traceMIS samples squareList[5] / [6] only: an emissive triangle is reached by BSDF sampling
 *    alone, with the reference's emitter-hit weighting (against hitRecord.PDF, which a triangle does not write).  With the
 *    flag the emissive triangles are sampled lights with a weighting of their own (TRC_FLAG_MESH_LIGHTS above); their tables
 *    are rebuilt after this call. */
trc_status trc_upload_triangle_materials(trc_ctx* ctx, const uint32_t* material, uint32_t n_triangles);
/* Moving geometry: replaces vertices [first, first + count) of the uploaded scene's triList by new positions, normals and uv, and
 * refits the tree in place.  The host of an animation calls it once per frame instead of uploading the scene again.
 *  - The topology does not change: parent, left, right, axis, pType and pIndex of every record stay, and so does the child order
 *    of the device's nodes.  The index list and the triangle count stay; spheres, squares and cubes do not move (they move by
 *    trc_update_primitives).
 *  - A triangle leaf's box becomes what trc_host_build_node gives, under the identity matrix, for the box of its three CURRENT
 *    vertices (what TRC_TREE_TRIANGLE_LEAVES writes at an upload).  An interior box becomes the component-wise min / max of its two
 *    children's boxes; where the two bounds compare equal (-0 against +0) the right child's is kept, as by trc_host_build_tree.  The
 *    root's box is the union of its two children.  Leaves of analytic primitives keep their boxes.  Only min and max of the
 *    children are involved, so the result does not depend on the order of execution.  A tree of trc_host_build_tree refitted with
 *    unchanged vertices is that tree again, bit for bit (tests/test_refit_cpu.py).
 *  - Rendering after the call is rendering through that tree with those vertices: the same frame, RNG texture and ray counts as
 *    uploading that tree with trc_upload_scene.
 *  - It works on the tree of any upload: trc_upload_scene (the caller's tree), trc_upload_scene_lbvh / _sah / _device with or
 *    without TRC_TREE_TRIANGLE_LEAVES.  For the device-built trees trc_download_bvh returns the refitted records afterwards; the
 *    padding lane of a rewritten box corner is 0.
 *  - The per-triangle materials of trc_upload_triangle_materials survive.
 *  - TRC_ERR_NO_SCENE before any upload.  TRC_ERR_INVALID_ARG: vertices == NULL with count > 0, first + count > the scene's
 *    n_vertex, a position that is not finite or has a coordinate beyond 1e37 in magnitude (trc_upload_scene_sah's bound), or
 *    count > 0 on a scene without triangles.  On any of these errors nothing has changed (state
 *    derived from the old geometry is dropped only once the new vertices are on their way to the device).  count == 0 is TRC_OK and changes nothing.
 *  - Launches kept back for coalescing run first.  The G-buffer and the denoiser history are dropped, as by trc_upload_scene*.  The
 *    tables of TRC_FLAG_MESH_LIGHTS are freed and rebuilt at the next flagged render (the areas changed).  trc_sppm_frames sees the
 *    new geometry at its next call: a consistent SPPM pass restarts with trc_sppm_init.  The accumulator and the RNG texture are
 *    not touched: the caller clears.  Textures, the environment, the camera, the density grid and the triangle materials stay.
 *  - The launch planner's block costs are KEPT, as after a small camera move: the next launch is one pass ordered by the last
 *    launch's raw durations.  Scheduling only, never a pixel.
 *  - The new vertices are copied out of the caller's array before the call returns; the kernels run behind it on the context's
 *    stream, like trc_render's.  (The root's box is an argument of every later launch: 24 bytes are copied back behind the refit,
 *    and the next entry point that is entered waits for them.  The first update of a scene also waits once for its maps.)
 *  - In a group every rank calls it for itself; it is not collective.
 *  - It repairs nothing: after a large deformation the tree is valid but slow to walk, and a host that wants a fresh one calls
 *    trc_rebuild_tree (trc_tree_cost tells it when).  Only the triangles that name a changed vertex get their records rewritten; every box of the tree is
 *    recomputed.
 * The scene's vertex and index arrays stay on the device for this call (32 B per vertex + 12 B per triangle beside the blob),
 * freed by the next trc_upload_scene* and by trc_destroy.
 * Knob refit_single (trc_debug_set): 0 = one launch per depth of the tree (the default), 1 = one launch with a counter per node. */
trc_status trc_update_vertices(trc_ctx* ctx, const trc_TriangleVertex* vertices, uint32_t first, uint32_t count);
/* device time in ms of the kernels of the last trc_update_vertices (record rewrite + refit, without the transfer).  It reports the
 * device time of the last call of the family -- trc_update_vertices, trc_pose_vertices, trc_skin_vertices, trc_morph_vertices,
 * trc_recompute_normals (gather + record rewrite; the one-off adjacency build is not in it), trc_update_primitives (record repack +
 * refit) -- whichever came last. */
trc_status trc_debug_refit_ms(trc_ctx* ctx, float* ms);
/* Moving analytic primitives: replaces spheres [first_sphere, first_sphere + n_sphere), squares [first_square, ..) and cubes
 * [first_cube, ..) of the uploaded scene's lists by new records and refits the tree in place, once for all three kinds.  The host of
 * an animation calls it once per frame instead of uploading the scene again: a light square, a sphere or a cube moves without the
 * mesh beside it being touched.  The records are the reference's PODs, exactly what trc_upload_scene* takes.
 *  - Records.  Each record is repacked on the device, one thread per primitive, into the device's record with the bits an upload
 *    gives for it.  Sphere: center, radius, material.  Square: range_i, range_j, value_k, 1 / (2 * di * dj) with di = range_i.y -
 *    range_i.x and dj = range_j.y - range_j.x (each operation one binary32 operation, 2 * di first, the division correctly rounded),
 *    the three axes, material.  Cube: the xyz rows of the four inverse_matrix, the four model_matrix and the first three normal_matrix
 *    columns, box, material.  Nothing else of a record is read, except by the leaf box below.
 *  - Leaf box.  A primitive's leaf box becomes what trc_host_build_node gives for boundingBOX under model_matrix (sphere, square) or
 *    box under model_matrix (cube): the eight corners in the order i, j, k, each row ((m0 * x + m1 * y) + m2 * z) + m3 * 1 without
 *    contraction, into fmin / fmax from +-FLT_MAX, the second operand kept on a tie.  It is written into the slot of the node that
 *    holds the leaf; for a device-built tree trc_download_bvh returns it in the leaf's record, padding lane 0.  A primitive that no
 *    leaf names -- the density container cube of the scenes other than TRC_SCENE_CORNELL_VOLUME, the spheres of a scene whose tree
 *    leaves them out -- gets its record rewritten and nothing else.  (Where two leaves name one primitive, one of them follows.)
 *  - Refit.  Every interior box and the root's are then recomputed as by trc_update_vertices (same rule, same two kernels, knob
 *    refit_single); triangle leaves keep their boxes and no triangle record is rewritten.  The topology does not change: parent,
 *    left, right, axis, pType and pIndex of every record stay, and the number of primitives of each kind stays.
 *  - Rendering, trc_trace_rays and trc_denoise after the call are what they are after trc_upload_scene of that tree with those
 *    primitive lists: the same frame, RNG texture and ray counts, bit for bit.  It works on the tree of any upload; trc_rebuild_tree
 *    after it builds from the new leaf boxes, trc_tree_cost sees them.
 *  - Kept: vertices and indices, the rest copy, skin and morph bindings, triangle materials, the normals' adjacency, textures, the
 *    environment, the camera, the density grid, and the launch planner's block costs (as after trc_update_vertices: the next launch
 *    is one pass ordered by the last launch's raw durations).  The accumulator and the RNG texture are not touched: the caller clears.
 *  - Dropped: the G-buffer and the denoiser history, as by trc_upload_scene* (with trc_denoise_track_motion on the history is kept
 *    and follows the primitives: "Motion tracking" below).  The tables of TRC_FLAG_MESH_LIGHTS are freed and rebuilt at the next
 *    flagged render.
 *    trc_sppm_frames sees the new geometry at its next call: a consistent SPPM pass restarts with trc_sppm_init.
 *  - TRC_ERR_NO_SCENE before any upload.  TRC_ERR_INVALID_ARG: r == NULL; a NULL list with a count > 0; first + n beyond the scene's
 *    count of that kind (the sum is never formed in 32 bits); a material >= the scene's n_material; a square axis > 2; a value
 *    that is not finite or beyond 1e37 in magnitude among the fields named above, boundingBOX / box and the xyz rows of model_matrix.
 *    On any of these errors nothing has changed.  All three counts zero is TRC_OK and changes nothing, the denoiser's history included.
 *  - Launches kept back for coalescing run first.  The records are copied out of the caller's arrays before the call returns; the
 *    kernels run behind it on the context's stream (the root's box comes back as after trc_update_vertices, and the first call of the
 *    family on a scene and tree waits once for its maps, which now include 4 bytes per analytic primitive).
 *  - In a group every rank calls it for itself; it is not collective. */
typedef struct trc_primitive_ranges {
    const trc_Sphere* spheres; uint32_t first_sphere, n_sphere;   /* replace sphereList[first .. first+n) */
    const trc_Square* squares; uint32_t first_square, n_square;
    const trc_Cube*   cubes;   uint32_t first_cube,   n_cube;
} trc_primitive_ranges;                                           /* 48 bytes */
trc_status trc_update_primitives(trc_ctx* ctx, const trc_primitive_ranges* r);
/* Posed geometry: the rigid (or affine) animation of whole objects, where the host has nothing to say per frame but one matrix per
 * object.  Each trc_pose names vertices [first, first + count) of the scene's triList and the two matrices to put them under; the
 * device computes the posed vertices from a REST copy it keeps, and the record rewrite and refit of trc_update_vertices run behind.
 *  - Rest vertices: the values the caller last gave -- by trc_upload_scene*, then by any trc_update_vertices for its range.  A pose
 *    is always applied to the rest vertices, never to the previous pose: frame k is M_k * rest, and nothing drifts.  Vertices in no
 *    range of a call keep their current values, which may be an earlier call's pose.
 *  - Position, binary32, no contraction, c0..c3 the columns of model_matrix, in this order (simd's matrix times vector, which the
 *    reference's placement of a primitive uses):  x' = ((c0.x*x + c1.x*y) + c2.x*z) + c3.x, and y', z' alike with .y and .z.  The
 *    fourth row (the .w lanes) is not read.
 *  - Normal, N = normal_matrix:  n' = (N.c0*nx + N.c1*ny) + N.c2*nz per component, no translation and NOT normalised (the reference
 *    shades in the frame of the normal as stored).  The caller passes the inverse transpose of the model matrix; for a rigid pose
 *    that is the rotation itself.  Column 3 and the .w lanes are not read.  uv is copied.
 *  - An identity pose reproduces the rest values as values; a -0 may come back as +0 (-0 + 0*y is +0).
 *  - After the call everything observable is what trc_update_vertices would have left had the host computed those vertices and
 *    passed them: triangle records, leaf and interior boxes (the right child's bound on a tie), the root box, the records of
 *    trc_download_bvh, frames, RNG texture and ray counts, the G-buffer, the tables of TRC_FLAG_MESH_LIGHTS.  The one exception: the
 *    rest copy stays what it was.  It works on the tree of every upload path and with both values of knob refit_single.  The same
 *    things survive (triangle materials, textures, environment, camera, density, accumulator, RNG texture) and the same are dropped
 *    (G-buffer, denoiser history, mesh-light tables); the launch planner's block costs are kept.  Launches kept back for coalescing
 *    run first.  Not collective.  The 144 * n_poses bytes are copied out of the caller's array before the call returns; the kernels
 *    run behind it on the context's stream.
 *  - TRC_ERR_NO_SCENE before any upload.  TRC_ERR_INVALID_ARG: poses == NULL with n_poses > 0, a range with count == 0 or with
 *    first + count > the scene's n_vertex, two ranges that overlap, a non-finite value among the 21 matrix entries that are read, or
 *    n_poses > 0 on a scene without triangles.  TRC_ERR_OOM if the rest copy cannot be allocated.  On any error nothing has changed.
 *    n_poses == 0 is TRC_OK and changes nothing.  The ranges may come in any order.
 *  - Overflow: the host cannot check posed positions without computing them.  Keeping every posed position finite and within 1e37
 *    in magnitude (trc_update_vertices' bound) is the CALLER's contract.  The kernel counts the positions that break it, and
 *    trc_debug_pose_overflows reports the count of the last trc_pose_vertices (it waits for that call's kernels).  A frame rendered
 *    after a non-zero count is not defined; no index is ever derived from a position, so nothing is read or written out of bounds,
 *    and a later pose within the bound (or any trc_update_vertices / upload) makes the scene well defined again.
 * The rest copy is 32 B per vertex more device memory, allocated by the first trc_pose_vertices of a scene (a copy of the vertices
 * as they are then) and freed with the scene; a host that never poses pays nothing.  While it exists trc_update_vertices writes
 * its range into it as well. */
typedef struct trc_pose {
    uint32_t     first, count;     /* vertices [first, first + count) of the scene's triList */
    uint32_t     _pad[2];
    trc_float4x4 model_matrix;     /* positions */
    trc_float4x4 normal_matrix;    /* normals: the caller's inverse transpose (the rotation itself for a rigid pose) */
} trc_pose;
trc_status trc_pose_vertices(trc_ctx* ctx, const trc_pose* poses, uint32_t n_poses);
/* the CURRENT vertices [first, first + count) as they are on the device (position, normal, uv): what the last upload, update or pose
 * left.  TRC_ERR_NO_SCENE before any upload; TRC_ERR_INVALID_ARG: first + count > the scene's n_vertex, out == NULL with count > 0, or
 * a scene without triangles.  count == 0 on a scene with triangles is TRC_OK.  Synchronous, like every download. */
trc_status trc_download_vertices(trc_ctx* ctx, trc_TriangleVertex* out, uint32_t first, uint32_t count);
/* the number of posed positions of the last trc_pose_vertices, of skinned positions of the last trc_skin_vertices, or of final positions
 * of the last trc_morph_vertices -- whichever of the three calls came last -- that came out non-finite or beyond 1e37 in magnitude (0
 * before any) */
trc_status trc_debug_pose_overflows(trc_ctx* ctx, uint32_t* n);
/* Skinned geometry: linear blend skinning for whatever bends -- characters, cloth proxies.  trc_skin_bind gives a range of vertices
 * four (bone, weight) influences each, once; trc_skin_vertices takes the frame's bone palette, the device blends the bones' matrices
 * per vertex, puts the REST vertex under the blend, and the record rewrite and refit of trc_update_vertices run behind.
 *  - trc_skin_bind: vertex first + i of the scene's triList gets influences[i].  A scene has ONE binding, which is one range: a
 *    second call replaces it, count == 0 removes it (influences may then be NULL).  Weights need not sum to 1 and may be zero or
 *    negative: the definition below is what runs.  The table is copied to the device before the call returns: 32 B per bound vertex
 *    of device memory, freed with the scene (every trc_upload_scene*, trc_destroy).  A bind alone moves no vertex and drops nothing.
 *    TRC_ERR_NO_SCENE before any upload.  TRC_ERR_INVALID_ARG: influences == NULL with count > 0, first + count > the scene's
 *    n_vertex, a weight that is not finite, a bone index >= TRC_SKIN_MAX_BONES (whatever its weight), or count > 0 on a scene without
 *    triangles.  TRC_ERR_OOM if the table cannot be allocated.  On any error the previous binding stays and nothing has changed.
 *    The binding survives trc_update_vertices, trc_pose_vertices and trc_upload_triangle_materials.
 *  - trc_skin_vertices: bones[b] is bone b's model_matrix and normal_matrix (the caller's inverse transpose).  Every bound vertex is
 *    computed from its REST vertex -- the rest copy of trc_pose_vertices: the caller's last values by upload or trc_update_vertices,
 *    allocated by whichever of the two calls comes first (32 B per vertex), never written by a pose or a skin -- so frame k never
 *    builds on frame k - 1.  Vertices outside the binding keep their current values; a pose may name bound vertices, the next skin
 *    overwrites them from rest.
 *  - Definition, binary32, one rounding per operation, no contraction; (b_k, w_k), k = 0..3, the vertex's influences, M = bones[.].
 *    For each of the 12 entries e that a pose reads of a model matrix (.x .y .z of columns 0..3):
 *        B.e = ((w0*M[b0].e + w1*M[b1].e) + w2*M[b2].e) + w3*M[b3].e
 *    and the same blend of the 9 entries read of the normal matrices (.x .y .z of columns 0..2) gives BN.  Then exactly
 *    trc_pose_vertices' expressions with B for model_matrix and BN for normal_matrix: x' = ((B.c0.x*x + B.c1.x*y) + B.c2.x*z) + B.c3.x,
 *    n' = (BN.c0*nx + BN.c1*ny) + BN.c2*nz, not normalised, uv copied.  The .w lanes and column 3 of the normal matrix are not read.
 *    So a vertex with one weight 1.0f and three weights 0.0f (any valid bone indices) gets, as values, what trc_pose_vertices gives it
 *    with that bone's two matrices; a -0 may come back as +0.
 *  - After the call everything observable is what trc_update_vertices would have left had the host computed those vertices and passed
 *    them, as for a pose: the same things survive, the same are dropped, the block costs are kept, launches kept back for coalescing
 *    run first, not collective.  The 128 * n_bones bytes are copied out of the caller's array before the call returns; the kernels
 *    run behind it on the context's stream.  The refit runs over the binding's range.
 *  - TRC_ERR_NO_SCENE before any upload.  n_bones == 0 is TRC_OK and changes nothing.  Otherwise TRC_ERR_INVALID_ARG: no binding,
 *    bones == NULL, n_bones > TRC_SKIN_MAX_BONES, n_bones <= the largest bone index of the binding, or a non-finite value among the
 *    21 entries read of any of the n_bones bones.  TRC_ERR_OOM if the rest copy or the palette buffer cannot be allocated.  On any
 *    error nothing has changed.  No index on the device comes from anything the host has not checked.
 *  - Overflow: as for a pose, keeping skinned positions finite and within 1e37 is the CALLER's contract; the kernel counts the ones
 *    that break it and trc_debug_pose_overflows reports the count.
 *  - Knob skin_no_lds (trc_debug_set): palettes of up to 256 bones are staged in LDS once per workgroup; 1 = always gather the bones
 *    from memory, as larger palettes do.  The same arithmetic on the same operands: never a bit of difference.
 * Out of scope: more than four influences per vertex; dual-quaternion blending; more than one binding per scene (several characters
 * share one palette through offset bone indices); fusing a pose and a skin of the same frame into one refit chain (they are two calls
 * and two chains). */
typedef struct trc_skin_influence { uint32_t bone[4]; float weight[4]; } trc_skin_influence;   /* 32 B */
typedef struct trc_skin_bone { trc_float4x4 model_matrix, normal_matrix; } trc_skin_bone;      /* 128 B */
#define TRC_SKIN_MAX_BONES 65536u
trc_status trc_skin_bind(trc_ctx* ctx, const trc_skin_influence* influences, uint32_t first, uint32_t count);
trc_status trc_skin_vertices(trc_ctx* ctx, const trc_skin_bone* bones, uint32_t n_bones);
/* Morphed geometry: blend shapes (morph targets) for faces, muscle correctives, cloth wrinkles -- v = rest + sum of w_k * delta_k -- alone
 * or with the skin of trc_skin_bind on top, which is the order of a character pipeline (glTF's: morph first, then the bones).
 * trc_morph_bind gives a range of vertices n_targets deltas each, once; trc_morph_vertices takes the frame's weights, the device adds the
 * weighted deltas to the REST vertex, and the record rewrite and refit of trc_update_vertices run behind.
 *  - trc_morph_bind: deltas[k * count + i] is target k's delta (dv to the position, dn to the normal) for vertex first + i of the
 *    scene's triList: target-major, so that a wavefront reads consecutive bytes.  A scene has ONE morph binding, which is one range: a
 *    second call replaces it, count == 0 or n_targets == 0 removes it (deltas may then be NULL and the other arguments are not looked
 *    at).  The table is copied to the device before the call returns: 24 B per bound vertex PER TARGET of device memory, freed with the
 *    scene (every trc_upload_scene*, trc_destroy).  A bind alone moves no vertex and drops nothing.  TRC_ERR_NO_SCENE before any
 *    upload.  TRC_ERR_INVALID_ARG: deltas == NULL with a non-empty table, first + count > the scene's n_vertex, n_targets >
 *    TRC_MORPH_MAX_TARGETS, a delta component that is not finite, or a non-empty table on a scene without triangles.  TRC_ERR_OOM if the
 *    table cannot be allocated.  On any error the previous binding stays and nothing has changed.  The binding survives
 *    trc_update_vertices, trc_pose_vertices, trc_skin_bind, trc_skin_vertices, trc_upload_triangle_materials and trc_rebuild_tree.
 *  - trc_morph_vertices, definition: binary32, one rounding per operation, no contraction.  The ACTIVE LIST is the targets k,
 *    ascending, whose weights[k] is not zero (neither +0 nor -0 counts).  For bound vertex i the accumulator starts as the six rest
 *    values (x y z nx ny nz) of the rest copy (trc_skin_vertices says what that is); then for every active k in order and every
 *    component c:  p = w_k * d[k][i].c;  acc.c = acc.c + p.  uv is copied, normals are NOT normalised.  With no active target the
 *    vertex is the rest vertex bit for bit, a -0 included: zero weights are skipped, not multiplied -- which is also what makes a
 *    rig of hundreds of mostly idle targets cheap.
 *  - n_bones == 0 (bones is not looked at): morph only.  Vertices outside the binding keep their current values.
 *  - n_bones > 0: the skin of trc_skin_bind runs on top, in the same kernel and the same single refit chain.  A vertex in both
 *    bindings gets trc_skin_vertices' expressions applied to its MORPHED six values in place of its rest values; a vertex in the skin
 *    binding only is skinned from rest; a vertex in the morph binding only is morphed.  The refit runs over the hull of the two
 *    ranges; a vertex of the hull that is in neither binding is not written.  This call is the only way to skin(rest + morph): a
 *    later plain trc_skin_vertices skins from rest again, as it always did.
 *  - After the call everything observable is what trc_update_vertices would have left had the host computed those vertices and passed
 *    them, as for a pose or a skin: the rest copy stays, the same things survive, the same are dropped, the block costs are kept,
 *    launches kept back for coalescing run first, not collective.  The 4 * n_weights bytes, and the 128 * n_bones bytes of a palette,
 *    are copied out of the caller's arrays before the call returns; the kernels run behind it on the context's stream.
 *  - TRC_ERR_NO_SCENE before any upload.  TRC_ERR_INVALID_ARG: no morph binding, weights == NULL, n_weights != the binding's n_targets,
 *    a weight that is not finite, and with n_bones > 0 everything trc_skin_vertices refuses, a missing skin binding included.
 *    TRC_ERR_OOM if the rest copy or the small buffers cannot be allocated.  On any error nothing has changed.  No index on the device
 *    comes from anything the host has not checked.
 *  - Overflow: as for a pose, keeping the final positions finite and within 1e37 is the CALLER's contract; the kernel counts the ones
 *    that break it and trc_debug_pose_overflows reports the count.
 * Out of scope: sparse targets (a target that names few vertices still stores a delta for every bound vertex); more than one morph
 * binding per scene; a morph under a trc_pose_vertices in one chain (they are two calls and two chains); re-derived (renormalised)
 * normals. */
typedef struct trc_morph_delta { float dv[3]; float dn[3]; } trc_morph_delta;   /* 24 B, packed */
#define TRC_MORPH_MAX_TARGETS 1024u
trc_status trc_morph_bind(trc_ctx* ctx, const trc_morph_delta* deltas, uint32_t n_targets, uint32_t first, uint32_t count);
trc_status trc_morph_vertices(trc_ctx* ctx, const float* weights, uint32_t n_weights, const trc_skin_bone* bones, uint32_t n_bones);
/* Re-derived normals: a pose puts the stored normal under the caller's inverse transpose, a skin under a blend of inverse transposes
 * (which is not the inverse transpose of the blend), a morph adds linear deltas, and none of them normalises -- so a bent or morphed
 * mesh is shaded with normals that are neither unit length nor perpendicular to the surface it now has.  trc_recompute_normals
 * replaces the normals of vertices [first, first + count) of the scene's CURRENT vertices by area-weighted smooth normals of the mesh
 * as it now stands, on the device: no vertex crosses the bus.  A host calls it after each update, pose, skin or morph it wants shaded
 * that way.
 *  - Definition: binary32, one rounding per operation, no contraction.
 *    Face term of triangle t with current positions p0, p1, p2 in index-list order: e1 = p1 - p0, e2 = p2 - p0,
 *        c.x = e1.y*e2.z - e1.z*e2.y,  c.y = e1.z*e2.x - e1.x*e2.z,  c.z = e1.x*e2.y - e1.y*e2.x
 *    (the e1, e2 and c of TRC_FLAG_MESH_LIGHTS' triangle area; its length is twice the area, which is the weight).
 *    Vertex sum: the CORNER LIST of vertex v is every k with idxList[k] == v, ascending in k.  s starts as (+0, +0, +0); for every
 *    corner in that order s = s + c(k / 3), component by component.  A triangle that names v twice contributes twice.
 *    Side: n_cur is the normal the vertex holds when the call starts, d = (s.x*n_cur.x + s.y*n_cur.y) + s.z*n_cur.z.  If d < 0 then
 *    s = -s; any other d, zero and NaN included, leaves s alone.  (The winding of a mesh need not agree with its stored normals:
 *    trc_host_scene_create mirrors z when it places a mesh, which turns every winding round and leaves the ball of
 *    trc_host_mesh_make_ball wound against its normals at every vertex.  Every pose, skin and morph leaves an interpolated normal
 *    behind, which is the hemisphere guide this rule needs.)
 *    Normalise: q = (s.x*s.x + s.y*s.y) + s.z*s.z, l = sqrt(q) correctly rounded.  If l is finite and > 0 then
 *    n = (s.x / l, s.y / l, s.z / l) with IEEE division.  Otherwise the vertex keeps the bits of the normal it had: a vertex with no
 *    corner, one with zero-area triangles only, overflow or underflow of q.
 *  - Vertices outside the range keep their normals, even where a triangle is shared (their positions are read).  Positions, uv, every
 *    box of the tree, the root box, the rest copy and all bindings are untouched.  trc_download_vertices returns the new normals, and
 *    the attribute records of every triangle that names a vertex of the range hold them; the triangle's material is kept.
 *  - After the call everything observable is what trc_update_vertices would have left had the host computed those vertices and passed
 *    them, with one exception: the rest copy is NOT written.  The next pose, skin or morph derives its normals from rest again, as
 *    always; a host calls this after each of them.  What survives: triangle materials, textures, environment, camera, density,
 *    accumulator, RNG texture, the skin and morph bindings, the refit maps.  What is dropped: the G-buffer, the denoiser history and
 *    the tables of TRC_FLAG_MESH_LIGHTS (they do not depend on normals; one rule for every call that changes vertices).  The launch
 *    planner's block costs are kept.  Launches kept back for coalescing run first.  Not collective.
 *  - The first call of a scene builds the vertex -> corner adjacency on the device from the index list it keeps (no index crosses the
 *    bus) and waits for that once: 4 * (n_vertex + 1) + 4 * n_index bytes of device memory, freed with the scene (every
 *    trc_upload_scene*, trc_destroy), kept across trc_rebuild_tree, the four animation calls and trc_upload_triangle_materials.  Every
 *    later call is asynchronous on the context's stream, like trc_render.
 *  - TRC_ERR_NO_SCENE before any upload.  count == 0 is TRC_OK and changes and drops nothing.  TRC_ERR_INVALID_ARG: first + count > the
 *    scene's n_vertex, or count > 0 on a scene without triangles.  TRC_ERR_OOM if the adjacency cannot be allocated.  On any error
 *    nothing has changed and nothing is dropped.  No index on the device comes from anything the host has not checked.
 * Out of scope: welding of duplicated seam vertices (two vertices at one position are two vertices); smoothing groups and crease angles;
 * angle weighting; writing the rest copy; fusing into the morph or skin kernel's chain (it is a second, short chain). */
trc_status trc_recompute_normals(trc_ctx* ctx, uint32_t first, uint32_t count);
/* A fresh tree for a moved mesh.  A refit keeps the topology of the tree it found: after objects have travelled past each other the boxes
 * near the top overlap and every ray walks more of them.  trc_rebuild_tree builds the tree anew from what the DEVICE holds -- no vertex,
 * index or record crosses the bus, nothing but the tree changes -- and trc_tree_cost (below) tells a host when to ask for it.
 *  - The tree afterwards is the tree trc_upload_scene_sah builds from the scene's current LEAF RECORDS when flags == TRC_TREE_SAH, and
 *    the tree trc_upload_scene_lbvh builds from them when flags == 0: record for record in trc_download_bvh, fat node for fat node on
 *    the device, with the LDS plan of that upload.  The vertices, the triangle records and the primitives are those it found: no vertex
 *    moves.
 *  - Leaf records of a device-built tree (trc_upload_scene_lbvh / _sah / _device): slots 1..n of trc_download_bvh, in the order of the
 *    upload, with the boxes the last upload or refit left them.  So after any update, pose or skin a TRC_TREE_SAH rebuild of a
 *    TRC_TREE_TRIANGLE_LEAVES scene equals a fresh context's trc_upload_scene_device(TRC_TREE_SAH | TRC_TREE_TRIANGLE_LEAVES) of the same
 *    analytic leaves and the vertices of trc_download_vertices.
 *  - Leaf records of a caller's tree (trc_upload_scene): the caller's bvhList is gone, so the leaf list has a canonical order -- by pType
 *    ascending, then by pIndex (the order of first[pType] + pIndex, first[] the prefix sums of the scene's sphere, square, cube and
 *    triangle counts).  A leaf's box is the one its child slot holds on the device (the caller's, or the last refit's), padding lanes
 *    0; parent, left, right and axis are 0.  A primitive that the caller's tree leaves out (the Cornell scenes list spheres that no
 *    leaf names) has no leaf afterwards either.  A tree that names one primitive in two leaves has no such list:
 *    TRC_ERR_UNSUPPORTED, nothing changes.  Afterwards the scene is a device-built one: trc_download_bvh and trc_lbvh_info work on it.
 *  - What survives: the kept vertex and index arrays, the rest copy of trc_pose_vertices / trc_skin_vertices and the skin and morph bindings; the
 *    triangle records with their per-triangle materials; textures, the environment, the camera, the density grid, the accumulator and the
 *    RNG texture (the caller clears).  The launch planner's block costs are KEPT as after trc_update_vertices: scheduling only.
 *  - What is dropped: the G-buffer and the denoiser history (a tie in t may now resolve to another primitive); the tables of
 *    TRC_FLAG_MESH_LIGHTS (rebuilt at the next flagged render); the maps of the refit, which the next trc_update_vertices,
 *    trc_pose_vertices or trc_skin_vertices makes again for the new topology, as the first update of a scene does.  trc_sppm_frames sees
 *    the new tree at its next call.
 *  - The leaf count does not change, so neither does the layout of the device's scene: the node region and the tree records are
 *    rewritten in place, only temporaries are allocated, and nothing larger than the build's small read-backs is transferred.
 *  - flags == (TRC_TREE_SAH | TRC_TREE_SAH3): the tree trc_upload_scene_device(TRC_TREE_SAH | TRC_TREE_SAH3) builds from those leaf
 *    records; everything else in this list holds for it unchanged.
 *  - Atomic on error.  TRC_ERR_INVALID_ARG: a flag other than TRC_TREE_SAH and its modifier TRC_TREE_SAH3 (TRC_TREE_TRIANGLE_LEAVES
 *    included: the leaves are the device's), or TRC_TREE_SAH3 without TRC_TREE_SAH.  TRC_ERR_NO_SCENE before any upload.  TRC_ERR_UNSUPPORTED: see above.  TRC_ERR_BVH_INVALID: a tree deeper than
 *    TRC_MAX_BVH_DEPTH, or a leaf box the SAH build does not take.  TRC_ERR_OOM: the temporaries.  All of them are found before the
 *    first byte of the old tree is overwritten: a render after a refused call gives the frame it would have given before it.
 *  - Launches kept back for coalescing run first.  Not collective.  The call waits where an upload waits -- the read-backs of the build
 *    -- and returns with the tree in place.  trc_lbvh_info reports the rebuild's height and device time. */
trc_status trc_rebuild_tree(trc_ctx* ctx, uint32_t flags);       /* flags: 0 (LBVH + rotations), TRC_TREE_SAH or TRC_TREE_SAH | TRC_TREE_SAH3 */
/* A surface-area measure of the tree as it stands, on any upload path (it reads the device's nodes): one kernel pass over 64 bytes per
 * interior node on the context's stream; synchronous like a download.  Launches kept back for coalescing run first.
 *  - For a box, d = max - min per axis in binary32, and a d that is not > 0 counts as 0; its half area is
 *    h = ((double)dx * dy + (double)dy * dz) + (double)dz * dx.  A product of two binary32 values is exact in binary64, so contraction
 *    cannot change a bit of h.
 *  - root_half_area is h of the root's box.  A tree of n leaves has n - 1 interior nodes with two child slots each: interior_half_area is
 *    the sum of h over the n - 2 slots that hold an interior child, leaf_half_area over the n slots that hold a leaf; n_interior and
 *    n_leaves count those slots (exact).  The sums are binary64 additions in the order the reduction takes: any order of n non-negative
 *    terms is within (n - 1) * 2^-53 relative of the exact sum.  Defined for boxes within the 1e37 bound of the device builds.
 *  - The expected cost of a ray through the tree, up to the host's own constants: (Ct * interior_half_area + Ci * leaf_half_area) /
 *    root_half_area with Ct the price of a box step and Ci that of a leaf test.  A refit changes it, a rebuild resets it: a host compares
 *    the value with the one right after its last build (examples/trc_render --rebuild-ratio).
 *  - TRC_ERR_NO_SCENE before any upload; TRC_ERR_INVALID_ARG: out == NULL. */
typedef struct trc_tree_cost_t {
    double   root_half_area, interior_half_area, leaf_half_area;
    uint32_t n_interior, n_leaves;
} trc_tree_cost_t;
trc_status trc_tree_cost(trc_ctx* ctx, trc_tree_cost_t* out);
/* Which of the mesh's triangles exist.  An object that enters or leaves a shot, a prop that is switched off, an LOD swap: without this
 * call they cost trc_download_vertices and a whole trc_upload_scene*, which drops the rest copy, the bindings, the per-triangle materials,
 * the block costs, the normals' adjacency and the denoiser history.  trc_set_triangle_visibility changes a per-triangle mask and builds the
 * tree over the leaves that are left, from what the DEVICE holds.  Triangle t is the t-th of idxList, as for trc_upload_triangle_materials.
 *  - Mask.  One bit per triangle.  Until the first call of a scene it is implicit: a triangle is visible iff a leaf of the tree in use
 *    names it.  The first call (set or download) makes it explicit on the device, one byte per triangle.  A tree that names one triangle in
 *    two leaves has no such mask: TRC_ERR_UNSUPPORTED, nothing changes (the case trc_rebuild_tree refuses).  Every trc_upload_scene*
 *    drops the mask; the next tree defines it again.
 *  - Ranges are applied in the order given, a later range wins.  visible is 0 or 1, first + count <= n_index / 3.  n_ranges == 0 is
 *    legal: the leaf list below is built from the mask as it stands.
 *  - The leaf list has two parts.  First the analytic leaves (spheres, squares, cubes): the records trc_rebuild_tree would start from at
 *    this moment -- slots 1..n of trc_download_bvh for a device-built tree, the canonical order for a caller's tree -- filtered to
 *    pType != TRC_PRIM_TRIANGLE, in that order, with the boxes they hold.  Then one record per visible triangle, ascending t: pType
 *    TRC_PRIM_TRIANGLE, pIndex t, the box BVH::buildNode of its three CURRENT vertices (the bits an upload with TRC_TREE_TRIANGLE_LEAVES
 *    writes), padding lanes 0, parent, left, right and axis 0.  One rule for every triangle, because a triangle that was hidden while its
 *    vertices moved has no stored box.  Its consequence: a visible triangle whose caller-supplied leaf box was not buildNode of its
 *    vertices gets the canonical box (the project's scene builders never make such a box).
 *  - Tree.  Over that list of n' leaves: the tree trc_upload_scene_sah builds from it (tree_flags == TRC_TREE_SAH), trc_upload_scene_lbvh
 *    (0), or trc_upload_scene_device(TRC_TREE_SAH | TRC_TREE_SAH3) (those two flags) -- record for record in trc_download_bvh (2 n' - 1
 *    records), fat node for fat node on the device, with the LDS plan of that upload: a scene that shrinks enough becomes LDS-resident.
 *    Afterwards the scene is a device-built one; a later trc_rebuild_tree takes slots 1..n', the visible leaves only.
 *  - Capacity.  The layout of the device's scene does not move: the node region keeps the room of the tree that was uploaded, and the
 *    reference-layout array is allocated for that many leaves; the counts trc_download_bvh and trc_lbvh_info report follow n'.  Showing
 *    everything again fits without reallocating the scene.  A caller's tree that left triangles out was laid out for its own leaf count: a
 *    call that would leave more leaves than that is TRC_ERR_INVALID_ARG.
 *  - What survives and what is dropped: trc_rebuild_tree's list, block costs kept.  With trc_denoise_track_motion on the G-buffer is
 *    stale and the history kept; a pixel whose surface appeared or vanished fails the id / depth test and starts again at length 1.
 *    Hidden triangles keep their records, vertices, materials and bindings: every animation call goes on computing their vertices and
 *    rewriting their records (they have no leaf to refit), and trc_recompute_normals still sums over them -- the adjacency is the index
 *    list's.  Under TRC_FLAG_MESH_LIGHTS a hidden triangle is no light: weight 0, pdfA 0; the tables are rebuilt at the next flagged render.
 *  - Atomic on error: mask and tree are as they were, and everything that can refuse comes before the first byte of the tree in use is
 *    overwritten.  TRC_ERR_INVALID_ARG: ranges == NULL with n_ranges > 0, a range beyond n_index / 3, visible > 1, a flag other than
 *    TRC_TREE_SAH and its modifier TRC_TREE_SAH3 (or the modifier alone), fewer than 2 leaves left, more than 2^31 - 2 ranges.
 *    TRC_ERR_NO_SCENE, TRC_ERR_UNSUPPORTED (above), TRC_ERR_BVH_INVALID and TRC_ERR_OOM as for trc_rebuild_tree.
 *  - Launches kept back for coalescing run first.  Not collective.  Cost: the ranges' triangles are stamped once each, then three
 *    streaming passes over the triangles and the leaves (mask, partition, leaf records), then the build over n' leaves.
 * trc_download_triangle_visibility writes n_index / 3 bytes, 1 = visible (nothing for a scene without triangles); it refuses what the
 * first bullet refuses.  trc_debug_visibility_ms: device time of the last call's leaf-list stage (tools/visibility_bench.py).
 * Out of scope: analytic primitives (move them away with trc_update_primitives); triangles beyond the uploaded index list; partial rebuilds. */
typedef struct trc_triangle_range { uint32_t first, count, visible; } trc_triangle_range;   /* 12 bytes */
trc_status trc_set_triangle_visibility(trc_ctx* ctx, const trc_triangle_range* ranges, uint32_t n_ranges, uint32_t tree_flags);
trc_status trc_download_triangle_visibility(trc_ctx* ctx, uint8_t* out /* n_index / 3 bytes, 1 = visible */);
trc_status trc_debug_visibility_ms(trc_ctx* ctx, float* leaf_list_ms);
trc_status trc_resize(trc_ctx* ctx, uint32_t width, uint32_t height);
/* deterministic stand-in for fillRNG (AAPLRenderer.mm:296-344, arc4random):
 * texel(x,y) = 4 successive pcg32 outputs of pcg32_srandom_r(seed, y*W+x),
 * generated on the device; identical to trc_host_fill_rng. */
trc_status trc_seed(trc_ctx* ctx, uint64_t seed);
trc_status trc_upload_rng(trc_ctx* ctx, const uint32_t* rgba /* 4*W*H */);
trc_status trc_download_rng(trc_ctx* ctx, uint32_t* rgba /* 4*W*H */);
trc_status trc_upload_accum(trc_ctx* ctx, const float* rgba /* 4*W*H */);
/* linear radiance running mean, same meaning as textureA/B (Render.metal:540-543) */
trc_status trc_download_accum(trc_ctx* ctx, float* rgba /* 4*W*H */);
trc_status trc_clear_accum(trc_ctx* ctx);

/* Output stage = what fragmentShader does to the accumulator before display (Render.metal:29-75):
 * auto-exposure from the frame's mean colour (the top mip level there; an exact mean here: per-channel sums in
 * 2^-16 fixed point, so the result does not depend on summation order), luma = dot(mean, (0.2126, 0.7152, 0.0722)),
 * expose = 1 - clamp(CETone(luma, 1), 0, 0.9999) (Render.hh:91-95), ACESTone(rgb, expose) (Render.hh:78-89),
 * no sRGB curve (commented out at :73), 8-bit = (uint8)(clamp(x, 0, 1) * 255 + 0.5), alpha 255.  Rows are
 * written top-down (the shader flips v, :51-56): out row 0 = frame row H-1.  The reference feeds its SVGF-denoised
 * texture here; this takes the raw accumulator (trc_tonemap_denoised below takes the denoised one).  rgba8: host buffer of
 * 4*W*H bytes; exposure_out may be NULL. */
trc_status trc_tonemap(trc_ctx* ctx, uint8_t* rgba8, float* exposure_out);

/* replaces -[AAPLRenderer render:] + kernelPathTracing dispatch
 * (AAPLRenderer.mm:1134-1196, Render.metal:495-558); asynchronous on the
 * context stream; spp samples are fused into one launch with bit-identical
 * results to spp launches of 1 sample.
 * Coalesced launches: a call of fewer than 8 samples (without TRC_FLAG_COLLECT_STATS) is not launched at once but kept, and
 * extended by following calls that continue it (identical parameters, frame0 = where it ends); it is launched when 16 samples
 * have come together, when a call arrives that does not continue it, or when ANY other trc_* entry point taking this context is
 * entered (each launches what was kept before it does anything else).  Results, statistics (trc_stats.launches counts
 * calls) and error behaviour of parameter checks are those of launching every call at once; a HIP error of a kept launch
 * is returned by the call that launches it, and trc_last_error then names the frame range (frame0 .. frame0 + spp - 1) and the
 * number of trc_render calls whose samples did not run, so that a host can re-issue exactly those.  trc_destroy drops a kept
 * launch without launching it (nobody could read its frame); call trc_synchronize first to learn its status.  Knob "no_coalesce"
 * (trc_debug_set) launches every call at once.
 * First launch of a block list (new context, frame size, tile share, scene, camera, integrator), >= 16 samples: run as a
 * head of 8 samples (then passes of 16 and 32 samples where at least four times as many remain) followed by the rest, each
 * pass ordered and split by its predecessor's per-block durations -- the same pixels (a pixel's samples are one chain
 * through its RNG texel); knob "no_cold_probe" runs it as one pass, "head_stages" = n caps the passes before the rest. */
trc_status trc_render(trc_ctx* ctx, const trc_params* params);
trc_status trc_synchronize(trc_ctx* ctx);

/* test hook = Scene::hit (Render.hh:135-252) on a batch of rays (host buffers).  `any_hit` is a bit set: */
#define TRC_TRACE_ANY_HIT     1   /* stop at the first accepted hit closer than tmax (shadow rays, Render.hh:244) */
#define TRC_TRACE_PRODUCTION  2   /* walk the tree with the round the render kernels run (no instrumentation; on trees
                                     read from global memory the wavefront leaves the descent early, dev_intersect.hpp):
                                     same hit record, n_descend / n_return / n_leaf left 0.  With TRC_TRACE_ANY_HIT it
                                     is the order-free walk the render kernels give shadow rays: an any-hit query only
                                     asks WHETHER something lies in front of tmax, which does not depend on the order
                                     the tree is walked in, but which primitive is met first does -- only `hit` is
                                     defined then (pType -1, the other fields 0) */
trc_status trc_trace_rays(trc_ctx* ctx, const trc_ray* rays, size_t n, trc_hit* out, int any_hit);

trc_status trc_get_stats(trc_ctx* ctx, trc_stats* out);   /* synchronises the stream */
trc_status trc_reset_stats(trc_ctx* ctx);

/* ------------------------------------------------------------------ */
/* SVGF denoiser (tracer_amd/csrc/trc_denoise.hip)                     */
/* ------------------------------------------------------------------ */
/* The reference filters the SPPM running mean (sourceSVGF, Photon.metal:622) with MPSSVGFDenoiser before display
 * (AAPLRenderer.mm:818-850, :1027), guided by a depth / normal G-buffer its camera pass writes (Photon.metal:23-24,154).
 * MPS is closed; this is the published filter, Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017,
 * stated here exactly (tests/svgf_ref/svgf_ref.cpp restates it operation by operation; every operation is binary32,
 * no contraction, division and sqrt correctly rounded, exp = dm_expf of trc_detmath.h, sums in the order written).
 *
 * G-buffer, one texel per pixel: the ray of pixel (x, y) through the lens centre, u = x / W, v = y / H,
 *   d = normalize((cornerLowLeft + horizontal * u) + vertical * v - lookFrom)  (kernelCameraRecording, Photon.metal:132-139),
 * walked by the render kernels' production scene_hit.  depth = t (+inf on a miss), normal = HitRecord.sn (0 on a miss),
 * albedo = texture_value of the hit material (1 for emitters -- DiffuseLight -- and misses), id = material index
 * (TRC_GBUFFER_MISS on a miss).  Rebuilt by trc_denoise only when the scene, the camera or the frame size changed.
 *
 * Notation: L(c) = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b (trc_tonemap's weights); "hit" = id != TRC_GBUFFER_MISS;
 * w8(x) = x squared log2(normal_exponent) times; taps are visited row by row (dy outer, dx inner), in-bounds hit taps only.
 * Miss pixels pass the accumulator through unchanged, never enter a hit pixel's sums and take none (history 1).
 *
 * 1. Input c = accumulator rgb; with TRC_DENOISE_DEMODULATE c = c / max(albedo, TRC_DENOISE_ALBEDO_EPS) per channel.
 * 2. Temporal pass (one kernel with 3).  Previous camera = the camera of the last trc_denoise.  Same camera (lookFrom,
 *    horizontal, vertical, cornerLowLeft bitwise equal): the one tap (x, y) with weight 1, depth to compare zq = depth.
 *    Otherwise P = lookFrom + d * depth, q = P - lookFrom', a = cornerLowLeft' - lookFrom', m = cross(horizontal', vertical'),
 *    s = dot(a, m) / dot(q, m) (invalid unless s > 0 and finite), u' = (dot(q, h') * s - dot(a, h')) / dot(h', h'),
 *    v' = (dot(q, v') * s - dot(a, v')) / dot(v', v') (h' = horizontal', v' = vertical'), px = u' W, py = v' H, valid
 *    only for -1 < px < W, -1 < py < H; zq = length(q); taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), x0 = floor(px),
 *    fx = px - x0, weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  A tap is consistent when it is in bounds, its
 *    previous texel has the same id, |depth' - zq| <= 0.1 zq and dot(normal', normal) >= 0.9.  Over the consistent taps
 *    W = sum w, C = sum w colour', M1, M2, N likewise (history colour, moments, history length); the history is valid
 *    when W >= 0.01, and then prev = C / W etc.  n = valid ? min(N / W + 1, 64) : 1,
 *    a = valid ? max(1 / n, alpha_color) : 1, am = valid ? max(1 / n, alpha_moments) : 1,
 *    colour = valid ? prev + (c - prev) * a : c, mu1 = valid ? m1 + (L(c) - m1) * am : L(c) (m1 = M1 / W), mu2 likewise
 *    with L(c)^2 (the blends and the sums below are written as corrections of the centre value: a constant stays exact).
 * 3. Variance: n >= min_history: max(0, mu2 - mu1 * mu1).  Otherwise the 7x7 estimate around p over the demodulated
 *    input: w = dm_expf(-(|z - z'| / D)) * w8(max(0, dot(n, n'))), D = sigma_z * (gx |dx| + gy |dy|) + 0.001 z, sums
 *    W, S1 = sum w L', S2 = sum w L'^2, variance = max(0, S2 / W - (S1 / W)^2) (0 when W = 0).
 *    Depth gradient stencil: gx = min(|z(x+1) - z|, |z(x-1) - z|) over the horizontal neighbours that are in bounds and
 *    hit (0 when neither is), gy the same vertically -- one-sided across a depth step, so the step does not widen it.
 * 4. A-trous iteration i (0-based, step 2^i), on (colour, variance): first the 3x3 Gaussian of the variance around p,
 *    weights 0.25 centre, 0.125 edge, 0.0625 corner, vf = sum g var' / sum g; phi = sigma_l * sqrt(max(0, vf)) + 1e-10.
 *    Then the 5x5 taps q = p + step (dx, dy), h = {1/16, 1/4, 3/8, 1/4, 1/16}: w = ((h[dx] h[dy]) * wn) * dm_expf(-(wz + wl)),
 *    wn = w8(max(0, dot(n, n'))), wz = |z - z'| / D (D as in 3 with the offsets step dx, step dy), wl = |L - L'| / phi;
 *    W += w, C += w (colour' - colour), V += (w w) var'; result colour = colour + C / W, variance = V / (W W) (the
 *    input when W = 0).
 *    Iteration 0's output is the next frame's colour history (Schied et al. section 4.2).
 * 5. Output rgb = the last iteration's colour (the temporal colour for 0 iterations), times max(albedo, eps) when
 *    demodulated; alpha = the accumulator's.  History is dropped by trc_resize, trc_upload_scene*, trc_set_environment*,
 *    trc_upload_textures and trc_denoise_reset: the next frame has n = 1 everywhere.
 */
#define TRC_GBUFFER_MISS        0xFFFFFFFFu
#define TRC_DENOISE_DEMODULATE  1u          /* filter colour / albedo, remodulate at the end */
#define TRC_DENOISE_ALBEDO_EPS  0.001f
#define TRC_DENOISE_MAX_ITERATIONS 5u
typedef struct trc_gbuffer_texel {
    float    depth;                /* hit distance along the normalised camera ray, +inf on a miss */
    float    normal[3];            /* HitRecord.sn */
    float    albedo[3];            /* texture_value of the hit material; 1 for emitters and misses */
    uint32_t id;                   /* material index, TRC_GBUFFER_MISS on a miss */
} trc_gbuffer_texel;
typedef struct trc_denoise_params {
    uint32_t flags;                /* TRC_DENOISE_* */
    uint32_t iterations;           /* a-trous iterations, 0 .. 5 (5) */
    float    alpha_color;          /* (0, 1]: 0.1 (temporalReprojectionBlendFactor, AAPLRenderer.mm) */
    float    alpha_moments;        /* (0, 1]: 0.2 */
    float    sigma_z;              /* > 0: 1 */
    uint32_t normal_exponent;      /* power of two, 1 .. 1024: 128 */
    float    sigma_l;              /* > 0: 4 */
    uint32_t min_history;          /* 1 .. 64: 4 (below it the variance is the 7x7 estimate) */
} trc_denoise_params;
void       trc_denoise_default_params(trc_denoise_params* out);
/* Denoises the accumulator as it stands into the context's RGBA32F output; asynchronous on the context stream like
 * trc_render.  TRC_ERR_NO_FRAME without trc_resize, TRC_ERR_NO_SCENE without a scene (or camera), TRC_ERR_UNSUPPORTED on a
 * context in a group, TRC_ERR_INVALID_ARG on bad parameters.  Never touches the accumulator or the RNG texture. */
trc_status trc_denoise(trc_ctx* ctx, const trc_denoise_params* params);
trc_status trc_download_denoised(trc_ctx* ctx, float* rgba /* 4*W*H */);            /* TRC_ERR_NO_FRAME before a trc_denoise */
trc_status trc_tonemap_denoised(trc_ctx* ctx, uint8_t* rgba8, float* exposure_out);  /* trc_tonemap's output stage on it */
trc_status trc_download_gbuffer(trc_ctx* ctx, trc_gbuffer_texel* out /* W*H */);
trc_status trc_denoise_reset(trc_ctx* ctx);
/* Motion tracking: the history follows surfaces that move (opt-in; with it off every call is what it was).
 *
 * The calls that move a scene in place -- trc_update_vertices, trc_pose_vertices, trc_skin_vertices, trc_morph_vertices (they move
 * vertices), trc_update_primitives (it moves spheres, squares and cubes), trc_recompute_normals and trc_rebuild_tree (they move
 * nothing) -- drop the history like every other change of the picture:
 * the frame after one has n = 1 everywhere.  With tracking on these seven mark the G-buffer stale and KEEP the history, and the temporal
 * pass finds a moved surface point where it was.  Every other call that drops the history (step 5's list, trc_upload_triangle_materials,
 * trc_denoise_reset) drops it as before.
 *
 * State.  trc_denoise_track_motion(ctx, on) is a switch of the context like the textures: off at trc_create, kept across
 * trc_upload_scene* and trc_resize (the two buffers below are not: they go with the scene and the frame).  A call that changes the
 * switch, either way, drops the history; switching off frees both buffers; a call that leaves it as it is does nothing.
 * While on, the context holds 16 bytes per vertex and the device's records of the analytic primitives, at most 40 KB (the snapshot),
 * and 16 bytes per pixel (the motion plane) more, and nothing else.  All are allocated by trc_denoise (the vertex part when the scene
 * has vertices, the primitive part when it has primitives): TRC_ERR_OOM surfaces there, the moving calls gain no failure mode.
 *
 * Snapshot.  While tracking is on, the FIRST moving call after a trc_denoise -- one of the four vertex-moving calls or
 * trc_update_primitives -- copies, as they stand before that call changes anything, the position of every vertex of the scene (x, y, z
 * as one 16-byte record per vertex) and the device's record of every sphere, square and cube into the snapshot: ONE event for both
 * kinds of geometry, whichever kind the call moves.  Further moving calls before the next trc_denoise, of either kind, take no new
 * one.  The snapshot is in force for that next trc_denoise and no longer: it holds every vertex and every primitive where the previous
 * trc_denoise saw it.  (Before the first trc_denoise with tracking on there is no buffer and no history: nothing is copied.)
 *
 * Motion texel of pixel (x, y), written when trc_denoise rebuilds the G-buffer with a snapshot in force.  o = lookFrom and d are
 * the G-buffer ray above (d normalised).  Where the primary hit is triangle t: a, b, c = the current positions of the vertices
 * idxList[3t], idxList[3t + 1], idxList[3t + 2] and a', b', c' their snapshot positions;
 *   e1 = b - a, e2 = c - a, pvec = cross(d, e2), det = dot(e1, pvec), inv = 1 / det, tvec = o - a, u = dot(tvec, pvec) * inv,
 *   qvec = cross(tvec, e1), v = dot(d, qvec) * inv, w = (1 - u) - v          (Triangle::hit_test's barycentrics, Triangle.hh)
 *   prev = (u * b' + v * c') + w * a'                                        (HitRecord.p's expression over the snapshot)
 * componentwise, with dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z and cross(p, q) = (p.y q.z - p.z q.y, p.z q.x - p.x q.z,
 * p.x q.y - p.y q.x); every operation one binary32 operation in the order written, no contraction, the division correctly rounded.
 * moved = 1 when any of the nine coordinates of a, b, c compares unequal (!=) to its snapshot value, else 0.  A triangle hit whose
 * triangle did not move still gets prev, which then has the bits of HitRecord.p.
 * Where the primary hit is an analytic primitive: p = HitRecord.p of the G-buffer walk, primed values are the snapshot's record of
 * that primitive, unprimed the current one; every operation one binary32 operation in the order written, no contraction, the
 * divisions correctly rounded.
 *   sphere  moved = any of c.x, c.y, c.z, r compares != to its snapshot value (r as the record holds it)
 *           n = ((p.x - c.x) / r, (p.y - c.y) / r, (p.z - c.z) / r);  prev = (c'.x + n.x * r', c'.y + n.y * r', c'.z + n.z * r')
 *   square  moved = any of range_i.x, range_i.y, range_j.x, range_j.y, value_k compares !=, or one of the three axes differs
 *           a = p[axis_i], b = p[axis_j], fu = (a - i0) / (i1 - i0), fv = (b - j0) / (j1 - j0); prev = 0, then written in the order
 *           k', i', j' with the snapshot's axes: prev[k'] = value_k', prev[i'] = i0' + fu * (i1' - i0'), prev[j'] = j0' + fv * (j1' - j0')
 *   cube    moved = any of the 12 xyz entries of the model_matrix columns or of the inverse_matrix columns compares !=
 *           q = ((I0 * p.x + I1 * p.y) + I2 * p.z) + I3 with the current inverse columns (its object-space point),
 *           prev = ((M0' * q.x + M1' * q.y) + M2' * q.z) + M3' with the snapshot's model columns
 * An analytic winner with moved = 0 gets prev = 0.  Every other texel -- a miss, and every texel of a trc_denoise with no snapshot in
 * force -- is prev = 0, moved = 0.
 *
 * Step 2, amended.  A pixel with moved = 1 always takes the general rule, whatever the two cameras, with P = prev in place of
 * lookFrom + d * depth; the previous camera is the camera of the last trc_denoise.  Everything after P is step 2 unchanged: q, a, m,
 * s, u', v', px, py and their validity, zq = length(q), the four taps and weights, the id, depth and normal tests.  A pixel with
 * moved = 0 takes step 2 as it stands (the one tap under the same camera, P from the depth otherwise).  So with tracking on and
 * nothing moved every plane has the bits it has with tracking off.
 *
 * Not covered: a square that turns (it is axis-aligned: its axes may change, a rotation cannot be said); a surface that appears has no history, its pixels start at n = 1;
 * lighting that moves lags behind -- the shadow and the reflection of a moved object follow alpha_color, as in the paper; there
 * is no screen-space motion-vector output; contexts in a group (trc_denoise refuses them). */
typedef struct trc_motion_texel {
    float    prev[3];              /* where this pixel's surface point was when the last trc_denoise ran */
    uint32_t moved;                /* 1: a triangle hit whose triangle, or a sphere, square or cube hit whose record, changed since then; else 0 */
} trc_motion_texel;                /* 16 bytes */
/* TRC_ERR_INVALID_ARG on a NULL context */
trc_status trc_denoise_track_motion(trc_ctx* ctx, int on);
/* The plane the last trc_denoise used (all zero when it had no snapshot in force).  TRC_ERR_NO_FRAME before a trc_denoise with
 * tracking on and whenever tracking is off, TRC_ERR_INVALID_ARG on a NULL argument. */
trc_status trc_download_motion(trc_ctx* ctx, trc_motion_texel* out /* W*H */);
/* The history length n of step 2 as the last trc_denoise left it, one float per pixel (1 on a miss): what a host watches to see whether
 * the history survives its animation.  Tracking on or off.  TRC_ERR_NO_FRAME before a trc_denoise, TRC_ERR_INVALID_ARG on a NULL argument. */
trc_status trc_download_history_length(trc_ctx* ctx, float* n /* W*H */);
/* A denoiser that follows the rays: trc_denoise_guide_rays(ctx, on) (opt-in; with it off every call is what it was).
 *
 * The G-buffer above is walked along the camera's own pinhole ray.  Under camera-ray sets (TRC_FLAG_CAMERA_RAYS) of another projection --
 * orthographic, a panorama, a host's own lens -- that guides the filter with surfaces the pixel does not show.  With the switch on the
 * filter reads the rays instead.
 *
 * State.  A switch of the context like trc_denoise_track_motion: off at trc_create, kept across trc_upload_scene* and trc_resize.  A call
 * that changes it, either way, drops the history (and the G-buffer is rebuilt); a call that leaves it as it is does nothing.
 * TRC_ERR_INVALID_ARG on a NULL context.  With the switch on:
 *
 * 1. G-buffer ray.  The ray of pixel (x, y) is record y * W + x of set 0 of the rays in force (a host puts the set it wants the filter
 *    guided by first: with sub-pixel offsets the one nearest the pixel's centre, or a set at the zero offset).  The ray is made as trc_trace_rays makes one: the direction is
 *    normalised on entry, tmax and _pad are ignored.  depth = t along that normalised ray from the ray's own origin; normal, albedo and
 *    id are as stated above; the walk is the same production walk.  So every texel is what trc_trace_rays(..., TRC_TRACE_PRODUCTION)
 *    answers for the record: depth has the bits of t, normal of sn, id is material; a miss is (+inf, 0, 1, TRC_GBUFFER_MISS).
 * 2. When the G-buffer is rebuilt: when the scene, the frame size or the switch changed; when the rays in force were replaced -- the
 *    context counts generations: trc_upload_camera_rays, trc_generate_camera_rays, trc_clear_camera_rays and trc_resize each begin a new
 *    one; when a tracked moving call marked it stale.  NOT when the camera changed: the rays hold their own camera, so trc_set_camera
 *    neither rebuilds the G-buffer nor touches the history while the switch is on.
 * 3. Temporal pass (step 2 above).  A new generation of rays drops the history: n = 1 everywhere, even if the new rays have the old
 *    bits.  So whenever there is a history the rays are the ones it was made under, and every pixel with moved = 0 takes the one tap
 *    (x, y) with weight 1 and zq = depth.  A pixel with moved = 1 (tracking on, a snapshot in force) has NO valid history: n = 1, a = 1
 *    -- a ray set defines no inverse to reproject through.  Pixels that did not move keep their history.  Steps 1 and 3 to 5 unchanged.
 * 4. Motion texel (tracking on): o and d are the G-buffer ray of 1; everything else as stated under "Motion tracking".  Under the
 *    camera's own pinhole rays the plane has the bits it has with the switch off.
 * 5. trc_denoise with the switch on and no rays in force returns TRC_ERR_UNSUPPORTED: nothing changes, the history is kept.
 * 6. Limits: no reprojection under the switch -- a host that changes its rays per frame restarts the history at every frame; the SPPM
 *    camera pass still uses the camera; contexts in a group are refused, as without the switch.
 * With the camera's own rays as set 0 (TRC_RAYS_PINHOLE, no offset, a camera that has not changed since), every plane has the bits it has
 * with the switch off.  trc_download_gbuffer, trc_download_motion and trc_download_history_length answer as before. */
trc_status trc_denoise_guide_rays(trc_ctx* ctx, int on);
/* ------------------------------------------------------------------ */
/* Tile mask, per-tile error estimate, adaptive sampling (tracer_amd/csrc/trc_adaptive.hip) */
/* ------------------------------------------------------------------ */
/* Tiles are the TRC_TILE x TRC_TILE pixel tiles of the frame, row-major from pixel row 0: tile t = (y / TRC_TILE) * ceil(W / TRC_TILE) +
 * x / TRC_TILE holds pixel (x, y) of the accumulator; there are ceil(W / TRC_TILE) * ceil(H / TRC_TILE) of them, the last column and row
 * partial when W or H is no multiple of TRC_TILE.
 *
 * trc_set_tile_mask: one byte per tile.  With a mask set, trc_render renders the pixel blocks of the tiles that are owned (tile_rank /
 * tile_nranks, as without a mask) AND have a non-zero byte; the accumulator and RNG texels of every other pixel are neither read nor written.
 * A pixel's samples are one chain through its own RNG texel and the running mean takes its weight from frame0 + s, so the pixels that ARE
 * rendered get exactly the bits of a launch over the whole frame; trc_stats counts the paths and rays of the rendered pixels.  The mask holds
 * for every launch shape (8x8 and 4x4 blocks, strips, persistent workgroups, the dense kernel, stacked views, TRC_FLAG_COLLECT_STATS).  A mask
 * with no tile set is legal: trc_render then launches nothing.  mask == NULL: every tile again (n_tiles is ignored).  trc_resize drops the
 * mask.  trc_sppm_* ignore it.  TRC_ERR_INVALID_ARG: n_tiles is not the frame's tile count; TRC_ERR_NO_FRAME before trc_resize;
 * TRC_ERR_UNSUPPORTED on a context in a group (trc_group_init / trc_group_set_collectives): a composed frame needs every rank's whole
 * share.  A refused call changes nothing.
 * Block costs: a mask that only clears tiles of the mask before it keeps what the context knows about the surviving blocks (each block's cost
 * as one block; the split plan starts over), so the next launch is ordered by them and runs as one pass; a mask that sets a tile again starts
 * a new block list, whose first launch measures afresh (trc_render's head).  Knob "mask_forgets_costs": every mask change does.  Pixels depend
 * on neither.
 * trc_download_tile_mask: the mask in force, 1 / 0 per tile (all 1 without a mask). */
trc_status trc_set_tile_mask(trc_ctx* ctx, const uint8_t* mask, uint32_t n_tiles);
trc_status trc_download_tile_mask(trc_ctx* ctx, uint8_t* out /* n tiles */);

/* Per-tile error estimate, after Dammertz, Hanika, Keller, Lensch: "A hierarchical automatic stopping condition for Monte Carlo global
 * illumination" (WSCG 2010).  The paper compares the image I of all samples with the image A of every second sample; here A is the
 * accumulator as it was after the FIRST half of every pixel's chain (trc_tile_snapshot) and I the accumulator now.  With A taken at half the
 * samples and B the mean of the second half, I = (A + B) / 2 and |I - A| = |B - A| / 2, as there.  There is no area factor.
 *
 * Per in-bounds pixel of tile t (N_t of them: 256, fewer in a partial tile), every operation in binary32, rounded to nearest, no contraction,
 * division and square root correctly rounded:
 *     d   = (|I.r - A.r| + |I.g - A.g|) + |I.b - A.b|
 *     s   = (I.r + I.g) + I.b;    s' = s > TRC_ADAPTIVE_EPS ? s : TRC_ADAPTIVE_EPS        (a NaN s takes the eps)
 *     e   = d / sqrt(s');         e' = e < 65535 ? e : 65535                              (a NaN or infinite e takes the cap)
 *     q   = (uint32_t)(e' * 65536)                                                        (truncation; e' * 65536 < 2^32)
 *     E_t = (float)((double)(sum of q over the tile's pixels, as uint64_t) / ((double)N_t * 65536.0))
 * The sum is one of integers, so E_t does not depend on the order of summation (trc_tonemap's mean is made the same way).
 * libtracer_amd_fast.so computes the same steps under its own rules for division, square root and denormals.
 *
 * trc_tile_snapshot: A := the accumulator, the whole plane (16 B per pixel, allocated by the first call, freed by trc_resize).
 * trc_tile_error: E_t of every tile of the mask in force (every tile without one) from I = the accumulator as it stands and A; the other
 * tiles keep the E_t they had (0 until a tile's first estimate).  snapshot_after != 0: A := I for the pixels of those tiles in the same pass
 * over the planes, ready for the next round.  TRC_ERR_NO_FRAME before trc_resize or before the first trc_tile_snapshot.
 * trc_download_tile_error: E_t of every tile.  All three: TRC_ERR_UNSUPPORTED on a context in a group. */
#define TRC_ADAPTIVE_EPS 1e-4f
trc_status trc_tile_snapshot(trc_ctx* ctx);
trc_status trc_tile_error(trc_ctx* ctx, int snapshot_after);
trc_status trc_download_tile_error(trc_ctx* ctx, float* e /* n tiles */);

/* trc_render_adaptive: a picture from sample 0 that stops sampling the tiles whose estimate has fallen to `threshold`.
 *   p->spp = h0, at least 8: the first pass, over every tile.  p->frame0 must be 0 (the call starts a picture; continuing one is not supported).
 *   a->max_spp >= 2 * h0: no pixel gets more samples.  a->threshold: finite and > 0.  a->reserved: 0.
 * The loop, with n the samples every active tile has and the mask M = every tile (whatever mask the host has set; that one is back in force
 * when the call returns, also when it fails):
 *   1. one pass of h0 samples, frame0 = 0; A := accumulator; n = h0
 *   2. one pass of m = min(n, max_spp - n) samples, frame0 = n, over the tiles of M; n += m          (n doubles; the last pass lands on max_spp)
 *   3. trc_tile_error(snapshot_after = 1) over M
 *   4. every tile of M with E_t <= threshold leaves M for good; n_t = n for every tile that was in M at step 2
 *   5. back to 2 unless n == max_spp or M is empty
 * Every pass is an ordinary trc_render pass of the production kernels (never kept for coalescing), so a tile's pixels hold exactly the bits
 * of a plain trc_render of n_t samples.  The check is made after the last pass too: E_t, active_tiles and max_error describe the picture as
 * returned.  TRC_ERR_INVALID_ARG: a NULL argument, frame0 != 0, spp < 8, max_spp < 2 * spp, a threshold that is not finite or not > 0;
 * TRC_ERR_UNSUPPORTED on a context in a group; otherwise what trc_render returns (no scene, no frame, no camera ...).  A refused call
 * leaves accumulator, RNG and mask as they were.
 * KNOWN LIMIT.  Stopping is permanent and decided from the samples themselves, so the result is slightly biased, as in the paper.  A tile
 * whose samples so far are all black has E_t = 0 and stops at the first check: under tracePath, whose paths find the light by chance, small
 * frames have such tiles at n = 16, and fireflies make its estimate GROW from n = 16 to 64, where traceMIS's falls.  Choose a first pass
 * long enough for the integrator (traceMIS: 8 to 16; tracePath: 64 or more), and prefer traceMIS.
 * trc_adaptive_default_params: max_spp = 256, threshold = TRC_ADAPTIVE_DEFAULT_THRESHOLD. */
typedef struct trc_adaptive_params { float threshold; uint32_t max_spp; uint32_t reserved[2]; } trc_adaptive_params;
typedef struct trc_adaptive_report {
    uint32_t passes;          /* render passes: 1 + the rounds of steps 2 .. 4 */
    uint32_t active_tiles;    /* tiles still in M after the last check */
    uint64_t samples;         /* sum over tiles of N_t * n_t: what trc_stats.paths grew by */
    float    max_error;       /* the largest E_t of the frame after the last check */
    uint32_t _pad;
} trc_adaptive_report;
/* the median E_t of BASELINE config 2 (Cornell box + 12 spheres) under traceMIS at 1920 x 1080, n = 64 with A at 32, as tools/adaptive_bench.py
 * measures it (profiles/r28/adaptive_sampling.txt, step 0: 0.05253): half of that frame's tiles have settled by then */
#define TRC_ADAPTIVE_DEFAULT_THRESHOLD 0.0525f
void       trc_adaptive_default_params(trc_adaptive_params* out);
trc_status trc_render_adaptive(trc_ctx* ctx, const trc_params* p, const trc_adaptive_params* a, trc_adaptive_report* out /* may be NULL */);
/* n_t of the last trc_render_adaptive, one per tile (TRC_ERR_NO_FRAME before one) */
trc_status trc_download_tile_samples(trc_ctx* ctx, uint32_t* n /* n tiles */);

/* ------------------------------------------------------------------ */
/* Camera-ray sets (TRC_FLAG_CAMERA_RAYS; tracer_amd/csrc/trc_camera_rays.hip, trc_render_rays.hpp) */
/* ------------------------------------------------------------------ */
/* A context may hold n_sets >= 1 camera-ray sets, each W x H trc_ray records of 32 bytes (tmax and _pad ignored), set-major, then
 * row-major like the accumulator: pixel (x, y) of set k is record (k * H + y) * W + x.  66 MB per set at 1920 x 1080.  The sets belong to
 * the frame size: trc_resize drops them; trc_upload_scene* and trc_set_camera do not (generated rays keep the camera they were made from).
 * What a render does with them: TRC_FLAG_CAMERA_RAYS above.
 *
 * trc_upload_camera_rays: the host's own rays, any lens, any projection: n_sets * W * H records.
 * trc_generate_camera_rays: built on the device from the context's camera as it stands (include/trc_raygen.h states the arithmetic once, for
 * the device and for trc_host_generate_camera_rays).  binary32, one rounding per operation in the order written, no contraction, divisions
 * correctly rounded.  For pixel (x, y) of set k with offset (dx, dy) = offsets[2 k], offsets[2 k + 1] (0, 0 when offsets == NULL):
 *     s = ((float)x + dx) / (float)W;    t = ((float)y + dy) / (float)H
 *     P(s, t) = (cornerLowLeft + horizontal * s) + vertical * t                                  per component
 *   TRC_RAYS_PINHOLE       origin = lookFrom;  direction = P(s, t) - lookFrom   (not normalised).  With zero offsets this is castRay's ray at
 *                          lens radius 0, because (float)x + 0.0f is (float)x
 *   TRC_RAYS_ORTHOGRAPHIC  origin = lookFrom + (P(s, t) - P(0.5f, 0.5f));  direction = P(0.5f, 0.5f) - lookFrom
 *   TRC_RAYS_EQUIRECT      origin = lookFrom;  phi = 6.2831855f * (s - 0.5f), lat = 3.1415927f * (t - 0.5f),
 *                          direction = (cos lat * cos phi, sin lat, cos lat * sin phi) with dm_sinf / dm_cosf of trc_detmath.h: the
 *                          parametrisation TRC_FLAG_ENV_LIGHT states for the map -- world axes, the camera's orientation is ignored
 *   written: tmax = FLT_MAX, _pad = 0.
 * Offsets are per set, not per pixel.  libtracer_amd_fast.so generates under its own rules (contraction, hardware sine and cosine): its rays
 * are not bit-equal to the host's; the parity statements here and under TRC_FLAG_CAMERA_RAYS are about the exact build.
 * trc_download_camera_rays: the W * H records of one set.  trc_clear_camera_rays: no rays in force.
 *
 * Errors.  TRC_ERR_NO_FRAME before trc_resize (trc_download_camera_rays: also with no rays in force); TRC_ERR_INVALID_ARG: a NULL argument,
 * n_sets outside 1 .. TRC_MAX_RAY_SETS, an unknown model, an offset outside [0, 1) or not finite, a set that is not below n_sets,
 * trc_generate_camera_rays before trc_set_camera.  TRC_ERR_OOM leaves the previous rays in force.  A refused call changes nothing. */
#define TRC_MAX_RAY_SETS 1024u
enum trc_ray_model { TRC_RAYS_PINHOLE = 0, TRC_RAYS_ORTHOGRAPHIC = 1, TRC_RAYS_EQUIRECT = 2 };
typedef struct trc_ray_gen {
    uint32_t model;          /* enum trc_ray_model */
    uint32_t n_sets;         /* 1 .. TRC_MAX_RAY_SETS */
    const float* offsets;    /* 2 * n_sets sub-pixel offsets (dx, dy), each in [0, 1); NULL = all zero */
} trc_ray_gen;
trc_status trc_upload_camera_rays(trc_ctx* ctx, const trc_ray* rays, uint32_t n_sets);
trc_status trc_generate_camera_rays(trc_ctx* ctx, const trc_ray_gen* g);
trc_status trc_download_camera_rays(trc_ctx* ctx, uint32_t set, trc_ray* out /* W*H */);
trc_status trc_clear_camera_rays(trc_ctx* ctx);

/* ------------------------------------------------------------------ */
/* Material parameters (TRC_FLAG_MATERIAL_PARAMS; tracer_amd/csrc/trc_material_params.hip, trc_render_params.hpp) */
/* ------------------------------------------------------------------ */
/* One record per material of the scene, in the order of trc_scene_view.materials.  The table belongs to the context and to the scene it
 * was uploaded for: every trc_upload_scene* drops it; trc_update_vertices and the other animation calls, trc_rebuild_tree,
 * trc_set_triangle_visibility, trc_upload_triangle_materials, trc_upload_textures and trc_resize keep it.  The scene blob does not change.
 * What a render does with it: TRC_FLAG_MATERIAL_PARAMS above.  Fields a material's type does not use are validated and never read.
 *
 * trc_upload_material_params(ctx, p, n_material): n_material must be the scene's; (NULL, 0) leaves no table in force.
 * trc_download_material_params: what was uploaded (TRC_ERR_INVALID_ARG with no table in force or another n_material).
 * Errors.  TRC_ERR_NO_SCENE before a scene upload; TRC_ERR_INVALID_ARG, nothing changed: n_material not the scene's, a field that is not
 * finite, alpha_x or alpha_y <= 0, eta <= 1, a component of metal_eta or metal_k <= 0, a non-NULL table with n_material 0 or the
 * reverse.  TRC_ERR_OOM leaves the previous table in force. */
typedef struct trc_material_params {      /* 48 bytes, three float4 */
    float alpha_x, alpha_y;   /* roughness pair of the material's microfacet distribution; each used as max(0.001f, a), as the
                                 reference's constructors clamp (MicrofacetBXDF.h:164, 306-309) */
    float eta;                /* dielectric index: Plastic's and Glass's reflection Fresnel term, Glass's etaB */
    float _pad0;
    float metal_eta[3]; float _pad1;      /* Metal: FresnelConductor's eta ... */
    float metal_k[3];   float _pad2;      /* ... and k */
} trc_material_params;
trc_status trc_upload_material_params(trc_ctx* ctx, const trc_material_params* p, uint32_t n_material);
trc_status trc_download_material_params(trc_ctx* ctx, trc_material_params* out, uint32_t n_material);

/* developer diagnostic: the pixel blocks of the last trc_render (x | y << 16, in units of the block edge 1 << *blk_shift)
 * and the duration each one's wavefront measured per sample (shader clocks / (4 spp) -- the sort key of the adaptive launch order); with
 * strips (spp < 8) the costs are per strip; a block that ran in parts (four 4x4 quarters, some of them as four 2x2
 * sixteenths, some of those as four single pixels) reports its slowest part with bit 31 set, bit 30 when it had sixteenths and bit 29 when it
 * had single pixels.  Any pointer may be NULL; at most `capacity` entries are written. */
trc_status trc_debug_block_costs(trc_ctx* ctx, uint32_t* tiles, uint32_t* costs, uint32_t capacity, uint32_t* n_blocks, uint32_t* blk_shift);
/* developer diagnostic: the two lower bounds of the last trc_render's kernel time that no schedule can beat.  A pixel's samples
 * are one chain through its RNG texel (Render.metal:545-557), so a launch lasts at least as long as its slowest wavefront-sized
 * item (a whole 8x8 block, or a 4x4 / 2x2 / single-pixel part of one) -- the bound a strong-scaled share of a frame runs into -- and at least
 * the items' summed durations over the wavefront slots of the GPU.  Durations are the wavefronts' own measurements (shader
 * clocks), converted with the device's nominal shader clock. */
typedef struct trc_launch_shape {
    uint32_t entries;             /* wavefront-sized items of the launch: whole blocks + parts */
    uint32_t wave_slots;          /* wavefronts the GPU holds at once for the kernel that ran */
    double   longest_entry_ms;    /* the slowest item */
    double   sum_entries_ms;      /* all items: slot time */
    double   work_over_slots_ms;  /* sum_entries_ms / wave_slots */
    double   clock_mhz;           /* hipDeviceAttributeClockRate, used for the conversion */
} trc_launch_shape;
trc_status trc_debug_launch_shape(trc_ctx* ctx, trc_launch_shape* out);
/* Camera rays that were answered from the memo of the pixel's first walk instead of being walked, since the last trc_reset_stats.
 * The reference's camera has no sub-pixel jitter, and with aperture 0 every sample of a pixel casts the same ray: k_render_dense
 * and the persistent-workgroup tracePath kernels keep the first hit per pixel and launch, and replay it for every later sample
 * whose origin has the same bits (never across launches; a lens, TRC_FLAG_SOBOL, TRC_FLAG_COLLECT_STATS, traceMIS / traceVolume and launches of fewer than 8
 * samples always walk).  Included in trc_stats.rays.  Knob "no_primary_replay" (trc_debug_set) makes every camera ray walk. */
trc_status trc_debug_primary_replays(trc_ctx* ctx, uint64_t* out);

/* device info for the bench line */
trc_status trc_device_info(trc_ctx* ctx, char* name, size_t name_len, int* cu_count, size_t* hbm_bytes);
/* which physical GPU this context sits on: "domain:bus:device.function" (hipDeviceGetPCIBusId).  Ranks exchange it to learn
 * whether they hold DIFFERENT devices (then RCCL composes) or share one (RCCL refuses a second rank on a device: the
 * collectives table composes) -- counting HIP_VISIBLE_DEVICES entries cannot tell, a launcher may give every rank its own */
trc_status trc_device_pci_bus_id(trc_ctx* ctx, char* out, size_t out_len);

/* --- SPPM pass (RT_Metal/Metal/Photon.metal, host sequencing AAPLRenderer.mm:860-1086) ------------
 * Uses the scene / camera / frame (canvas RNG + accumulator) of the context. */
/* allocates the 512x512 photon records, photon RNG texture (seeded like trc_seed), per-pixel camera
 * records and the hash grids; resets Complex (frame_count = 0, totalPhotonSum = 0) */
trc_status trc_sppm_init(trc_ctx* ctx, uint64_t photon_seed);
/* n_frames x `photon:` (AAPLRenderer.mm:1077-1086): frame 0 runs photonPrepare (camera records, their
 * bounding box, hash scale, initial radius), every frame photonWork (odd frames re-run the camera pass,
 * photon bounce, hashing, mark/count grid, photon sum, progressive refine into the accumulator).
 * In a group (trc_group_init / trc_group_set_collectives) EVERY rank calls it: rank r traces and refines the pixels of its tiles and
 * bounces its share of the 512*512 photons (whole wavefronts of 64, the last non-empty share shorter when the ranks do not divide them;
 * at most 64 ranks), the bound of the visible points
 * is all-reduced and the photon records all-gathered each frame; a rank that owns no tile of a small frame still takes part.
 * Two corners are fixed as the reference's arithmetic has them: a frame in which no pixel records a visible point ends with the
 * bound {FLT_MAX, -FLT_MAX}, i.e. radius -inf and hash scale -0 (Photon.metal:157-161,357-372); a photon whose BSDF sample is NaN
 * counts the NaN as positive where copysign(1, wi.z) picks the side of the surface, and its stored direction / flux NaNs are the
 * canonical 0x7FC00000 (the sign of a NaN is the platform's: DESIGN.md 2). */
trc_status trc_sppm_frames(trc_ctx* ctx, uint32_t n_frames);
/* any pointer may be NULL.  mark: 4 floats per cell as texturePhotonMark (x, y of the winning photon,
 * cell x, y; -1 when empty), count: 1 float per cell as texturePhotonCount.
 * With a communicator / collectives table and photon_records != NULL the call is COLLECTIVE (every rank makes it): the
 * per-frame exchange moves only the 40 bytes of a photon the hash / table / refine passes read, the whole 80-byte records
 * of the other ranks' photons are all-gathered here, on demand. */
trc_status trc_sppm_download(trc_ctx* ctx, trc_CameraRecord* camera_records /* W*H */,
                             trc_PhotonRecord* photon_records /* 512*512 */, float* mark /* 512*512*4 */,
                             float* count /* 512*512 */, trc_Complex* complex);

/* --- multi-GPU: pixel tiles sharded over ranks, one RCCL reduce -------- */
#define TRC_UNIQUE_ID_BYTES 128
/* rank 0 creates the id, every rank gets the same bytes out-of-band */
trc_status trc_group_unique_id(uint8_t id[TRC_UNIQUE_ID_BYTES]);
trc_status trc_group_init(trc_ctx* ctx, const uint8_t id[TRC_UNIQUE_ID_BYTES], int nranks, int rank);
/* ncclReduce(sum) of the full-frame accum buffer to `root` on the ctx stream:
 * every rank holds zeros outside its own tiles, so sum == gather */
trc_status trc_group_reduce_accum(trc_ctx* ctx, int root);
/* --- sample sharding: the split that scales (SURVEY 8e "alternative") -------------------------------------------
 * A pixel's samples are ONE chain through its RNG texel (Render.metal:511-519,545-557), so a rank that owns a share of
 * the TILES still runs every owned pixel's whole chain: its launch ends on its slowest 8x8 block however few blocks it
 * owns.  Splitting the SAMPLES shortens the chains instead.  Definition (bit-level; oracle/pyoracle.py::render_sample_sharded
 * restates it and the GPU tests hold the composed frame to it bit for bit):
 *   - the nranks ranks are S sample groups x T tile ranks, nranks == S * T; rank r is tile rank r % T of group g = r / T;
 *   - group g renders the WHOLE frame (its T ranks share the tiles as usual: trc_params.tile_rank = r % T, tile_nranks = T,
 *     zeros elsewhere) with spp / S samples per pixel, frame0 counting from 0 within the group, from the RNG texture
 *     trc_seed(trc_shard_seed(seed, g)) -- group 0 keeps the seed, so S == 1 is the unsharded frame;
 *   - composed pixel = (((A_0 + A_1) + A_2) + ... + A_{nranks-1}) / (float)S per channel in binary32, A_r = rank r's
 *     accumulator texel: a rank-ORDERED sum (zeros of the other tile ranks are exact identities), one IEEE division.
 * Every group must have rendered the same number of samples (the mean of running means is the running mean only then).
 * Defined for the PCG sampler: under TRC_FLAG_SOBOL a sample's Sobol' point is a function of (frame, pixel) alone, so groups that all
 * count their frames from 0 draw the SAME points and differ only in the PCG draws (light pick, Russian roulette) -- legal, bit-defined
 * the same way, and statistically worth little more than one group.
 * How it moves: each rank owns the r-th of nranks equal pixel slices; an all-to-all brings that slice of every rank's
 * accumulator (ncclSend / ncclRecv in one group call; at N = 8 and 1080p 29 MB in and out per rank, every pair on its own
 * xGMI link), a small kernel folds them in rank order, and a gather (root >= 0) brings the N slices (4 MB each) to the
 * root.  The ranks' accumulators are left untouched -- a progressive host goes on rendering and composes again. */
uint64_t   trc_shard_seed(uint64_t seed, uint32_t sample_group);   /* seed + sample_group * 0x9E3779B97F4A7C15 (mod 2^64) */
/* on the context stream; the composed frame is read with trc_download_composed (root only).  sample_groups == 0: nranks
 * (every rank its own group, no tile split) */
trc_status trc_group_compose_samples(trc_ctx* ctx, int root, uint32_t sample_groups);
/* pipelined: the exchange runs on the communication stream once the work queued so far has finished, on a SNAPSHOT of the
 * accumulator taken in render-stream order (a device copy of the frame, ~20 us at 1080p) -- the compose only reads, so unlike
 * trc_group_reduce_accum_async the context keeps its accumulator: the next trc_render overlaps with the exchange AND may go on
 * accumulating (frame0 continuing); a progressive host calls this after every trc_render and never clears.
 * trc_download_composed (root) waits for the exchange */
trc_status trc_group_compose_samples_async(trc_ctx* ctx, int root, uint32_t sample_groups);
/* the same compose with sample_groups = nranks, delivered into EVERY rank's accumulator (all-gather instead of the gather).
 * Until ABI 4 this was ncclAllReduce(sum) / nranks, whose sum order is the ring's; it is the rank-ordered sum now. */
trc_status trc_group_allreduce_mean_accum(trc_ctx* ctx);
/* same compose, pipelined: the reduce runs on a second stream as soon as the work queued so far has finished,
 * and the context switches to its OTHER accumulator (allocated on first use, zero-filled), so the next
 * trc_clear_accum / trc_render overlap with the collective.  The composed frame of the call is read with
 * trc_download_composed (root only); trc_synchronize waits for the collectives too. */
trc_status trc_group_reduce_accum_async(trc_ctx* ctx, int root);
trc_status trc_download_composed(trc_ctx* ctx, float* rgba /* 4*W*H */);
trc_status trc_group_finalize(trc_ctx* ctx);

/* The collectives behind every trc_group_* / grouped trc_sppm_frames call, as a table.  RCCL (trc_group_init) is the
 * default; a host that has its own transport -- MPI, a socket mesh, gloo in the Python harness -- or that runs several
 * ranks on ONE GPU (where RCCL refuses a second rank on a device) installs its own with trc_group_set_collectives and
 * needs no communicator.  The program of collectives is the same either way:
 *   compose          reduce(sum, f32, 4*W*H) of the accumulator to the root           (trc_group_reduce_accum[_async])
 *   sample sharding  alltoall of the accumulator's nranks pixel slices, then gather of the composed slices to the root
 *                    (or allgather to every rank)            (trc_group_compose_samples[_async], trc_group_allreduce_mean_accum)
 *   SPPM frame 0     allreduce(min, u32, 3) + allreduce(max, u32, 3) of the bound keys (Photon.metal:169-218's reduction)
 *   SPPM every frame allgather of the photon records, 512*512/N * 80 bytes per rank    (so that kernelPhotonSumming,
 *                    Photon.metal:458-496, sees every photon on every rank)
 * Every function works IN PLACE on `buf`, is called by all ranks in the same order, returns 0 on success, and must
 * be complete (result visible to work queued later on `stream`) in stream order:
 *   host_staged = 0: `buf` is DEVICE memory and `stream` the hipStream_t the surrounding work is queued on (enqueue
 *                    on it, or synchronise it);
 *   host_staged = 1: the library waits for the stream, copies the buffer into pinned HOST memory, calls the function
 *                    with that host pointer (stream = NULL; it may block), and copies the result back -- slow,
 *                    meant for tests, 1-GPU plumbing runs and hosts without a GPU-aware transport.
 * reduce: the result is defined on `root` only.  allgather: rank r's contribution sits at buf + r * bytes_per_rank on
 * entry, all of them on return.  alltoall: `buf` holds nranks slices of bytes_per_rank; on return slice p holds what rank
 * p had in ITS slice r (r = the caller's rank; slice r stays).  gather: like allgather, the result is defined on `root`
 * only.  alltoall / gather may be NULL in a table whose host never composes sample shards (TRC_ERR_UNSUPPORTED then).
 * dtype / op use ncclDataType_t / ncclRedOp_t ordinals. */
enum trc_coll_dtype { TRC_DT_U8 = 1, TRC_DT_U32 = 3, TRC_DT_F32 = 7 };
enum trc_coll_op { TRC_OP_SUM = 0, TRC_OP_MAX = 2, TRC_OP_MIN = 3 };
typedef struct trc_collectives {
    void* user;
    int32_t host_staged;
    int32_t _pad;
    int (*reduce)(void* user, void* buf, size_t count, int dtype, int op, int root, void* stream);
    int (*allreduce)(void* user, void* buf, size_t count, int dtype, int op, void* stream);
    int (*allgather)(void* user, void* buf, size_t bytes_per_rank, void* stream);
    int (*alltoall)(void* user, void* buf, size_t bytes_per_rank, void* stream);
    int (*gather)(void* user, void* buf, size_t bytes_per_rank, int root, void* stream);
} trc_collectives;
/* installs `table` (copied) and makes the context rank `rank` of `nranks`; replaces a communicator made by
 * trc_group_init.  trc_group_finalize removes it.  table == NULL: same as trc_group_finalize. */
trc_status trc_group_set_collectives(trc_ctx* ctx, const trc_collectives* table, int nranks, int rank);

/* A/B and test knobs of ONE context (the defaults come from the environment variables of the same upper-case names at
 * trc_create): "no_lds_fit", "stack_lds_levels", "strip_len", "no_pwg", "sppm_serial_camera" (tools/README.md), and
 * "no_split" (no cost-adaptive block size), "no_cost_filter" (launch order and plan from the last launch's durations instead of
 * the shortest seen lately), "force_blk_shift" (k + 1 forces 2^k x 2^k pixel blocks per wavefront, k = 0..3: measurement only), and
 * "sppm_timing" (event pairs around an SPPM frame's photon pass and its hash / table / refine passes, added to
 * trc_stats.kernel_ms; one `launch` per frame), "descend_min" (n > 0: on trees read from memory the box-step loop of a wavefront goes on
 * while at least n lanes are still descending and others wait with a leaf; 0 = the scene's own value, 12, or 6 beyond 256 MiB), "camera_policy" (what trc_set_camera does with the recorded block costs: 0 = keeps them when the camera moved a little -- the view turned by
 * at most 5 degrees and the eye moved by at most 5 % of the scene's diagonal: the next launch is one pass ordered by the last launch's raw durations -- and forgets them
 * otherwise -- the next launch runs as a head + the rest; 1 always forgets, 2 always keeps the filtered costs, 3 always keeps and takes the raw durations: tools/moving_camera.py),
 * "no_primary_replay" (every camera ray is walked: trc_debug_primary_replays), "replay_min_lanes" / "replay_chain" (measurement only: a trip of
 * the render loop shades replayed hits alone where at least n lanes of the wavefront hold one, at most m such trips between two walks; 0 = the
 * defaults, 1 and 1; 65 lanes = never), "strip_force" (tests only: n > 0 gives every wavefront a strip of exactly n blocks, at any spp and whatever
 * the size of the frame -- "strip_len" asks for a length and is capped so that the GPU keeps 1.5 workgroups per wavefront slot, which on a
 * frame of a few blocks always leaves 1), "refit_single" (trc_update_vertices, trc_update_primitives), "skin_no_lds" (trc_skin_vertices), "mask_forgets_costs" (trc_set_tile_mask).  They change scheduling / bookkeeping only, never a pixel.  Unknown name: TRC_ERR_INVALID_ARG. */
trc_status trc_debug_set(trc_ctx* ctx, const char* knob, int value);

/* ------------------------------------------------------------------ */
/* host path: libtrc_host.so (CPU only)                                */
/* ------------------------------------------------------------------ */

/* BVH::buildNode, RT_Metal/Metal/BVH.hh:273-314: world AABB of the 8 corners
 * of `box` under model_matrix -> one leaf record */
void trc_host_build_node(const trc_AABB* box, const trc_float4x4* model_matrix,
                         int32_t pType, uint32_t pIndex, trc_BVH* out_leaf);
/* The reference's primitive constructors (Tracer.mm:127-172), as the scene builders of this library use them: what a C host fills the
 * records of trc_update_primitives with.  make_sphere: radius + 1e-4 in the record, boundingBOX = center -+ radius (not inflated),
 * identity model_matrix.  make_square: boundingBOX padded by 1 / 512 along axis_k, identity model_matrix.  make_cube: the unit box
 * under model_matrix, inverse_matrix by Gauss-Jordan in double rounded once, normal_matrix its transpose.  Everything else zero. */
void trc_host_make_sphere(trc_Sphere* out, float radius, const float center[3], uint32_t material);
void trc_host_make_square(trc_Square* out, uint8_t axis_i, float i0, float i1, uint8_t axis_j, float j0, float j1,
                          uint8_t axis_k, float k, uint32_t material);
void trc_host_make_cube(trc_Cube* out, uint32_t material, const trc_float4x4* model_matrix);
/* BVH::buildTree + BVH::make, BVH.hh:35-269: 10-bucket SAH over the n_leaves
 * leaf records at nodes[0..n_leaves); writes 2*n_leaves-1 nodes (root moved to
 * index 0); `nodes` must have room for 2*n_leaves-1.  Serial post-order
 * interior numbering (one legal schedule of the reference's GCD build). */
trc_status trc_host_build_tree(trc_BVH* nodes, uint32_t n_leaves, uint32_t* out_n_nodes);
/* flags == TRC_TREE_SAH: trc_host_build_tree itself.  flags == (TRC_TREE_SAH | TRC_TREE_SAH3): the same call with the split of
 * TRC_TREE_SAH3 (above, at trc_upload_scene_device) -- the tree the device builds under that flag, for a host that uploads its own
 * tree with trc_upload_scene.  Any other flags: TRC_ERR_INVALID_ARG, `nodes` untouched. */
trc_status trc_host_build_tree_flags(trc_BVH* nodes, uint32_t n_leaves, uint32_t flags, uint32_t* out_n_nodes);
/* depth of the deepest leaf (root = 0); TRC_ERR_BVH_INVALID on malformed trees */
trc_status trc_host_tree_depth(const trc_BVH* nodes, uint32_t n_nodes, uint32_t* out_depth);

/* MakeCamera / prepareCamera defaults, Tracer.mm:87-125,371-411 */
void trc_host_make_camera(trc_Camera* out, const float lookFrom[3], const float lookAt[3],
                          const float viewUp[3], float aperture, float aspect,
                          float vfov_radians, float focus_dist);
void trc_host_prepare_camera(trc_Camera* out, float width, float height);

/* deterministic fillRNG stand-in (see trc_seed) */
void trc_host_fill_rng(uint64_t seed, uint32_t width, uint32_t height, uint32_t* rgba);

/* The definition of trc_generate_camera_rays ("Camera-ray sets" above): g->n_sets * W * H records, set-major then row-major, bit for bit what
 * the exact build of the device library makes from the same camera.  Reads lookFrom, horizontal, vertical and cornerLowLeft of the camera.
 * TRC_ERR_INVALID_ARG as there, and for W == 0 or H == 0. */
trc_status trc_host_generate_camera_rays(const trc_Camera* camera, uint32_t W, uint32_t H, const trc_ray_gen* g, trc_ray* out);
/* n sub-pixel offsets for trc_ray_gen.offsets: offset k = (radical inverse base 2, radical inverse base 3) of k + 1, each the exact fraction
 * rounded once to binary32 (a value that rounds to 1 is stored as the largest float below 1), all in [0, 1) */
void trc_host_halton_offsets(uint32_t n, float* out /* 2 n */);
/* The reference's literals for a material type (MicrofacetBXDF.h:438-455, 514-530, 576-586): Plastic alpha (0.01, 0.1), eta 1.5;
 * Glass (0.01, 0.01), 1.5; Metal (0.01, 0.02), metal_eta (0.18, 0.15, 0.81), metal_k (1, 1, 1).  Fields a type does not use, and every
 * other type, take Plastic's values and metal_eta / metal_k Metal's: a table made of these is valid, and a render under
 * TRC_FLAG_MATERIAL_PARAMS with it is the unflagged render. */
void trc_host_default_material_params(int32_t material_type, trc_material_params* out);

/* Scene assembly in the reference's order (AAPLRenderer.mm:213-246,459-468,
 * 513-610): prepareCubeList (materials 0-2), prepareCornellBox (3-6),
 * prepareSphereList (7-18), testMaterial (19); leaves = cubes 0..n-2, all
 * squares, [spheres], [mesh triangles]; then buildTree. */
typedef struct trc_host_scene trc_host_scene;

enum trc_host_scene_kind {
    TRC_SCENE_CORNELL          = 0,  /* as shipped: 2 cubes + 7 squares (spheres not in the BVH) */
    TRC_SCENE_CORNELL_SPHERES  = 1,  /* BASELINE config 2: + the 12 spheres, materials remapped */
    TRC_SCENE_CORNELL_MESH     = 2,  /* + a triangle mesh placed by the reference transform */
    TRC_SCENE_CORNELL_VOLUME   = 3   /* kind 0 + the third cube of prepareCubeList (Tracer.mm:221-243: material _NIL_,
                                        medium GridDensity -- the cloud container the reference keeps out of
                                        its BVH, AAPLRenderer.mm:459) as a leaf; optional mesh as in kind 2 */
};

/* mesh: optional (NULL for kinds 0/1); positions/normals/uvs as
 * trc_TriangleVertex + triangle indices in OBJECT space; placement
 * (AAPLRenderer.mm:513-525,562-572) is applied by the call. */
trc_status trc_host_scene_create(int32_t kind,
                                 const trc_TriangleVertex* mesh_vertices, uint32_t n_vertices,
                                 const uint32_t* mesh_indices, uint32_t n_indices,
                                 trc_host_scene** out);
/* analytic_leaves_only != 0: the same scene without the per-triangle leaf records and without the tree -- bvhList = the leaf
 * records of the analytic primitives, the input of trc_upload_scene_device(TRC_TREE_SAH | TRC_TREE_TRIANGLE_LEAVES), which
 * writes the triangles' leaves and builds the reference's tree on the GPU */
trc_status trc_host_scene_create_leaves(int32_t kind,
                                        const trc_TriangleVertex* mesh_vertices, uint32_t n_vertices,
                                        const uint32_t* mesh_indices, uint32_t n_indices,
                                        int32_t analytic_leaves_only, trc_host_scene** out);
void       trc_host_scene_destroy(trc_host_scene* s);
/* view of the assembled arrays (valid until destroy) */
void       trc_host_scene_view(const trc_host_scene* s, trc_scene* out);

/* GridDensityInfo::GridDensityInfo (Medium.hh:92-105): sigma_t = sigma_a + sigma_s, invMaxDensity = 1 / max */
void trc_host_make_density_info(float sigma_a, float sigma_s, float g, uint32_t nx, uint32_t ny, uint32_t nz,
                                const float* density, trc_GridDensityInfo* out);
/* procedural stand-in for cloud/geometry/density_render.70.pbrt (100x100x40, does not travel to the GPU box):
 * a few smooth blobs, values in [0, ~2], deterministic in `seed` */
void trc_host_make_cloud(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t seed, float* out /* nx*ny*nz */);
/* reads the `MakeNamedMedium ... "integer nx" .. "float density" [ ... ]` block of a pbrt-v3 file (the subset
 * of minipbrt the reference uses, AAPLRenderer.mm:629-636); *out is malloc'ed, free with trc_host_free */
trc_status trc_host_load_density_pbrt(const char* path, uint32_t* nx, uint32_t* ny, uint32_t* nz, float** out);
void trc_host_free(void* p);

/* Radiance RGBE (.hdr) image -> float RGB, rows BOTTOM-UP (what trc_set_environment_map takes, and what the reference's
 * vertically flipped HDR texture holds: vulture_hide_4k.hdr, AAPLRenderer.mm:352-383, sampled through Render.hh:42-48);
 * flat and run-length-encoded scanlines; *rgb is malloc'ed (3 * w * h floats), free with trc_host_free */
trc_status trc_host_load_hdr(const char* path, uint32_t* width, uint32_t* height, float** rgb);

/* PNG -> float RGB for trc_upload_textures, in trc_host_load_hdr's layout (rows bottom-up: the reference's
 * MTKTextureLoaderOriginFlippedVertically): channel = byte / 255 (no gamma: MTKTextureLoaderOptionSRGB NO), grey replicated,
 * alpha dropped.  Bit depth 8, colour types 0 / 2 / 4 / 6, not interlaced, filters 0-4; palette, 16-bit and Adam7 files:
 * TRC_ERR_UNSUPPORTED; bad chunk CRC, bad Adler-32, truncated stream, more than 2^28 pixels: TRC_ERR_INVALID_ARG.
 * *rgb is malloc'ed (3 * w * h floats), free with trc_host_free */
trc_status trc_host_load_png(const char* path, uint32_t* width, uint32_t* height, float** rgb);

/* "Export as PNG file" (the reference's unchecked to-do, RT_Metal/README.md:61): 8-bit RGBA, rows top-down,
 * stored (uncompressed) deflate blocks -- no zlib dependency */
trc_status trc_host_write_png(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* Tables of pbrt::SobolSampler (SobolSampler.hh:126-160), generated by include/trc_sobol.h from the published
 * direction numbers instead of being stored: SobolMatrices32 for the first TRC_SOBOL_DIMS (40) dimensions
 * (out[dim * 52 + column]) and VdCSobolMatrices[log2res - 1] / VdCSobolMatricesInv[log2res - 1] (52 words each,
 * unused entries 0; 1 <= log2res <= 26).  libtracer_amd.so builds the same tables itself for TRC_FLAG_SOBOL. */
void       trc_host_sobol_matrices32(uint32_t* out /* [40 * 52] */);
trc_status trc_host_sobol_interval_tables(uint32_t log2res, uint64_t* vdc /* [52] */, uint64_t* inv /* [52] */);

/* minimal Wavefront OBJ reader (v / vn / vt / f; polygons fan-triangulated;
 * smooth normals generated when the file has none), standing in for ModelIO
 * (AAPLRenderer.mm:474-511).  Returns arrays owned by the mesh handle. */
typedef struct trc_host_mesh trc_host_mesh;
trc_status trc_host_mesh_load_obj(const char* path, trc_host_mesh** out);
/* every `Shape "trianglemesh"` of a pbrt-v3 file (the reference's unchecked to-do "Support pbrt-v3 file format",
 * RT_Metal/README.md:57; it vendors minipbrt for it, Tracer/minipbrt.h:1528-1546): points through the current
 * transformation matrix, normals through its inverse transpose (smooth normals when absent), uv / st, Include
 * followed; shapes inside ObjectBegin/ObjectEnd and other shape types are skipped */
trc_status trc_host_mesh_load_pbrt(const char* path, trc_host_mesh** out);
/* the triangles of a PLY file (ascii / binary_little_endian / binary_big_endian; x y z, optional nx ny nz and u v | s t;
 * triangles as they are, quads split (0 1 3) (2 3 1), larger polygons fanned) -- what `Shape "plymesh"` of a pbrt-v3 scene
 * refers to and what minipbrt's PLYMesh::triangle_mesh() returns (minipbrt.cpp:4380-4450) */
trc_status trc_host_mesh_load_ply(const char* path, trc_host_mesh** out);
/* A whole scene from a pbrt-v3 file -- the reference's unchecked to-do "Support pbrt-v3 file format"
 * (RT_Metal/README.md:57, the vendored parser RT_Metal/Tracer/minipbrt.h:1528-1546, its one call site
 * AAPLRenderer.mm:626-651): Camera "perspective" + LookAt, Film resolution, AreaLightSource "diffuse", Material
 * matte / plastic / metal / mirror / glass (+ MakeNamedMaterial / NamedMaterial), Texture "checkerboard", Shape "sphere",
 * "trianglemesh", "plymesh" (the PLY file is read: ascii / binary, triangles and quads), "disk" and "cylinder"
 * (tessellated) through the transformation and attribute stacks, Include.  Mapping onto the reference's primitives
 * (tracer_amd/host/pbrt_scene.cpp): sphere -> trc_Sphere; a trianglemesh that is an axis-aligned rectangle ->
 * trc_Square, emitters placed at squareList[5] / [6] (the two lights traceMIS samples); any other mesh -> triangles with
 * material 19 (the first mesh's material; per-mesh materials: trc_host_scene_load_pbrt_flags below).
 * `info` / `shapes` (optional, up to `capacity` entries in file order) describe what was parsed and what it became;
 * the scene handle is used like one from trc_host_scene_create. */
enum trc_pbrt_material { TRC_PBRT_MATTE = 0, TRC_PBRT_PLASTIC = 1, TRC_PBRT_METAL = 2, TRC_PBRT_MIRROR = 3,
                         TRC_PBRT_GLASS = 4, TRC_PBRT_OTHER = 5 };
/* what the file's Shape directive was (sphere / trianglemesh keep the primitive-type ordinals they map to) */
enum trc_pbrt_shape_kind { TRC_PBRT_SHAPE_SPHERE = 0, TRC_PBRT_SHAPE_TRIANGLEMESH = 3, TRC_PBRT_SHAPE_DISK = 6,
                           TRC_PBRT_SHAPE_CYLINDER = 7, TRC_PBRT_SHAPE_PLYMESH = 8, TRC_PBRT_SHAPE_CONE = 9,
                           TRC_PBRT_SHAPE_PARABOLOID = 10, TRC_PBRT_SHAPE_HYPERBOLOID = 11 };
/* what the material's colour parameter names ("texture Kd" "name"): nothing, a 2-D checkerboard (rendered through the
 * reference's TextureInfo{Checker}, Texture.hh:17-43, with albedo = tex1), any other texture class (not rendered) */
enum trc_pbrt_texture { TRC_PBRT_TEX_NONE = 0, TRC_PBRT_TEX_CHECKERBOARD = 1, TRC_PBRT_TEX_OTHER = 2 };
typedef struct trc_pbrt_info {
    float    camera_to_world[16];   /* row-major, inverse of the CTM at the Camera directive (minipbrt Camera::cameraToWorld) */
    float    fov, lensradius, focaldistance;
    uint32_t perspective;           /* Camera "perspective" */
    uint32_t xres, yres;            /* Film "image" */
    uint32_t n_shapes;              /* world shapes in file order (object templates excluded), then the shapes of every instance */
    uint32_t n_unsupported_shapes, n_unsupported_materials, n_triangle_material_conflicts;
    uint32_t mis_ready;             /* squareList[5] and [6] are emitters: TRC_INTEGRATOR_MIS / _VOLUME are usable */
    uint32_t n_unsupported_textures;/* shapes whose colour names a texture other than a 2-D checkerboard */
    uint32_t n_instances;           /* ObjectInstance directives: each placed as a flat copy of its template's shapes, after the
                                       world's own shapes, in file order (the reference's scene arrays have no instance level) */
} trc_pbrt_info;
typedef struct trc_pbrt_shape {
    int32_t  kind;                  /* enum trc_pbrt_shape_kind, or -1 (a shape class that is not handled) */
    float    shape_to_world[16];    /* row-major CTM at the Shape directive */
    float    radius;                /* spheres, disks, cylinders, cones, paraboloids */
    uint32_t n_vertices, n_indices; /* triangle meshes, PLY meshes; quadrics (disk ... hyperboloid): of their tessellation */
    int32_t  material;              /* enum trc_pbrt_material of the graphics state */
    float    color[3];              /* Kd (matte, plastic, other), Kr (mirror), Kt (glass), 1 (metal) */
    int32_t  emitter;               /* inside an AreaLightSource "diffuse" */
    float    L[3];
    int32_t  mapped_type;           /* TRC_PRIM_SPHERE / _SQUARE / _TRIANGLE it became, -1 if dropped */
    uint32_t mapped_index;          /* index in that primitive list (first triangle for a mesh) */
    uint32_t mapped_material;       /* index into the scene's material table */
    float    zmin, zmax;            /* cylinder, paraboloid; disk: both = height; cone: 0, height; hyperboloid: the z range of p1, p2 */
    float    innerradius, phimax;   /* disk; every quadric (degrees) */
    int32_t  texture;               /* enum trc_pbrt_texture of the material's colour parameter */
    float    tex2[3];               /* checkerboard: the second colour (color[] holds tex1) */
    float    p1[3], p2[3];          /* hyperboloid: the swept segment's end points */
} trc_pbrt_shape;
trc_status trc_host_scene_load_pbrt(const char* path, trc_host_scene** out_scene, trc_Camera* out_camera,
                                    trc_pbrt_info* info, trc_pbrt_shape* shapes, uint32_t capacity);
/* trc_host_scene_load_pbrt with options; flags == 0 is trc_host_scene_load_pbrt, output for output.
 * TRC_PBRT_TRIANGLE_MATERIALS: every mesh shape (trianglemesh, plymesh, tessellated quadrics, instance copies; emitters and
 * checkerboards included) also gets its own material, interned into the table after index 19 -- the materials of today's
 * load keep their indices, 19 included, so a caller that ignores the array renders the same scene.  Its shape record's
 * mapped_material names that material, n_triangle_material_conflicts stays 0, and trc_host_scene_triangle_materials returns
 * one index per triangle for trc_upload_triangle_materials.  Unknown flag bits: TRC_ERR_INVALID_ARG. */
#define TRC_PBRT_TRIANGLE_MATERIALS 1u
trc_status trc_host_scene_load_pbrt_flags(const char* path, uint32_t flags, trc_host_scene** out_scene, trc_Camera* out_camera,
                                          trc_pbrt_info* info, trc_pbrt_shape* shapes, uint32_t capacity);
/* the per-triangle material indices of a scene loaded with TRC_PBRT_TRIANGLE_MATERIALS (valid until destroy); *n = 0 for
 * any other handle */
void       trc_host_scene_triangle_materials(const trc_host_scene* s, const uint32_t** out, uint32_t* n);

/* procedural stand-in for the missing/untravelling assets: a displaced
 * UV-sphere "ball" with n_lat x n_lon quads (2 triangles each) */
trc_status trc_host_mesh_make_ball(uint32_t n_lat, uint32_t n_lon, float bump, trc_host_mesh** out);
/* a mesh handle over caller arrays (copied): the vertex / index buffers a host already holds -- what the reference
 * gets from MDLMesh.vertexBuffers / submesh.indexBuffer (AAPLRenderer.mm:527-529) */
trc_status trc_host_mesh_from_arrays(const trc_TriangleVertex* vertices, uint32_t n_vertices,
                                     const uint32_t* indices, uint32_t n_indices, trc_host_mesh** out);
/* k x k grid replication (config 4: >= 1 M triangles) */
trc_status trc_host_mesh_replicate(const trc_host_mesh* src, uint32_t k, float spacing, trc_host_mesh** out);
void       trc_host_mesh_view(const trc_host_mesh* m, const trc_TriangleVertex** vertices,
                              uint32_t* n_vertices, const uint32_t** indices, uint32_t* n_indices);
void       trc_host_mesh_destroy(trc_host_mesh* m);

#ifdef __cplusplus
}  /* extern "C" */
#endif

/* ------------------------------------------------------------------ */
/* layout locks                                 */
/* ------------------------------------------------------------------ */
#if defined(__cplusplus)
#define TRC_SA(c, m) static_assert(c, m)
#else
#define TRC_SA(c, m) _Static_assert(c, m)
#endif
TRC_SA(sizeof(trc_float2) == 8 && sizeof(trc_float3) == 16 && sizeof(trc_float4x4) == 64, "simd sizes");
TRC_SA(sizeof(trc_AABB) == 32 && offsetof(trc_AABB, maxi) == 16, "AABB");
TRC_SA(sizeof(trc_BVH) == 64 && offsetof(trc_BVH, pType) == 16 && offsetof(trc_BVH, pIndex) == 20 &&
       offsetof(trc_BVH, bBOX) == 32, "BVH");
TRC_SA(sizeof(trc_Sphere) == 272 && offsetof(trc_Sphere, center) == 16 && offsetof(trc_Sphere, model_matrix) == 32 &&
       offsetof(trc_Sphere, normal_matrix) == 96 && offsetof(trc_Sphere, inverse_matrix) == 160 &&
       offsetof(trc_Sphere, material) == 224 && offsetof(trc_Sphere, boundingBOX) == 240, "Sphere");
TRC_SA(sizeof(trc_Square) == 272 && offsetof(trc_Square, axis_j) == 1 && offsetof(trc_Square, range_i) == 8 &&
       offsetof(trc_Square, range_j) == 16 && offsetof(trc_Square, axis_k) == 24 &&
       offsetof(trc_Square, value_k) == 28 && offsetof(trc_Square, model_matrix) == 32 &&
       offsetof(trc_Square, material) == 224 && offsetof(trc_Square, boundingBOX) == 240, "Square");
TRC_SA(sizeof(trc_Cube) == 240 && offsetof(trc_Cube, normal_matrix) == 64 && offsetof(trc_Cube, inverse_matrix) == 128 &&
       offsetof(trc_Cube, box) == 192 && offsetof(trc_Cube, material) == 224, "Cube");
TRC_SA(sizeof(trc_TriangleVertex) == 32, "TriangleVertex");
TRC_SA(sizeof(trc_material_params) == 48 && offsetof(trc_material_params, metal_eta) == 16 && offsetof(trc_material_params, metal_k) == 32, "material_params");
TRC_SA(sizeof(trc_pose) == 144 && offsetof(trc_pose, model_matrix) == 16 && offsetof(trc_pose, normal_matrix) == 80, "pose");
TRC_SA(sizeof(trc_skin_influence) == 32 && offsetof(trc_skin_influence, weight) == 16, "skin_influence");
TRC_SA(sizeof(trc_skin_bone) == 128 && offsetof(trc_skin_bone, normal_matrix) == 64, "skin_bone");
TRC_SA(sizeof(trc_morph_delta) == 24 && offsetof(trc_morph_delta, dn) == 12, "morph_delta");
TRC_SA(sizeof(trc_tree_cost_t) == 32 && offsetof(trc_tree_cost_t, n_interior) == 24, "tree_cost");
TRC_SA(sizeof(trc_triangle_range) == 12 && offsetof(trc_triangle_range, visible) == 8, "triangle_range");
TRC_SA(sizeof(trc_TextureInfo) == 32 && offsetof(trc_TextureInfo, albedo) == 16, "TextureInfo");
TRC_SA(sizeof(trc_Material) == 64 && offsetof(trc_Material, medium) == 4 && offsetof(trc_Material, specular) == 8 &&
       offsetof(trc_Material, eta) == 12 && offsetof(trc_Material, roughness) == 16 &&
       offsetof(trc_Material, textureInfo) == 32, "Material");
TRC_SA(sizeof(trc_Camera) == 176 && offsetof(trc_Camera, vfov) == 48 && offsetof(trc_Camera, focus_dist) == 64 &&
       offsetof(trc_Camera, u) == 80 && offsetof(trc_Camera, vertical) == 128 &&
       offsetof(trc_Camera, cornerLowLeft) == 160, "Camera");
TRC_SA(sizeof(trc_Complex) == 96 && offsetof(trc_Complex, frame_count) == 20 && offsetof(trc_Complex, photonBox) == 32 &&
       offsetof(trc_Complex, photonBoxSize) == 64 && offsetof(trc_Complex, photonInitialRadius) == 80 &&
       offsetof(trc_Complex, framePhotonSum) == 92, "Complex");
TRC_SA(sizeof(trc_ray) == 32, "trc_ray");
TRC_SA(sizeof(trc_hit) == 80 && offsetof(trc_hit, p) == 16 && offsetof(trc_hit, uv) == 52 && offsetof(trc_hit, n_descend) == 68, "trc_hit");
TRC_SA(sizeof(trc_params) == 32 && sizeof(trc_stats) == 112, "trc_params / trc_stats");
TRC_SA(sizeof(trc_GridDensityInfo) == 32 && offsetof(trc_GridDensityInfo, invMaxDensity) == 16 && offsetof(trc_GridDensityInfo, nx) == 20, "GridDensityInfo");
TRC_SA(sizeof(trc_PhotonRecord) == 80 && offsetof(trc_PhotonRecord, normal) == 16 && offsetof(trc_PhotonRecord, position) == 32 &&
       offsetof(trc_PhotonRecord, direction) == 48 && offsetof(trc_PhotonRecord, step) == 64 &&
       offsetof(trc_PhotonRecord, active) == 65, "PhotonRecord");
TRC_SA(sizeof(trc_CameraRecord) == 112 && offsetof(trc_CameraRecord, position) == 16 && offsetof(trc_CameraRecord, direction) == 32 &&
       offsetof(trc_CameraRecord, valid) == 48 && offsetof(trc_CameraRecord, alternative) == 64 &&
       offsetof(trc_CameraRecord, flux) == 80 && offsetof(trc_CameraRecord, radius) == 96 &&
       offsetof(trc_CameraRecord, photonCount) == 100, "CameraRecord");
TRC_SA(sizeof(trc_gbuffer_texel) == 32 && offsetof(trc_gbuffer_texel, normal) == 4 && offsetof(trc_gbuffer_texel, albedo) == 16 &&
       offsetof(trc_gbuffer_texel, id) == 28, "gbuffer texel");
TRC_SA(sizeof(trc_denoise_params) == 32, "trc_denoise_params");
TRC_SA(sizeof(trc_motion_texel) == 16, "trc_motion_texel");
TRC_SA(sizeof(trc_adaptive_params) == 16 && offsetof(trc_adaptive_params, max_spp) == 4 && offsetof(trc_adaptive_params, reserved) == 8, "trc_adaptive_params");
TRC_SA(sizeof(trc_adaptive_report) == 24 && offsetof(trc_adaptive_report, active_tiles) == 4 && offsetof(trc_adaptive_report, samples) == 8 &&
       offsetof(trc_adaptive_report, max_error) == 16, "trc_adaptive_report");

#endif /* TRACER_ABI_H */
