// trc_render.cpp -- a C++ host driving the path through the C ABI only (include/tracer_abi.h), the way
// -[AAPLRenderer render:] drives the Metal path: scene prep on the host (libtrc_host.so), upload, N samples,
// output stage, PNG.  Nothing but the two shared libraries is involved.
//
//   trc_render [--scene cornell|spheres|volume] [--integrator path|mis|volume] [--size W H] [--spp N]
//              [--mesh file.obj|file.pbrt] [--albedo-map file.png] [--density cloud.pbrt] [--lbvh | --device-sah | --device-sah3] [--sobol] [--out frame.png]
//              [--hdr map.hdr [--env-light]]  --env-light: traceMIS samples the map as a light (TRC_FLAG_ENV_LIGHT), no square light needed
//              [--spin N]  after the frame, N more frames of the mesh turned about its own vertical axis (360 / N degrees per frame) through
//                          trc_update_vertices: no second upload, the tree is refitted in place; frame k goes to <out>.k.png
//              [--pose N]  the same turn, sent as ONE matrix per frame (trc_pose_vertices: the device keeps the rest vertices and poses
//                          them itself, 144 bytes cross the bus instead of the vertex array); frame k goes to <out>.k.png
//              [--bend N]  N frames of a two-bone bend: the foot of the mesh stands, its top makes --pose's turn, and every vertex blends
//                          the two by its height (trc_skin_bind once, trc_skin_vertices per frame); frame k goes to <out>.k.png
//              [--morph N] N frames of two blend shapes with swinging weights: one swells the mesh, one presses it towards its foot
//                          (trc_morph_bind once, trc_morph_vertices per frame); with --bend each of these frames is the morph AND --bend's
//                          two bones on top of it in one call; frame k goes to <out>.k.png
//              [--orbit N] N frames of the config-2 scene (--scene spheres) with its twelve spheres circling the vertical axis through the middle
//                          of the box, 360 / N degrees per frame: the records are built on the host (trc_host_make_sphere) and sent through
//                          trc_update_primitives -- no second upload, the tree is refitted in place; frame k goes to <out>.k.png
//              [--rebuild-ratio R]  beside --spin / --pose / --bend / --morph: after every animation call the tree's cost is read (trc_tree_cost), and
//                          when (interior + leaf) / root exceeds R times what it was right after the last build, the tree is built anew on the
//                          device (trc_rebuild_tree, TRC_TREE_SAH); the number of rebuilds is printed at the end
//              [--normals]  beside --spin / --pose / --bend / --morph: after every animation call the smooth normals of the whole mesh are
//                          derived anew on the device from the vertices as they now stand (trc_recompute_normals); its device time is printed
//                          beside the animation call's, and the first call, which builds the adjacency, is timed between two trc_synchronize
//              [--denoise]  beside --spin / --pose / --bend / --morph / --orbit: the SVGF history follows the moving mesh or spheres (trc_denoise_track_motion), every
//                          frame is denoised (trc_denoise) and the DENOISED frame is what <out> and <out>.k.png hold; per frame the mean
//                          history length over the hit pixels is printed (1 = no history; it grows by one per frame where the filter
//                          found the surface again).  Use it with a low --spp: that is what the history is for
//              [--hide FIRST:COUNT]  after the upload, triangles FIRST .. FIRST + COUNT - 1 of the mesh lose their leaves (trc_set_triangle_visibility,
//                          TRC_TREE_SAH: the tree over what is left is built on the device); may be given more than once, and combines with
//                          --spin / --pose / --bend / --morph: hidden triangles go on moving, they have no leaf to refit
//              [--adaptive THRESHOLD|default [--max-spp N]]  the frame by trc_render_adaptive instead of trc_render: a first pass of --spp samples
//                          (16 unless given) over every tile, then passes that double the count on the 16 x 16 tiles whose error estimate is still
//                          above THRESHOLD, up to N (256) samples; prints the report and writes the per-tile sample counts as a grey image
//                          (255 = N samples) to <out>.samples.png.  Takes traceMIS unless --integrator says otherwise (tracer_abi.h: why)
//              [--aa N]    anti-aliasing: N camera-ray sets (1 .. 1024) with Halton sub-pixel offsets are generated on the device
//                          (trc_host_halton_offsets, trc_generate_camera_rays) and the frame is rendered with TRC_FLAG_CAMERA_RAYS: sample s takes
//                          set s % N.  tracePath / traceMIS, with --env-light too (a final frame of an env-lit scene); not with --sobol or
//                          --mesh-lights (tracer_abi.h)
//              [--projection pinhole|ortho|equirect]  the projection of those sets (one set at zero offset without --aa): the camera's own,
//                          orthographic through the view plane, or a 360 degree panorama from the eye (world axes, as the --hdr map's:
//                          --projection equirect --hdr map.hdr --env-light --integrator mis is a panorama of the scene lit by that map).
//                          With --denoise the filter follows these rays (trc_denoise_guide_rays): its G-buffer is walked along set 0
//              [--material-params M:AX:AY[:ETA]]  material M of the scene gets the roughness pair (AX, AY) and, if given, the dielectric index
//                          ETA instead of the reference's literals (Plastic 0.01, 0.1, 1.5; Glass 0.01, 0.01, 1.5; Metal 0.01, 0.02): every
//                          other entry of the table keeps trc_host_default_material_params, and the frame is rendered with
//                          TRC_FLAG_MATERIAL_PARAMS.  May be given more than once.  tracePath / traceMIS; not with --sobol, --env-light,
//                          --mesh-lights, --aa or --projection (tracer_abi.h)
//              [--mesh-lights]  traceMIS samples the mesh's emissive triangles as lights (TRC_FLAG_MESH_LIGHTS; with --triangle-materials a
//                               pbrt file's emissive trianglemesh), no square light needed
//              --albedo-map: the mesh's material (19) becomes an Image texture of that PNG (trc_host_load_png + trc_upload_textures),
//              as the reference's host binds uv_test.png (AAPLRenderer.mm:385-390)
//   trc_render --pbrt scene.pbrt [--triangle-materials] [--integrator path|mis] [--spp N] [--size W H] [--out frame.png]
//              a whole pbrt-v3 scene (camera, film, lights, materials, spheres, meshes: trc_host_scene_load_pbrt)
//              --triangle-materials: every mesh keeps its own material (TRC_PBRT_TRIANGLE_MATERIALS + trc_upload_triangle_materials)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tracer_abi.h"

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        trc_status st_ = (call);                                                                     \
        if (st_ != TRC_OK) {                                                                         \
            std::fprintf(stderr, "%s failed: %s (%s)\n", #call, trc_status_string(st_), ctx ? trc_last_error(ctx) : ""); \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

int main(int argc, char** argv) {
    std::string scene_name = "spheres", integ_name = "path", out = "frame.png", mesh_path, density_path, pbrt_path, hdr_path, albedo_path;
    uint32_t W = 640, H = 360, spp = 64;
    uint32_t spin = 0, pose = 0, bend = 0, morph = 0, orbit = 0;
    uint32_t aa = 0, ray_model = TRC_RAYS_PINHOLE;
    struct ParamEdit { uint32_t material; float ax, ay, eta; };      // --material-params (eta 0: keep the default)
    std::vector<ParamEdit> param_edits;
    bool projection = false;
    std::vector<trc_triangle_range> hidden;
    double rebuild_ratio = 0.0;
    bool adaptive = false, spp_given = false, integ_given = false;
    trc_adaptive_params ad;
    trc_adaptive_default_params(&ad);
    bool lbvh = false, device_sah = false, device_sah3 = false, sobol = false, size_given = false, env_light = false, mesh_lights = false, tri_materials = false, normals = false, denoise = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--scene" && i + 1 < argc) scene_name = argv[++i];
        else if (a == "--integrator" && i + 1 < argc) { integ_name = argv[++i]; integ_given = true; }
        else if (a == "--size" && i + 2 < argc) { W = (uint32_t)std::atoi(argv[++i]); H = (uint32_t)std::atoi(argv[++i]); size_given = true; }
        else if (a == "--pbrt" && i + 1 < argc) pbrt_path = argv[++i];          // a whole pbrt-v3 scene
        else if (a == "--spp" && i + 1 < argc) { spp = (uint32_t)std::atoi(argv[++i]); spp_given = true; }
        else if (a == "--adaptive" && i + 1 < argc) {                           // samples where the picture is still noisy: trc_render_adaptive
            adaptive = true;
            if (std::strcmp(argv[++i], "default") != 0) ad.threshold = (float)std::atof(argv[i]);
            if (!(ad.threshold > 0.0f) || !std::isfinite(ad.threshold)) { std::fprintf(stderr, "--adaptive wants a threshold above 0 (or `default`), not %s\n", argv[i]); return 2; }
        }
        else if (a == "--max-spp" && i + 1 < argc) ad.max_spp = (uint32_t)std::atoi(argv[++i]);
        else if (a == "--mesh" && i + 1 < argc) mesh_path = argv[++i];          // Wavefront OBJ, PLY or pbrt-v3 trianglemeshes
        else if (a == "--hdr" && i + 1 < argc) hdr_path = argv[++i];            // Radiance .hdr backdrop (the reference's texHDR)
        else if (a == "--albedo-map" && i + 1 < argc) albedo_path = argv[++i];  // PNG image texture on the mesh material
        else if (a == "--density" && i + 1 < argc) density_path = argv[++i];    // pbrt-v3 heterogeneous medium
        else if (a == "--lbvh") lbvh = true;
        else if (a == "--device-sah") device_sah = true;
        else if (a == "--device-sah3") device_sah = device_sah3 = true;      // --device-sah with the three-axis, 32-bin split (TRC_TREE_SAH3)
        else if (a == "--sobol") sobol = true;
        else if (a == "--spin" && i + 1 < argc) {                               // moving geometry: trc_update_vertices per frame
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > 100000) { std::fprintf(stderr, "--spin wants a number of frames from 1 to 100000, not %s\n", argv[i]); return 2; }
            spin = (uint32_t)n;
        }
        else if (a == "--pose" && i + 1 < argc) {                               // moving geometry: one matrix per frame, trc_pose_vertices
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > 100000) { std::fprintf(stderr, "--pose wants a number of frames from 1 to 100000, not %s\n", argv[i]); return 2; }
            pose = (uint32_t)n;
        }
        else if (a == "--bend" && i + 1 < argc) {                               // bending geometry: a two-bone palette per frame, trc_skin_vertices
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > 100000) { std::fprintf(stderr, "--bend wants a number of frames from 1 to 100000, not %s\n", argv[i]); return 2; }
            bend = (uint32_t)n;
        }
        else if (a == "--morph" && i + 1 < argc) {                              // blend shapes: two weights per frame, trc_morph_vertices
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > 100000) { std::fprintf(stderr, "--morph wants a number of frames from 1 to 100000, not %s\n", argv[i]); return 2; }
            morph = (uint32_t)n;
        }
        else if (a == "--orbit" && i + 1 < argc) {                              // moving primitives: twelve sphere records per frame, trc_update_primitives
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > 100000) { std::fprintf(stderr, "--orbit wants a number of frames from 1 to 100000, not %s\n", argv[i]); return 2; }
            orbit = (uint32_t)n;
        }
        else if (a == "--rebuild-ratio" && i + 1 < argc) {                   // a fresh tree when the refitted one has worn: trc_tree_cost, trc_rebuild_tree
            rebuild_ratio = std::atof(argv[++i]);
            if (!(rebuild_ratio >= 1.0)) { std::fprintf(stderr, "--rebuild-ratio wants a factor of at least 1, not %s\n", argv[i]); return 2; }
        }
        else if (a == "--hide" && i + 1 < argc) {                               // mesh triangles without a leaf: trc_set_triangle_visibility
            unsigned long long first = 0, count = 0;
            if (std::sscanf(argv[++i], "%llu:%llu", &first, &count) != 2 || first > 0xFFFFFFFFull || count > 0xFFFFFFFFull) {
                std::fprintf(stderr, "--hide wants FIRST:COUNT, two triangle numbers, not %s\n", argv[i]);
                return 2;
            }
            hidden.push_back(trc_triangle_range{(uint32_t)first, (uint32_t)count, 0u});
        }
        else if (a == "--aa" && i + 1 < argc) {                                 // anti-aliasing: Halton-offset camera-ray sets, TRC_FLAG_CAMERA_RAYS
            const int n = std::atoi(argv[++i]);
            if (n <= 0 || n > (int)TRC_MAX_RAY_SETS) { std::fprintf(stderr, "--aa wants a number of ray sets from 1 to %u, not %s\n", TRC_MAX_RAY_SETS, argv[i]); return 2; }
            aa = (uint32_t)n;
        }
        else if (a == "--material-params" && i + 1 < argc) {                    // per-material roughness / index, TRC_FLAG_MATERIAL_PARAMS
            unsigned m = 0;
            float ax = 0, ay = 0, eta = 0;
            const int got = std::sscanf(argv[++i], "%u:%f:%f:%f", &m, &ax, &ay, &eta);
            if (got < 3 || !(ax > 0) || !(ay > 0) || (got == 4 && !(eta > 1))) {
                std::fprintf(stderr, "--material-params wants M:AX:AY[:ETA] with AX, AY > 0 and ETA > 1, not %s\n", argv[i]);
                return 2;
            }
            param_edits.push_back(ParamEdit{m, ax, ay, got == 4 ? eta : 0.0f});
        }
        else if (a == "--projection" && i + 1 < argc) {                         // the projection of the camera-ray sets
            const std::string m = argv[++i];
            if (m != "pinhole" && m != "ortho" && m != "equirect") { std::fprintf(stderr, "--projection wants pinhole, ortho or equirect, not %s\n", argv[i]); return 2; }
            ray_model = m == "ortho" ? TRC_RAYS_ORTHOGRAPHIC : m == "equirect" ? TRC_RAYS_EQUIRECT : TRC_RAYS_PINHOLE;
            projection = true;
        }
        else if (a == "--normals") normals = true;                             // smooth normals re-derived on the device after every animation call
        else if (a == "--denoise") denoise = true;                              // SVGF on every frame, the history kept across the animation calls
        else if (a == "--mesh-lights") mesh_lights = true;                     // traceMIS samples the emissive triangles (TRC_FLAG_MESH_LIGHTS)
        else if (a == "--env-light") env_light = true;                          // traceMIS samples the --hdr map as a light (TRC_FLAG_ENV_LIGHT)
        else if (a == "--triangle-materials") tri_materials = true;            // --pbrt: per-mesh materials instead of material 19
        else if (a == "--out" && i + 1 < argc) out = argv[++i];
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (adaptive && !integ_given) integ_name = "mis";
    if (adaptive && !spp_given) spp = 16;
    int kind = scene_name == "cornell" ? TRC_SCENE_CORNELL : scene_name == "volume" ? TRC_SCENE_CORNELL_VOLUME : TRC_SCENE_CORNELL_SPHERES;
    if (!mesh_path.empty() && kind != TRC_SCENE_CORNELL_VOLUME) kind = TRC_SCENE_CORNELL_MESH;   // the mesh slot of AAPLRenderer.mm:474-603
    const uint32_t integrator = integ_name == "mis" ? TRC_INTEGRATOR_MIS : integ_name == "volume" ? TRC_INTEGRATOR_VOLUME : TRC_INTEGRATOR_PATH;

    trc_ctx* ctx = nullptr;
    trc_host_scene* hs = nullptr;
    trc_host_mesh* mesh = nullptr;
    const trc_TriangleVertex* mv = nullptr; const uint32_t* mi = nullptr;
    uint32_t n_mv = 0, n_mi = 0;
    if (!mesh_path.empty()) {
        const bool pbrt = mesh_path.size() > 5 && mesh_path.compare(mesh_path.size() - 5, 5, ".pbrt") == 0;
        const bool ply = mesh_path.size() > 4 && mesh_path.compare(mesh_path.size() - 4, 4, ".ply") == 0;
        if ((pbrt ? trc_host_mesh_load_pbrt(mesh_path.c_str(), &mesh) : ply ? trc_host_mesh_load_ply(mesh_path.c_str(), &mesh)
                  : trc_host_mesh_load_obj(mesh_path.c_str(), &mesh)) != TRC_OK) {
            std::fprintf(stderr, "cannot read a triangle mesh from %s\n", mesh_path.c_str());
            return 1;
        }
        trc_host_mesh_view(mesh, &mv, &n_mv, &mi, &n_mi);
    }
    trc_Camera cam;
    if (tri_materials && pbrt_path.empty()) { std::fprintf(stderr, "--triangle-materials needs --pbrt\n"); return 2; }
    if (!pbrt_path.empty()) {
        trc_pbrt_info info;
        if (trc_host_scene_load_pbrt_flags(pbrt_path.c_str(), tri_materials ? TRC_PBRT_TRIANGLE_MATERIALS : 0u, &hs, &cam, &info, nullptr, 0) != TRC_OK) {
            std::fprintf(stderr, "cannot read a scene from %s\n", pbrt_path.c_str());
            return 1;
        }
        if (!size_given) { W = info.xres; H = info.yres; }         // the camera's aspect is the film's
        if (integrator != TRC_INTEGRATOR_PATH && !info.mis_ready && !(env_light && !hdr_path.empty()) && !mesh_lights) {
            std::fprintf(stderr, "%s has no rectangular area light: traceMIS samples squareList[5] / [6]; use --integrator path, --hdr with --env-light, or --mesh-lights\n",
                         pbrt_path.c_str());
            return 1;
        }
        if (mesh_lights && !tri_materials && !info.mis_ready) {      // every triangle is material 19: no light triangle, and no square either
            std::fprintf(stderr, "%s has no rectangular area light, and without --triangle-materials no triangle is an emitter: --mesh-lights would render black\n",
                         pbrt_path.c_str());
            return 1;
        }
        scene_name = pbrt_path;
        std::fprintf(stderr, "%s: %u shapes (%u not handled), %u materials and %u textures not handled\n", pbrt_path.c_str(), info.n_shapes,
                     info.n_unsupported_shapes, info.n_unsupported_materials, info.n_unsupported_textures);
    } else {
        // --device-sah: the host prepares its analytic primitives and the mesh only -- no leaf record per triangle, no tree
        if (trc_host_scene_create_leaves(kind, mv, n_mv, mi, n_mi, device_sah ? 1 : 0, &hs) != TRC_OK) { std::fprintf(stderr, "scene prep failed\n"); return 1; }
        trc_host_prepare_camera(&cam, (float)W, (float)H);
    }
    trc_scene scene;
    trc_host_scene_view(hs, &scene);
    std::vector<trc_Material> materials;         // --albedo-map: the scene's materials with the mesh's (19, dev_intersect.hpp) as Image 0
    constexpr uint32_t kMeshMaterial = 19;
    if (!albedo_path.empty()) {
        if (scene.n_material <= kMeshMaterial || !pbrt_path.empty() || mesh_path.empty()) {
            std::fprintf(stderr, "--albedo-map textures the mesh material of a --mesh scene\n");
            return 2;
        }
        materials.assign(scene.materials, scene.materials + scene.n_material);
        materials[kMeshMaterial].textureInfo.type = TRC_TEX_IMAGE;
        materials[kMeshMaterial].textureInfo.textureIndex = 0;
        scene.materials = materials.data();
    }

    CHECK(trc_create(0, &ctx));
    if (device_sah && pbrt_path.empty()) {        // triangle leaves + BVH::buildTree itself, both on the device
        CHECK(trc_upload_scene_device(ctx, &scene, TRC_TREE_SAH | TRC_TREE_TRIANGLE_LEAVES | (device_sah3 ? TRC_TREE_SAH3 : 0u)));
    } else if (lbvh || device_sah) {              // hand over the leaf records only; the tree is built on the GPU
        trc_scene leaves = scene;
        leaves.bvhList = scene.bvhList + 1;       // BVH::buildTree keeps the leaves at [1, n]
        leaves.n_bvh = (scene.n_bvh + 1) / 2;
        if (device_sah3) CHECK(trc_upload_scene_device(ctx, &leaves, TRC_TREE_SAH | TRC_TREE_SAH3));
        else if (device_sah) CHECK(trc_upload_scene_sah(ctx, &leaves));
        else CHECK(trc_upload_scene_lbvh(ctx, &leaves));
    } else {
        CHECK(trc_upload_scene(ctx, &scene));
    }
    if (tri_materials) {                          // one material per triangle instead of the reference's 19 for all
        const uint32_t* tm = nullptr;
        uint32_t n_tm = 0;
        trc_host_scene_triangle_materials(hs, &tm, &n_tm);
        if (n_tm) CHECK(trc_upload_triangle_materials(ctx, tm, n_tm));
    }
    if (!param_edits.empty()) {                   // the reference's literals per material, then the entries the command line names
        std::vector<trc_material_params> table(scene.n_material);
        for (uint32_t m = 0; m < scene.n_material; ++m) trc_host_default_material_params(scene.materials[m].type, &table[m]);
        for (const ParamEdit& e : param_edits) {
            if (e.material >= scene.n_material) { std::fprintf(stderr, "--material-params: the scene has %u materials, no material %u\n", scene.n_material, e.material); return 2; }
            table[e.material].alpha_x = e.ax; table[e.material].alpha_y = e.ay;
            if (e.eta != 0.0f) table[e.material].eta = e.eta;
        }
        CHECK(trc_upload_material_params(ctx, table.data(), scene.n_material));
        std::printf("material parameters: %zu of %u entries changed\n", param_edits.size(), scene.n_material);
    }
    std::vector<float> cloud;
    if (kind == TRC_SCENE_CORNELL_VOLUME) {
        uint32_t nx = 100, ny = 100, nz = 40;
        if (!density_path.empty()) {              // what AAPLRenderer.mm:629-636 reads through minipbrt
            float* grid = nullptr;
            if (trc_host_load_density_pbrt(density_path.c_str(), &nx, &ny, &nz, &grid) != TRC_OK) {
                std::fprintf(stderr, "cannot read a density grid from %s\n", density_path.c_str());
                return 1;
            }
            cloud.assign(grid, grid + (size_t)nx * ny * nz);
            trc_host_free(grid);
        } else {
            cloud.resize((size_t)nx * ny * nz);
            trc_host_make_cloud(nx, ny, nz, 1, cloud.data());
        }
        trc_GridDensityInfo info;
        trc_host_make_density_info(10.0f, 90.0f, 0.5f, nx, ny, nz, cloud.data(), &info);
        CHECK(trc_upload_density(ctx, &info, cloud.data()));
    }
    if (!hdr_path.empty()) {                     // AAPLRenderer.mm:352-383: the equirectangular backdrop, rows bottom-up
        uint32_t ew = 0, eh = 0;
        float* env = nullptr;
        if (trc_host_load_hdr(hdr_path.c_str(), &ew, &eh, &env) != TRC_OK) { std::fprintf(stderr, "cannot read a Radiance .hdr image from %s\n", hdr_path.c_str()); return 1; }
        const trc_status es = trc_set_environment_map(ctx, ew, eh, env);
        trc_host_free(env);
        CHECK(es);
    }
    if (!albedo_path.empty()) {                  // MTKTextureLoader with sRGB off, flipped vertically (AAPLRenderer.mm:349-447)
        trc_image img;
        float* rgb = nullptr;
        if (trc_host_load_png(albedo_path.c_str(), &img.width, &img.height, &rgb) != TRC_OK) {
            std::fprintf(stderr, "cannot read an 8-bit PNG image from %s\n", albedo_path.c_str());
            return 1;
        }
        img.rgb = rgb;
        const trc_status ts = trc_upload_textures(ctx, &img, 1);
        trc_host_free(rgb);
        CHECK(ts);
    }
    CHECK(trc_set_camera(ctx, &cam));
    CHECK(trc_resize(ctx, W, H));
    CHECK(trc_seed(ctx, 0x5EED0000ull));

    if (!hidden.empty()) {
        const auto h0 = std::chrono::steady_clock::now();
        CHECK(trc_set_triangle_visibility(ctx, hidden.data(), (uint32_t)hidden.size(), TRC_TREE_SAH | (device_sah3 ? TRC_TREE_SAH3 : 0u)));
        const double hide_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
        uint32_t n_records = 0;
        CHECK(trc_lbvh_info(ctx, &n_records, nullptr, nullptr));
        std::printf("--hide: %zu ranges, trc_set_triangle_visibility %.2f ms -> a tree of %u leaves\n", hidden.size(), hide_ms, (n_records + 1) / 2);
    }

    trc_params prm;
    std::memset(&prm, 0, sizeof prm);
    prm.spp = spp; prm.max_depth = 8; prm.integrator = integrator; prm.tile_nranks = 1;
    if (sobol) prm.flags |= TRC_FLAG_SOBOL;      // pbrt::SobolSampler instead of the random sampler (Render.metal:529-530)
    if (mesh_lights) prm.flags |= TRC_FLAG_MESH_LIGHTS;   // the mesh's emissive triangles as area-sampled lights of traceMIS
    if (env_light) prm.flags |= TRC_FLAG_ENV_LIGHT;  // the --hdr map as an importance-sampled light of traceMIS
    if (!param_edits.empty()) prm.flags |= TRC_FLAG_MATERIAL_PARAMS;      // the lobes read the table uploaded above
    if (aa || projection) {                      // camera-ray sets made on the device from the camera; every render below reads them
        const uint32_t n_sets = aa ? aa : 1u;
        std::vector<float> offsets(2 * (size_t)n_sets, 0.0f);
        if (aa) trc_host_halton_offsets(n_sets, offsets.data());
        trc_ray_gen gen;
        gen.model = ray_model; gen.n_sets = n_sets; gen.offsets = offsets.data();
        const auto g0 = std::chrono::steady_clock::now();
        CHECK(trc_generate_camera_rays(ctx, &gen));
        CHECK(trc_synchronize(ctx));
        const double gen_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
        std::printf("camera rays: %u set%s, %s, %.1f MB on the device, trc_generate_camera_rays %.2f ms\n", n_sets, n_sets == 1 ? "" : "s",
                    ray_model == TRC_RAYS_ORTHOGRAPHIC ? "orthographic" : ray_model == TRC_RAYS_EQUIRECT ? "equirectangular" : aa ? "pinhole with Halton offsets" : "pinhole",
                    (double)n_sets * W * H * sizeof(trc_ray) / 1e6, gen_ms);
        prm.flags |= TRC_FLAG_CAMERA_RAYS;
    }
    const auto t0 = std::chrono::steady_clock::now();
    trc_adaptive_report report{};
    if (adaptive) CHECK(trc_render_adaptive(ctx, &prm, &ad, &report));
    else CHECK(trc_render(ctx, &prm));
    CHECK(trc_synchronize(ctx));
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    trc_stats st;
    CHECK(trc_get_stats(ctx, &st));

    std::vector<uint8_t> rgba8((size_t)W * H * 4);
    float exposure = 0;
    // --denoise: the frame's output stage.  Tracking is switched on before the first trc_denoise, so that the history this frame leaves
    // is the one the first animation frame finds; history_note: what that frame's line of output ends with
    std::vector<float> history;
    std::vector<trc_gbuffer_texel> gbuffer;
    std::string history_note;
    trc_denoise_params dn;
    trc_denoise_default_params(&dn);
    dn.flags = TRC_DENOISE_DEMODULATE;
    auto denoised_output = [&]() {
        trc_status rs;
        if ((rs = trc_denoise(ctx, &dn)) != TRC_OK || (rs = trc_tonemap_denoised(ctx, rgba8.data(), &exposure)) != TRC_OK) return rs;
        history.resize((size_t)W * H); gbuffer.resize((size_t)W * H);
        if ((rs = trc_download_history_length(ctx, history.data())) != TRC_OK || (rs = trc_download_gbuffer(ctx, gbuffer.data())) != TRC_OK) return rs;
        double sum = 0.0; size_t hit = 0;
        for (size_t i = 0; i < history.size(); ++i)
            if (gbuffer[i].id != TRC_GBUFFER_MISS) { sum += history[i]; ++hit; }
        char text[96];
        std::snprintf(text, sizeof text, ", denoised, mean history length %.2f over %zu hit pixels", hit ? sum / hit : 0.0, hit);
        history_note = text;
        return TRC_OK;
    };
    // what every animation frame does once its vertices are in place
    auto animation_frame = [&]() {
        trc_status rs;
        if ((rs = trc_clear_accum(ctx)) != TRC_OK || (rs = trc_render(ctx, &prm)) != TRC_OK) return rs;
        return denoise ? denoised_output() : trc_tonemap(ctx, rgba8.data(), &exposure);
    };
    if (denoise) {
        CHECK(trc_denoise_track_motion(ctx, 1));
        if (prm.flags & TRC_FLAG_CAMERA_RAYS) {      // rays in force: the G-buffer is walked along set 0 of them (with --aa the first Halton offset), not along the camera's ray
            CHECK(trc_denoise_guide_rays(ctx, 1));
            std::printf("denoiser guided by the camera rays (set 0)\n");
        }
        CHECK(denoised_output());
    } else {
        CHECK(trc_tonemap(ctx, rgba8.data(), &exposure));
    }
    if (trc_host_write_png(out.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
    std::printf("%s %ux%u %u spp %s: %llu rays, kernel %.2f ms (wall %.2f ms), %.1f Mrays/s, exposure %.4f -> %s\n",
                scene_name.c_str(), W, H, spp, integ_name.c_str(), (unsigned long long)st.rays, st.kernel_ms, wall_ms,
                st.rays / st.kernel_ms / 1e3, exposure, out.c_str());
    if (denoise) std::printf("frame 0%s\n", history_note.c_str());
    if (adaptive) {
        // the report, and every pixel's tile count as a grey value over the frame (rows top-down, as the frame's)
        const uint32_t tw = (W + TRC_TILE - 1) / TRC_TILE, th = (H + TRC_TILE - 1) / TRC_TILE;
        std::vector<uint32_t> n_t((size_t)tw * th);
        std::vector<float> e_t((size_t)tw * th);
        CHECK(trc_download_tile_samples(ctx, n_t.data()));
        CHECK(trc_download_tile_error(ctx, e_t.data()));
        std::vector<uint8_t> grey((size_t)W * H * 4);
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const uint32_t n = n_t[(size_t)((H - 1 - y) / TRC_TILE) * tw + x / TRC_TILE];
                uint8_t* px = &grey[((size_t)y * W + x) * 4];
                px[0] = px[1] = px[2] = (uint8_t)((255ull * n + ad.max_spp / 2) / ad.max_spp);
                px[3] = 255;
            }
        const std::string name = out + ".samples.png";
        if (trc_host_write_png(name.c_str(), grey.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
        std::vector<float> sorted = e_t;
        std::sort(sorted.begin(), sorted.end());
        std::printf("adaptive: threshold %g, first pass %u, max %u spp: %u passes, %llu samples (%.1f per pixel, %.1f %% of %u spp everywhere), "
                    "%u of %zu tiles still active, error median %g max %g -> %s\n",
                    ad.threshold, spp, ad.max_spp, report.passes, (unsigned long long)report.samples, (double)report.samples / ((double)W * H),
                    100.0 * (double)report.samples / ((double)W * H * ad.max_spp), ad.max_spp, report.active_tiles, n_t.size(), sorted[sorted.size() / 2],
                    report.max_error, name.c_str());
    }
    // --rebuild-ratio: the cost right after the last build is the yardstick; called after every animation call
    uint32_t rebuilds = 0, cost_reads = 0;
    double built_cost = 0.0;
    auto tree_ratio = [&](double* ratio) {
        trc_tree_cost_t c;
        const trc_status cs = trc_tree_cost(ctx, &c);
        if (cs == TRC_OK) *ratio = c.root_half_area > 0.0 ? (c.interior_half_area + c.leaf_half_area) / c.root_half_area : 0.0;
        return cs;
    };
    auto rebuild_if_worn = [&]() {
        if (rebuild_ratio == 0.0) return TRC_OK;
        double now = 0.0;
        trc_status rs = tree_ratio(&now);
        if (rs != TRC_OK) return rs;
        ++cost_reads;
        if (now <= rebuild_ratio * built_cost) return TRC_OK;
        const auto r0 = std::chrono::steady_clock::now();
        if ((rs = trc_rebuild_tree(ctx, TRC_TREE_SAH | (device_sah3 ? TRC_TREE_SAH3 : 0u))) != TRC_OK) return rs;      // the flavour of the upload
        const double rebuild_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();
        const double worn = now;
        if ((rs = tree_ratio(&now)) != TRC_OK) return rs;
        std::printf("tree cost %.3f > %.2f x %.3f: trc_rebuild_tree %.2f ms -> cost %.3f\n", worn, rebuild_ratio, built_cost, rebuild_ms, now);
        built_cost = now;
        ++rebuilds;
        return TRC_OK;
    };
    if (rebuild_ratio != 0.0) CHECK(tree_ratio(&built_cost));
    // --normals: called after every animation call, over the whole mesh.  The first call of a scene builds the vertex -> corner adjacency
    // and waits for it: that call is timed on the host with a trc_synchronize on each side, and what it took beyond its own kernels'
    // device time (trc_debug_refit_ms) is the build.  normals_note: what the animation's own line of output ends with
    uint32_t normal_calls = 0;
    std::string normals_note;
    auto recompute_normals = [&]() {
        if (!normals) return TRC_OK;
        trc_status rs;
        float device_ms = 0.0f;
        char text[160];
        if (normal_calls++ == 0) {
            if ((rs = trc_synchronize(ctx)) != TRC_OK) return rs;
            const auto n0 = std::chrono::steady_clock::now();
            if ((rs = trc_recompute_normals(ctx, 0, scene.n_vertex)) != TRC_OK || (rs = trc_synchronize(ctx)) != TRC_OK) return rs;
            const double first_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - n0).count();
            if ((rs = trc_debug_refit_ms(ctx, &device_ms)) != TRC_OK) return rs;
            std::printf("trc_recompute_normals, first call: %.2f ms between two trc_synchronize, %.3f ms of it its kernels, the rest the adjacency build "
                        "(%.1f KB kept on the device)\n", first_ms, device_ms, (4.0 * (scene.n_vertex + 1.0) + 4.0 * scene.n_index) / 1024.0);
        } else {
            if ((rs = trc_recompute_normals(ctx, 0, scene.n_vertex)) != TRC_OK || (rs = trc_debug_refit_ms(ctx, &device_ms)) != TRC_OK) return rs;
        }
        std::snprintf(text, sizeof text, ", trc_recompute_normals %.3f ms device", device_ms);
        normals_note = text;
        return TRC_OK;
    };
    if (spin && scene.n_vertex) {
        // the mesh's world-space vertices, turned about the vertical axis through the centre of their box; normals alike
        const std::vector<trc_TriangleVertex> rest(scene.triList, scene.triList + scene.n_vertex);
        std::vector<trc_TriangleVertex> turned(rest);
        float lo[3] = {rest[0].v[0], rest[0].v[1], rest[0].v[2]}, hi[3] = {lo[0], lo[1], lo[2]};
        for (const trc_TriangleVertex& q : rest)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], q.v[k]); hi[k] = std::max(hi[k], q.v[k]); }
        const float cx = 0.5f * (lo[0] + hi[0]), cz = 0.5f * (lo[2] + hi[2]);
        for (uint32_t f = 1; f <= spin; ++f) {
            const double a = 6.283185307179586 * f / spin;
            const float ca = (float)std::cos(a), sa = (float)std::sin(a);
            for (size_t i = 0; i < rest.size(); ++i) {
                const float x = rest[i].v[0] - cx, z = rest[i].v[2] - cz;
                turned[i].v[0] = cx + ca * x + sa * z; turned[i].v[2] = cz - sa * x + ca * z;
                turned[i].n[0] = ca * rest[i].n[0] + sa * rest[i].n[2]; turned[i].n[2] = -sa * rest[i].n[0] + ca * rest[i].n[2];
            }
            const auto u0 = std::chrono::steady_clock::now();
            CHECK(trc_update_vertices(ctx, turned.data(), 0, scene.n_vertex));
            const double update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
            CHECK(recompute_normals());
            CHECK(rebuild_if_worn());
            CHECK(animation_frame());
            const std::string name = out + "." + std::to_string(f) + ".png";
            if (trc_host_write_png(name.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
            std::printf("spin %u / %u: trc_update_vertices %.2f ms%s%s -> %s\n", f, spin, update_ms, normals_note.c_str(), history_note.c_str(), name.c_str());
        }
    } else if (spin) {
        std::fprintf(stderr, "--spin turns the mesh of a --mesh or --pbrt scene: this scene has no triangles\n");
    }
    if (pose && scene.n_vertex) {
        // the same turn about the vertical axis through the centre of the mesh's box, as T(c) * R_y(a) * T(-c): the device poses its
        // own rest copy of the vertices, so the host sends one trc_pose per frame and computes no vertex
        float lo[3] = {scene.triList[0].v[0], scene.triList[0].v[1], scene.triList[0].v[2]}, hi[3] = {lo[0], lo[1], lo[2]};
        for (uint32_t i = 0; i < scene.n_vertex; ++i)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], scene.triList[i].v[k]); hi[k] = std::max(hi[k], scene.triList[i].v[k]); }
        const float cx = 0.5f * (lo[0] + hi[0]), cz = 0.5f * (lo[2] + hi[2]);
        const uint32_t first_frame = spin;             // after --spin's frames, when both are given
        for (uint32_t f = 1; f <= pose; ++f) {
            const double a = 6.283185307179586 * f / pose;
            const float ca = (float)std::cos(a), sa = (float)std::sin(a);
            trc_pose p;
            std::memset(&p, 0, sizeof p);
            p.first = 0; p.count = scene.n_vertex;
            p.model_matrix.columns[0] = {ca, 0.0f, -sa, 0.0f};
            p.model_matrix.columns[1] = {0.0f, 1.0f, 0.0f, 0.0f};
            p.model_matrix.columns[2] = {sa, 0.0f, ca, 0.0f};
            p.model_matrix.columns[3] = {cx - ca * cx - sa * cz, 0.0f, cz + sa * cx - ca * cz, 1.0f};
            p.normal_matrix = p.model_matrix;          // a rotation is its own inverse transpose; the translation column is not read
            const auto u0 = std::chrono::steady_clock::now();
            CHECK(trc_pose_vertices(ctx, &p, 1));
            const double pose_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
            CHECK(recompute_normals());
            CHECK(rebuild_if_worn());
            CHECK(animation_frame());
            const std::string name = out + "." + std::to_string(first_frame + f) + ".png";
            if (trc_host_write_png(name.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
            std::printf("pose %u / %u: trc_pose_vertices %.2f ms%s%s -> %s\n", f, pose, pose_ms, normals_note.c_str(), history_note.c_str(), name.c_str());
        }
    } else if (pose) {
        std::fprintf(stderr, "--pose turns the mesh of a --mesh or --pbrt scene: this scene has no triangles\n");
    }
    if (bend && scene.n_vertex) {
        // two bones: bone 0 stays, bone 1 makes --pose's turn, and a vertex follows bone 1 by its height in the mesh's box -- the foot
        // stands, the top turns, what lies between is twisted.  The influences go up once; a frame sends 256 bytes of palette
        float lo[3] = {scene.triList[0].v[0], scene.triList[0].v[1], scene.triList[0].v[2]}, hi[3] = {lo[0], lo[1], lo[2]};
        for (uint32_t i = 0; i < scene.n_vertex; ++i)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], scene.triList[i].v[k]); hi[k] = std::max(hi[k], scene.triList[i].v[k]); }
        const float cx = 0.5f * (lo[0] + hi[0]), cz = 0.5f * (lo[2] + hi[2]), height = hi[1] - lo[1];
        std::vector<trc_skin_influence> influences(scene.n_vertex);
        for (uint32_t i = 0; i < scene.n_vertex; ++i) {
            const float up = height > 0.0f ? (scene.triList[i].v[1] - lo[1]) / height : 0.0f;
            influences[i] = {{0u, 1u, 0u, 0u}, {1.0f - up, up, 0.0f, 0.0f}};
        }
        CHECK(trc_skin_bind(ctx, influences.data(), 0, scene.n_vertex));
        const uint32_t first_frame = spin + pose;      // after --spin's and --pose's frames, when they are given too
        for (uint32_t f = 1; f <= bend; ++f) {
            const double a = 6.283185307179586 * f / bend;
            const float ca = (float)std::cos(a), sa = (float)std::sin(a);
            trc_skin_bone bones[2];
            std::memset(bones, 0, sizeof bones);
            for (int c = 0; c < 4; ++c) (&bones[0].model_matrix.columns[c].x)[c] = 1.0f;
            bones[0].normal_matrix = bones[0].model_matrix;
            bones[1].model_matrix.columns[0] = {ca, 0.0f, -sa, 0.0f};
            bones[1].model_matrix.columns[1] = {0.0f, 1.0f, 0.0f, 0.0f};
            bones[1].model_matrix.columns[2] = {sa, 0.0f, ca, 0.0f};
            bones[1].model_matrix.columns[3] = {cx - ca * cx - sa * cz, 0.0f, cz + sa * cx - ca * cz, 1.0f};
            bones[1].normal_matrix = bones[1].model_matrix;      // a rotation is its own inverse transpose; the translation column is not read
            const auto u0 = std::chrono::steady_clock::now();
            CHECK(trc_skin_vertices(ctx, bones, 2));
            const double skin_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
            CHECK(recompute_normals());
            CHECK(rebuild_if_worn());
            CHECK(animation_frame());
            const std::string name = out + "." + std::to_string(first_frame + f) + ".png";
            if (trc_host_write_png(name.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
            std::printf("bend %u / %u: trc_skin_vertices %.2f ms%s%s -> %s\n", f, bend, skin_ms, normals_note.c_str(), history_note.c_str(), name.c_str());
        }
    } else if (bend) {
        std::fprintf(stderr, "--bend bends the mesh of a --mesh or --pbrt scene: this scene has no triangles\n");
        trc_destroy(ctx);
        trc_host_scene_destroy(hs);
        trc_host_mesh_destroy(mesh);
        return 1;
    }
    if (morph && scene.n_vertex) {
        // two targets over the whole mesh, target-major: target 0 swells the mesh away from the vertical axis through the centre of its
        // box, target 1 presses it towards its foot; the normals keep their rest values (deltas of 0).  The table goes up once; a frame
        // sends two weights.  After --bend the skin binding is still there: every frame then goes through the fused call, the morph and
        // --bend's two bones on top of it
        float lo[3] = {scene.triList[0].v[0], scene.triList[0].v[1], scene.triList[0].v[2]}, hi[3] = {lo[0], lo[1], lo[2]};
        for (uint32_t i = 0; i < scene.n_vertex; ++i)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], scene.triList[i].v[k]); hi[k] = std::max(hi[k], scene.triList[i].v[k]); }
        const float cx = 0.5f * (lo[0] + hi[0]), cz = 0.5f * (lo[2] + hi[2]);
        std::vector<trc_morph_delta> deltas(2 * (size_t)scene.n_vertex);
        for (uint32_t i = 0; i < scene.n_vertex; ++i) {
            const float* q = scene.triList[i].v;
            deltas[i] = {{0.5f * (q[0] - cx), 0.0f, 0.5f * (q[2] - cz)}, {0.0f, 0.0f, 0.0f}};
            deltas[(size_t)scene.n_vertex + i] = {{0.0f, -0.5f * (q[1] - lo[1]), 0.0f}, {0.0f, 0.0f, 0.0f}};
        }
        CHECK(trc_morph_bind(ctx, deltas.data(), 2, 0, scene.n_vertex));
        const uint32_t first_frame = spin + pose + bend;      // after the other animations' frames, when they are given too
        for (uint32_t f = 1; f <= morph; ++f) {
            const double a = 6.283185307179586 * f / morph;
            const float weights[2] = {(float)std::sin(a), (float)(0.5 - 0.5 * std::cos(a))};      // swinging: -1..1 and 0..1
            const float ca = (float)std::cos(a), sa = (float)std::sin(a);
            trc_skin_bone bones[2];
            std::memset(bones, 0, sizeof bones);
            for (int c = 0; c < 4; ++c) (&bones[0].model_matrix.columns[c].x)[c] = 1.0f;
            bones[0].normal_matrix = bones[0].model_matrix;
            bones[1].model_matrix.columns[0] = {ca, 0.0f, -sa, 0.0f};
            bones[1].model_matrix.columns[1] = {0.0f, 1.0f, 0.0f, 0.0f};
            bones[1].model_matrix.columns[2] = {sa, 0.0f, ca, 0.0f};
            bones[1].model_matrix.columns[3] = {cx - ca * cx - sa * cz, 0.0f, cz + sa * cx - ca * cz, 1.0f};
            bones[1].normal_matrix = bones[1].model_matrix;
            const auto u0 = std::chrono::steady_clock::now();
            CHECK(trc_morph_vertices(ctx, weights, 2, bones, bend ? 2u : 0u));
            const double morph_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
            CHECK(recompute_normals());
            CHECK(rebuild_if_worn());
            CHECK(animation_frame());
            const std::string name = out + "." + std::to_string(first_frame + f) + ".png";
            if (trc_host_write_png(name.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
            std::printf("morph %u / %u: trc_morph_vertices%s %.2f ms%s%s -> %s\n", f, morph, bend ? " under two bones" : "", morph_ms, normals_note.c_str(), history_note.c_str(), name.c_str());
        }
    } else if (morph) {
        std::fprintf(stderr, "--morph morphs the mesh of a --mesh or --pbrt scene: this scene has no triangles\n");
        trc_destroy(ctx);
        trc_host_scene_destroy(hs);
        trc_host_mesh_destroy(mesh);
        return 1;
    }
    if (orbit && kind == TRC_SCENE_CORNELL_SPHERES && pbrt_path.empty() && scene.n_sphere) {
        // every sphere keeps its height and its distance from the vertical axis through (278, *, 278) and goes round it; the record is what
        // the scene builder makes for the new centre (the record's radius is the builder's argument + 1e-4: taken off again here)
        const std::vector<trc_Sphere> rest(scene.sphereList, scene.sphereList + scene.n_sphere);
        std::vector<trc_Sphere> moved(rest);
        const uint32_t first_frame = spin + pose + bend + morph;
        for (uint32_t f = 1; f <= orbit; ++f) {
            const double a = 6.283185307179586 * f / orbit;
            const float ca = (float)std::cos(a), sa = (float)std::sin(a);
            for (size_t i = 0; i < rest.size(); ++i) {
                const float x = rest[i].center.x - 278.0f, z = rest[i].center.z - 278.0f;
                const float c[3] = {278.0f + ca * x + sa * z, rest[i].center.y, 278.0f - sa * x + ca * z};
                trc_host_make_sphere(&moved[i], rest[i].radius - 0.0001f, c, rest[i].material);
            }
            trc_primitive_ranges r;
            std::memset(&r, 0, sizeof r);
            r.spheres = moved.data(); r.first_sphere = 0; r.n_sphere = scene.n_sphere;
            const auto u0 = std::chrono::steady_clock::now();
            CHECK(trc_update_primitives(ctx, &r));
            const double update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
            CHECK(rebuild_if_worn());
            CHECK(animation_frame());
            const std::string name = out + "." + std::to_string(first_frame + f) + ".png";
            if (trc_host_write_png(name.c_str(), rgba8.data(), W, H) != TRC_OK) { std::fprintf(stderr, "cannot write %s\n", name.c_str()); return 1; }
            std::printf("orbit %u / %u: trc_update_primitives %.2f ms%s -> %s\n", f, orbit, update_ms, history_note.c_str(), name.c_str());
        }
    } else if (orbit) {
        std::fprintf(stderr, "--orbit moves the spheres of --scene spheres: this scene's tree holds none\n");
        trc_destroy(ctx);
        trc_host_scene_destroy(hs);
        trc_host_mesh_destroy(mesh);
        return 1;
    }
    if (rebuild_ratio != 0.0) std::printf("rebuild-ratio %.2f: %u rebuilds after %u animation calls\n", rebuild_ratio, rebuilds, cost_reads);
    trc_destroy(ctx);
    trc_host_scene_destroy(hs);
    trc_host_mesh_destroy(mesh);
    return 0;
}
