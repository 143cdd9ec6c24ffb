// tools/sanitize/driver.cpp -- the CPU half of the repository (libtrc_host sources + the oracle, which is test
// infrastructure) as ONE program for the sanitizers: `make asan` / `make tsan` compile the sources themselves with
// -fsanitize=address,undefined / -fsanitize=thread (no Python in the process, so no interposer noise), and this driver
// runs what the threaded and the parsing code paths do:
//   1. scene assembly + the multi-threaded SAH build on a 150 k-triangle mesh (host/bvh_builder.cpp, the GCD build of
//      BVH.hh:35-244 restated with std::thread), tree depth, a second build in parallel from another thread
//   2. the oracle's row-band workers: tracePath / traceMIS / traceVolume frames with 8 threads, the SPPM pass, LBVH
//   3. every file reader on well-formed files it writes itself (pbrt scene with plymesh / disk / cylinder / texture, PLY in
//      three encodings, OBJ, pbrt density, Radiance .hdr), then on `--fuzz N` mutations of each: a reader must return a
//      status, never crash, over-read or leak
//   4. the range check of trc_pose_vertices (tracer_amd/csrc/pose_ranges.hpp, host code of the HIP library that includes nothing of
//      HIP) on hostile tables: first + count wrapping past 2^32, equal ranges, a table of one, non-finite matrix entries
//   5. the checks of trc_skin_bind and trc_skin_vertices (tracer_amd/csrc/skin_check.hpp, HIP-free like pose_ranges.hpp) on hostile
//      influence tables and palettes: NULL with a count, a range that wraps, non-finite weights, a bone index at the bound, a palette
//      one bone too small, NaN in entries that are read and in entries that are not
//   6. the checks of trc_morph_bind and trc_morph_vertices (tracer_amd/csrc/morph_check.hpp, HIP-free as well) on hostile delta tables
//      and weights: NULL with a non-empty table, a range that wraps, non-finite deltas at the table's end, n_targets beyond the cap, a
//      weight count off by one, non-finite weights, all-zero weights, and the compaction of the weights into the active list
//   7. the range check of trc_recompute_normals (tracer_amd/csrc/normals_check.hpp, HIP-free too): the off-by-one, a range that wraps,
//      the empty range, and the key bits of the adjacency build's sort at the powers of two
//   8. the checks of trc_update_primitives (tracer_amd/csrc/primitives_check.hpp, HIP-free too) on hostile ranges and records, built by the
//      host helpers (trc_host_make_sphere / _square / _cube): NULL with a count, first + n that wraps, a material and an axis at the
//      bound, NaN / infinity / 2e37 in fields that are read and NaN in fields that are not; lists exactly as long as their count
// "build host code under -fsanitize=thread,address".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "tracer_abi.h"
#include "../../oracle/oracle.h"
#include "../../tracer_amd/csrc/pose_ranges.hpp"
#include "../../tracer_amd/csrc/skin_check.hpp"
#include "../../tracer_amd/csrc/morph_check.hpp"
#include "../../tracer_amd/csrc/normals_check.hpp"
#include "../../tracer_amd/csrc/primitives_check.hpp"

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "EXPECT failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static void write_file(const std::string& p, const std::string& data) {
    FILE* f = std::fopen(p.c_str(), "wb");
    if (!f) { std::perror(p.c_str()); std::exit(2); }
    std::fwrite(data.data(), 1, data.size(), f);
    std::fclose(f);
}
static std::string read_file(const std::string& p) {
    FILE* f = std::fopen(p.c_str(), "rb");
    std::string s;
    if (!f) return s;
    char buf[65536]; size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    std::fclose(f);
    return s;
}

static void build_and_render(bool second_thread) {
    trc_host_mesh *ball = nullptr, *many = nullptr;
    EXPECT(trc_host_mesh_make_ball(80, 80, 0.07f, &ball) == TRC_OK);
    EXPECT(trc_host_mesh_replicate(ball, second_thread ? 2 : 3, 2.4f, &many) == TRC_OK);     // 12 800 x 9 = 115 200 triangles
    const trc_TriangleVertex* v; const uint32_t* idx; uint32_t nv, ni;
    trc_host_mesh_view(many, &v, &nv, &idx, &ni);
    trc_host_scene* hs = nullptr;
    EXPECT(trc_host_scene_create(TRC_SCENE_CORNELL_MESH, v, nv, idx, ni, &hs) == TRC_OK);
    trc_scene sc;
    trc_host_scene_view(hs, &sc);
    uint32_t depth = 0;
    EXPECT(trc_host_tree_depth(sc.bvhList, sc.n_bvh, &depth) == TRC_OK && depth > 10 && depth <= TRC_MAX_BVH_DEPTH);
    if (!second_thread) {
        // the oracle on that scene: 8 row-band workers, all three integrators
        const uint32_t W = 48, H = 32;
        trc_Camera cam;
        trc_host_prepare_camera(&cam, (float)W, (float)H);
        const float env[3] = {0.1f, 0.2f, 0.3f};
        for (uint32_t integ = 0; integ < 3; ++integ) {
            std::vector<uint32_t> rng((size_t)W * H * 4);
            std::vector<float> acc((size_t)W * H * 4, 0.0f), acc1((size_t)W * H * 4, 0.0f);
            trc_host_fill_rng(7, W, H, rng.data());
            std::vector<uint32_t> rng1 = rng;
            trc_params prm; std::memset(&prm, 0, sizeof prm);
            prm.spp = 2; prm.max_depth = 8; prm.integrator = integ; prm.tile_nranks = 1;
            trc_stats st, st1;                     // orc_render ADDS to the counters
            std::memset(&st, 0, sizeof st); std::memset(&st1, 0, sizeof st1);
            orc_render(&sc, &cam, env, W, H, rng.data(), acc.data(), &prm, &st, 8);
            orc_render(&sc, &cam, env, W, H, rng1.data(), acc1.data(), &prm, &st1, 1);
            EXPECT(st.rays == st1.rays);                                                  // thread-count independent
            size_t diff = 0;
            for (size_t k = 0; k < acc.size(); ++k) diff += std::memcmp(&acc[k], &acc1[k], 4) != 0;
            if (diff || st.rays != st1.rays) std::fprintf(stderr, "integrator %u: rays %llu vs %llu, %zu of %zu accumulator words differ\n", integ,
                                                          (unsigned long long)st.rays, (unsigned long long)st1.rays, diff, acc.size());
            EXPECT(diff == 0);
        }
        // the oracle's statement of the project's own features (oracle.h): random per-triangle materials with emitters among them, an
        // image on every non-emitter material, then traceMIS with the environment map and with the mesh's triangles as lights, 8 workers
        {
            const uint32_t n_tri = sc.n_index / 3;
            std::vector<uint32_t> tri_mat(n_tri);
            for (uint32_t t = 0; t < n_tri; ++t) tri_mat[t] = (t * 2654435761u >> 8) % sc.n_material;
            std::vector<trc_Material> mats(sc.materials, sc.materials + sc.n_material);
            std::vector<float> texels(3 * 5 * 3), map(3 * 16 * 8, 0.0f);
            for (size_t k = 0; k < texels.size(); ++k) texels[k] = (float)(k % 7) / 7.0f;
            for (size_t k = 0; k < map.size(); ++k) map[k] = k % 5 == 0 ? 0.0f : (float)(k % 11);
            const trc_image img = {5, 3, texels.data()};
            for (auto& m : mats) if (m.type != TRC_MAT_DIFFUSE) { m.textureInfo.type = TRC_TEX_IMAGE; m.textureInfo.textureIndex = 0; }
            trc_scene tex = sc;
            tex.materials = mats.data();
            orc_set_triangle_materials(tri_mat.data(), n_tri);
            orc_set_textures(&img, 1);
            orc_set_environment_map(16, 8, map.data());
            for (uint32_t flag : {(uint32_t)TRC_FLAG_ENV_LIGHT, (uint32_t)TRC_FLAG_MESH_LIGHTS}) {
                std::vector<uint32_t> rng((size_t)W * H * 4);
                std::vector<float> acc((size_t)W * H * 4, 0.0f);
                trc_host_fill_rng(11, W, H, rng.data());
                trc_params prm; std::memset(&prm, 0, sizeof prm);
                prm.spp = 4; prm.max_depth = 8; prm.integrator = TRC_INTEGRATOR_MIS; prm.tile_nranks = 1; prm.flags = flag;
                trc_stats st; std::memset(&st, 0, sizeof st);
                orc_render(&tex, &cam, env, W, H, rng.data(), acc.data(), &prm, &st, 8);
                EXPECT(st.paths == (uint64_t)W * H * 4 && st.rays > st.paths);
            }
            uint64_t visits[ORC_BRANCH_COUNT];
            orc_debug_branch_counts(visits, 1);
            EXPECT(visits[ORC_BR_PICK_LIGHT] > 0 && visits[ORC_BR_SUPPORT] > 0);
            orc_set_triangle_materials(nullptr, 0); orc_set_textures(nullptr, 0); orc_set_environment_map(0, 0, nullptr);
        }
        // LBVH oracle on the leaves
        const uint32_t n_leaves = (sc.n_bvh + 1) / 2;
        std::vector<trc_BVH> out(2 * (size_t)n_leaves - 1);
        uint32_t h = 0;
        orc_lbvh_build(sc.bvhList + 1, n_leaves, out.data(), &h);
        EXPECT(h > 10);
    }
    trc_host_scene_destroy(hs);
    trc_host_mesh_destroy(many);
    trc_host_mesh_destroy(ball);
}

static void sppm_pass() {
    trc_host_scene* hs = nullptr;
    EXPECT(trc_host_scene_create(TRC_SCENE_CORNELL_SPHERES, nullptr, 0, nullptr, 0, &hs) == TRC_OK);
    trc_scene sc; trc_host_scene_view(hs, &sc);
    const uint32_t W = 40, H = 24;
    trc_Camera cam; trc_host_prepare_camera(&cam, (float)W, (float)H);
    std::vector<uint32_t> rng((size_t)W * H * 4);
    std::vector<float> acc((size_t)W * H * 4, 0.0f);
    trc_host_fill_rng(3, W, H, rng.data());
    const float env[3] = {0, 0, 0};
    orc_sppm* s = orc_sppm_create(W, H, 5);
    orc_sppm_frames(s, &sc, &cam, env, rng.data(), acc.data(), 2);
    trc_Complex cx;
    orc_sppm_download(s, nullptr, nullptr, nullptr, nullptr, &cx);
    EXPECT(cx.frame_count == 2);
    orc_sppm_destroy(s);
    std::vector<uint8_t> rgba8((size_t)W * H * 4);
    float expose = 0;
    orc_tonemap(acc.data(), W, H, rgba8.data(), &expose);
    trc_host_scene_destroy(hs);
}

// ---------------------------------------------------------------- trc_pose_vertices' table check
static trc_pose make_pose(uint32_t first, uint32_t count) {
    trc_pose p; std::memset(&p, 0, sizeof p);
    p.first = first; p.count = count;
    for (int c = 0; c < 4; ++c) { float* m = &p.model_matrix.columns[c].x; float* n = &p.normal_matrix.columns[c].x; m[c] = n[c] = 1.0f; }
    return p;
}
static void pose_tables() {
    const uint32_t n_vertex = 1000;
    std::vector<uint32_t> order;
    auto ok = [&](const std::vector<trc_pose>& t) { return trc_pose_table_check(t.data(), (uint32_t)t.size(), n_vertex, order) == nullptr; };
    EXPECT(trc_pose_table_check(nullptr, 0, n_vertex, order) == nullptr && order.empty());
    EXPECT(trc_pose_table_check(nullptr, 3, n_vertex, order) != nullptr);
    EXPECT(ok({make_pose(0, 1000)}) && order.size() == 1);                                     // n_poses of 1, the whole array
    EXPECT(ok({make_pose(999, 1)}) && !ok({make_pose(1000, 1)}) && !ok({make_pose(999, 2)}));
    EXPECT(!ok({make_pose(0, 0)}) && !ok({make_pose(5, 3), make_pose(9, 0)}));
    EXPECT(!ok({make_pose(0xFFFFFFFFu, 2)}) && !ok({make_pose(2, 0xFFFFFFFFu)}) && !ok({make_pose(0xFFFFFF00u, 0x200u)}));   // first + count wraps
    EXPECT(!ok({make_pose(10, 5), make_pose(10, 5)}));                                         // equal ranges
    EXPECT(!ok({make_pose(10, 5), make_pose(14, 1)}) && !ok({make_pose(14, 3), make_pose(0, 15)}) && !ok({make_pose(0, 1000), make_pose(500, 1)}));
    EXPECT(ok({make_pose(500, 500), make_pose(10, 5), make_pose(0, 10), make_pose(15, 485)}));  // unsorted, back to back, up to the end
    EXPECT(order.size() == 4 && order[0] == 2 && order[1] == 1 && order[2] == 3 && order[3] == 0);
    trc_pose bad = make_pose(0, 10);
    bad.model_matrix.columns[3].y = NAN;
    EXPECT(!ok({bad}));
    bad = make_pose(0, 10); bad.normal_matrix.columns[2].z = INFINITY;
    EXPECT(!ok({bad}));
    bad = make_pose(0, 10); bad.model_matrix.columns[1].w = NAN; bad.normal_matrix.columns[3].x = INFINITY;      // lanes that are not read
    EXPECT(ok({bad}));
    // a large table of unit ranges in reverse order, and the same with one duplicate in the middle
    std::vector<trc_pose> many;
    for (uint32_t i = 0; i < n_vertex; ++i) many.push_back(make_pose(n_vertex - 1 - i, 1));
    EXPECT(ok(many) && order.front() == n_vertex - 1 && order.back() == 0);
    many[n_vertex / 2].first = 3;
    EXPECT(!ok(many));
}

// ---------------------------------------------------------------- trc_skin_bind's and trc_skin_vertices' checks
static trc_skin_bone make_bone() {
    trc_skin_bone b; std::memset(&b, 0, sizeof b);
    for (int c = 0; c < 4; ++c) { (&b.model_matrix.columns[c].x)[c] = 1.0f; (&b.normal_matrix.columns[c].x)[c] = 1.0f; }
    return b;
}
static void skin_tables() {
    const uint32_t n_vertex = 1000;
    uint32_t max_bone = 77;
    std::vector<trc_skin_influence> t(10);
    for (uint32_t i = 0; i < t.size(); ++i) t[i] = {{i, 2u * i, 0u, 3u}, {0.5f, 0.25f, 0.0f, -0.125f}};
    auto ok = [&](uint32_t first, uint32_t count) { return trc_skin_influence_check(t.data(), first, count, n_vertex, &max_bone) == nullptr; };
    EXPECT(trc_skin_influence_check(nullptr, 5, 0, n_vertex, &max_bone) == nullptr && max_bone == 0);      // count == 0: NULL is fine
    max_bone = 77;
    EXPECT(trc_skin_influence_check(nullptr, 0, 3, n_vertex, &max_bone) != nullptr && max_bone == 77);     // NULL with a count; nothing written
    EXPECT(ok(0, 10) && max_bone == 18);
    EXPECT(ok(990, 10) && !ok(991, 10) && !ok(1000, 1) && !ok(1001, 0xFFFFFFFFu));
    EXPECT(!ok(0xFFFFFFFFu, 2) && !ok(2, 0xFFFFFFFFu) && !ok(0xFFFFFF00u, 0x200u));                        // first + count wraps
    for (const float bad : {NAN, INFINITY, -INFINITY}) {
        t[7].weight[3] = bad;
        EXPECT(!ok(0, 10) && ok(0, 7));
        t[7].weight[3] = -0.125f;
    }
    t[9].bone[2] = TRC_SKIN_MAX_BONES;                                                                     // refused whatever its weight (0)
    EXPECT(!ok(0, 10) && ok(0, 9));
    t[9].bone[2] = TRC_SKIN_MAX_BONES - 1;
    max_bone = 77;
    EXPECT(ok(0, 10) && max_bone == TRC_SKIN_MAX_BONES - 1);
    // palettes
    std::vector<trc_skin_bone> pal(19, make_bone());
    auto pal_ok = [&](uint32_t n_bones, uint32_t largest) { return trc_skin_palette_check(pal.data(), n_bones, largest) == nullptr; };
    EXPECT(trc_skin_palette_check(nullptr, 19, 18) != nullptr);
    EXPECT(pal_ok(19, 18) && !pal_ok(18, 18) && pal_ok(1, 0) && !pal_ok(19, 19));                          // n_bones one too small
    EXPECT(trc_skin_palette_check(pal.data(), TRC_SKIN_MAX_BONES + 1, 18) != nullptr);                     // refused before a bone is read
    EXPECT(trc_skin_palette_check(pal.data(), 0xFFFFFFFFu, 18) != nullptr);
    pal[18].model_matrix.columns[3].y = NAN;
    EXPECT(!pal_ok(19, 18) && !pal_ok(19, 3));                                                             // a bone that no vertex names counts
    pal[18] = make_bone(); pal[0].normal_matrix.columns[2].z = INFINITY;
    EXPECT(!pal_ok(19, 18));
    pal[0] = make_bone(); pal[5].model_matrix.columns[1].w = NAN; pal[5].normal_matrix.columns[3].x = INFINITY; pal[5].normal_matrix.columns[0].w = NAN;
    EXPECT(pal_ok(19, 18));                                                                                // lanes that are not read
}

// ---------------------------------------------------------------- trc_morph_bind's and trc_morph_vertices' checks
static void morph_tables() {
    const uint32_t n_vertex = 1000;
    std::vector<trc_morph_delta> t(3 * 10);                                                                // three targets over ten vertices
    for (uint32_t r = 0; r < t.size(); ++r) t[r] = {{0.5f * r, -1.0f, 0.0f}, {0.0f, 0.25f, -0.125f * r}};
    auto ok = [&](uint32_t n_targets, uint32_t first, uint32_t count) { return trc_morph_table_check(t.data(), n_targets, first, count, n_vertex) == nullptr; };
    EXPECT(trc_morph_table_check(nullptr, 3, 5, 0, n_vertex) == nullptr && trc_morph_table_check(nullptr, 0, 5, 7, n_vertex) == nullptr);      // empty: NULL is fine
    EXPECT(trc_morph_table_check(nullptr, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, n_vertex) == nullptr);              // ... and nothing else is looked at
    EXPECT(trc_morph_table_check(nullptr, 3, 0, 10, n_vertex) != nullptr);                                 // NULL with a non-empty table
    EXPECT(ok(3, 0, 10) && ok(3, 990, 10) && !ok(3, 991, 10) && !ok(1, 1000, 1) && !ok(1, 1001, 0xFFFFFFFFu));
    EXPECT(!ok(1, 0xFFFFFFFFu, 2) && !ok(1, 2, 0xFFFFFFFFu) && !ok(1, 0xFFFFFF00u, 0x200u));                // first + count wraps
    EXPECT(!ok(TRC_MORPH_MAX_TARGETS + 1, 0, 10) && !ok(0xFFFFFFFFu, 0, 10));                              // beyond the cap: refused before a delta is read
    for (const float bad : {NAN, INFINITY, -INFINITY}) {
        t[2 * 10 + 7].dv[1] = bad;                                                                         // target 2, vertex 7
        EXPECT(!ok(3, 0, 10) && ok(2, 0, 10) && ok(1, 0, 30 - 3));                                         // (one target over the first 27 records)
        t[2 * 10 + 7].dv[1] = -1.0f;
        t[29].dn[2] = bad;                                                                                 // the last component of the table
        EXPECT(!ok(3, 0, 10) && ok(3, 0, 9) && ok(1, 0, 29));
        t[29].dn[2] = 0.0f;
    }
    {   // the cap itself is legal: 1024 targets over one vertex
        std::vector<trc_morph_delta> wide(TRC_MORPH_MAX_TARGETS);
        std::memset(wide.data(), 0, wide.size() * sizeof(trc_morph_delta));
        EXPECT(trc_morph_table_check(wide.data(), TRC_MORPH_MAX_TARGETS, 999, 1, n_vertex) == nullptr);
    }
    // weights, and their compaction into the active list
    std::vector<trc_morph_active> active(5, trc_morph_active{7u, 1.0f});
    const float w[6] = {0.5f, 0.0f, -0.25f, -0.0f, 1e-45f, 0.0f};
    EXPECT(trc_morph_weights_check(nullptr, 6, 6, active) != nullptr && active.empty());
    EXPECT(trc_morph_weights_check(w, 5, 6, active) != nullptr && trc_morph_weights_check(w, 6, 5, active) != nullptr && active.empty());      // off by one, either way
    EXPECT(trc_morph_weights_check(w, 6, 6, active) == nullptr && active.size() == 3);
    EXPECT(active.size() == 3 && active[0].target == 0 && active[0].weight == 0.5f && active[1].target == 2 && active[1].weight == -0.25f &&
           active[2].target == 4 && active[2].weight == 1e-45f);                                           // a denormal is not zero; +0 and -0 are
    const float zeros[4] = {0.0f, -0.0f, 0.0f, -0.0f};
    EXPECT(trc_morph_weights_check(zeros, 4, 4, active) == nullptr && active.empty());                     // all zero: accepted, nothing active
    for (const float bad : {NAN, INFINITY, -INFINITY}) {
        float v[6]; std::memcpy(v, w, sizeof v); v[5] = bad;
        EXPECT(trc_morph_weights_check(v, 6, 6, active) != nullptr && active.empty());
        EXPECT(trc_morph_weights_check(v, 5, 5, active) == nullptr && active.size() == 3);                 // ... which lies past the weights that are read
    }
    std::vector<float> all(TRC_MORPH_MAX_TARGETS, 0.125f);
    EXPECT(trc_morph_weights_check(all.data(), TRC_MORPH_MAX_TARGETS, TRC_MORPH_MAX_TARGETS, active) == nullptr && active.size() == TRC_MORPH_MAX_TARGETS &&
           active.back().target == TRC_MORPH_MAX_TARGETS - 1);
}

// ---------------------------------------------------------------- trc_recompute_normals' checks
static void normals_ranges() {
    EXPECT(trc_normals_range_check(0, 10, 10) == nullptr && trc_normals_range_check(3, 7, 10) == nullptr && trc_normals_range_check(9, 1, 10) == nullptr);
    EXPECT(trc_normals_range_check(0, 11, 10) != nullptr && trc_normals_range_check(3, 8, 10) != nullptr && trc_normals_range_check(10, 1, 10) != nullptr);      // off by one
    EXPECT(trc_normals_range_check(0xFFFFFFFFu, 1, 10) != nullptr && trc_normals_range_check(2, 0xFFFFFFFFu, 10) != nullptr);                                   // first + count wraps
    EXPECT(trc_normals_range_check(0xFFFFFFFFu, 2, 0xFFFFFFFFu) != nullptr && trc_normals_range_check(0xFFFFFFFEu, 1, 0xFFFFFFFFu) == nullptr);
    EXPECT(trc_normals_range_check(0, 0, 10) == nullptr && trc_normals_range_check(10, 0, 10) == nullptr && trc_normals_range_check(0xFFFFFFFFu, 0, 10) == nullptr);  // empty
    EXPECT(trc_normals_key_bits(0) == 1 && trc_normals_key_bits(1) == 1 && trc_normals_key_bits(2) == 1 && trc_normals_key_bits(3) == 2);
    EXPECT(trc_normals_key_bits(256) == 8 && trc_normals_key_bits(257) == 9 && trc_normals_key_bits(2601) == 12 && trc_normals_key_bits(0xFFFFFFFFu) == 32);
}

// ---------------------------------------------------------------- trc_update_primitives' checks
static void primitive_ranges() {
    const uint32_t big = 0xFFFFFFFFu, n_material = 20;
    const float centre[3] = {200.0f, 250.0f, 200.0f};
    trc_float4x4 model;
    std::memset(&model, 0, sizeof model);
    model.columns[0].x = 165.0f; model.columns[1].y = 330.0f; model.columns[2].z = 165.0f; model.columns[3] = {265.0f, 1.0f, 295.0f, 1.0f};
    // heap arrays exactly as long as the counts: a check that reads one record too many is an overflow the sanitizer sees
    std::vector<trc_Sphere> sp(3); std::vector<trc_Square> sq(2); std::vector<trc_Cube> cb(1);
    for (size_t i = 0; i < sp.size(); ++i) trc_host_make_sphere(&sp[i], 40.0f + (float)i, centre, 7u + (uint32_t)i);
    for (size_t i = 0; i < sq.size(); ++i) trc_host_make_square(&sq[i], 0, 400.0f, 555.0f, 2, 200.0f, 355.0f, 1, 554.9f, 3);
    trc_host_make_cube(&cb[0], 0, &model);
    EXPECT(cb[0].inverse_matrix.columns[0].x == 1.0f / 165.0f && cb[0].normal_matrix.columns[1].y == cb[0].inverse_matrix.columns[1].y);
    auto check = [&](const trc_primitive_ranges& r, uint32_t ns = 12, uint32_t nq = 7, uint32_t nc = 3) { return trc_primitive_ranges_check(&r, ns, nq, nc, n_material); };
    trc_primitive_ranges all{sp.data(), 9, 3, sq.data(), 5, 2, cb.data(), 2, 1};
    EXPECT(check(all) == nullptr);
    EXPECT(trc_primitive_ranges_check(nullptr, 12, 7, 3, n_material) != nullptr);
    trc_primitive_ranges none{};
    EXPECT(check(none) == nullptr && check(none, 0, 0, 0) == nullptr);
    none.first_sphere = none.first_square = none.first_cube = big;                      // n == 0: the range names nothing
    EXPECT(check(none) == nullptr);
    { trc_primitive_ranges r = all; r.spheres = nullptr; EXPECT(check(r) != nullptr); }
    { trc_primitive_ranges r = all; r.squares = nullptr; EXPECT(check(r) != nullptr); }
    { trc_primitive_ranges r = all; r.cubes = nullptr; EXPECT(check(r) != nullptr); }
    for (uint32_t first : {10u, 12u, big, big - 1u, big - 2u}) { trc_primitive_ranges r = all; r.first_sphere = first; EXPECT(check(r) != nullptr); }
    for (uint32_t first : {6u, 7u, big, big - 1u}) { trc_primitive_ranges r = all; r.first_square = first; EXPECT(check(r) != nullptr); }
    for (uint32_t first : {3u, big}) { trc_primitive_ranges r = all; r.first_cube = first; EXPECT(check(r) != nullptr); }
    EXPECT(check(all, 11) != nullptr && check(all, 12, 6) != nullptr && check(all, 12, 7, 2) != nullptr && check(all, 0, 0, 0) != nullptr);
    // a record at the end of each list spoilt in turn, and put right again
    const float bad[] = {std::nanf(""), INFINITY, -INFINITY, 2e37f, -2e37f};
    auto spoil = [&](float& field, const char* what) {
        const float keep = field;
        for (float b : bad) { field = b; EXPECT(check(all) != nullptr); }
        field = 1e37f; EXPECT(check(all) == nullptr);
        field = keep;
        if (check(all) != nullptr) { std::fprintf(stderr, "primitive_ranges: %s did not recover\n", what); ++g_fail; }
    };
    spoil(sp.back().radius, "radius"); spoil(sp.back().center.z, "center"); spoil(sp.back().boundingBOX.mini.y, "sphere box"); spoil(sp.back().model_matrix.columns[3].x, "sphere model");
    spoil(sq.back().range_i.x, "range_i"); spoil(sq.back().range_j.y, "range_j"); spoil(sq.back().value_k, "value_k"); spoil(sq.back().boundingBOX.maxi.z, "square box");
    spoil(sq.back().model_matrix.columns[0].y, "square model");
    spoil(cb.back().inverse_matrix.columns[3].z, "inverse"); spoil(cb.back().model_matrix.columns[2].x, "model"); spoil(cb.back().normal_matrix.columns[2].z, "normal");
    spoil(cb.back().box.maxi.x, "cube box");
    sp.back().inverse_matrix.columns[1].y = std::nanf(""); sq.back().normal_matrix.columns[0].x = INFINITY; cb.back().normal_matrix.columns[3].x = std::nanf("");
    cb.back().model_matrix.columns[1].w = std::nanf("");                             // fields nobody reads
    EXPECT(check(all) == nullptr);
    sp.back().material = n_material; EXPECT(check(all) != nullptr); sp.back().material = n_material - 1; EXPECT(check(all) == nullptr);
    sq.back().material = big; EXPECT(check(all) != nullptr); sq.back().material = 0;
    cb.back().material = n_material; EXPECT(check(all) != nullptr); cb.back().material = 0;
    for (uint8_t* axis : {&sq.back().axis_i, &sq.back().axis_j, &sq.back().axis_k}) { const uint8_t keep = *axis; *axis = 3; EXPECT(check(all) != nullptr); *axis = 255; EXPECT(check(all) != nullptr); *axis = keep; }
    EXPECT(check(all) == nullptr);
}

// ---------------------------------------------------------------- trc_host_build_tree_flags
static void flagged_trees() {
    // a heap array of exactly 2n - 1 records: a builder that writes one record too many is an overflow the sanitizer sees
    const uint32_t sizes[] = {2, 3, 5, 64, 65, 300};
    for (uint32_t n : sizes)
        for (int family = 0; family < 3; ++family)
            for (uint32_t flags : {(uint32_t)TRC_TREE_SAH, (uint32_t)(TRC_TREE_SAH | TRC_TREE_SAH3)}) {
                std::vector<trc_BVH> nodes(2 * n - 1);
                std::memset(nodes.data(), 0, sizeof(trc_BVH) * nodes.size());
                uint32_t s = 12345u + n;
                auto next = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); };
                for (uint32_t i = 0; i < n; ++i) {
                    // 0: random boxes; 1: identical centroids (the median fallback); 2: centroids on a line along y
                    const float c[3] = {family == 0 ? 100.0f * next() : 3.0f, family == 1 ? 3.0f : 100.0f * next(), family == 0 ? 100.0f * next() : 3.0f};
                    const float h = family == 0 ? 0.1f + next() : 0.25f * (float)(1 + i % 7);
                    nodes[i].pType = TRC_PRIM_SPHERE; nodes[i].pIndex = i;
                    nodes[i].bBOX.mini = {c[0] - h, c[1] - h, c[2] - h}; nodes[i].bBOX.maxi = {c[0] + h, c[1] + h, c[2] + h};
                }
                uint32_t count = 0, depth = 0;
                EXPECT(trc_host_build_tree_flags(nodes.data(), n, flags, &count) == TRC_OK && count == 2 * n - 1);
                EXPECT(trc_host_tree_depth(nodes.data(), count, &depth) == TRC_OK && depth >= 1);
            }
    trc_BVH two[3];
    std::memset(two, 0, sizeof two);
    for (uint32_t flags : {0u, (uint32_t)TRC_TREE_SAH3, 4u, 8u, (uint32_t)TRC_TREE_TRIANGLE_LEAVES}) EXPECT(trc_host_build_tree_flags(two, 2, flags, nullptr) == TRC_ERR_INVALID_ARG);
}

// ---------------------------------------------------------------- readers
static const char* kScene =
    "LookAt 0 3 -12  0 1 0  0 1 0\nCamera \"perspective\" \"float fov\" [ 40 ]\nFilm \"image\" \"integer xresolution\" [ 64 ] \"integer yresolution\" [ 48 ]\n"
    "WorldBegin\nAttributeBegin\n AreaLightSource \"diffuse\" \"rgb L\" [ 9 9 8 ]\n"
    " Shape \"trianglemesh\" \"integer indices\" [ 0 1 2 0 2 3 ] \"point P\" [ -3 8 -3  3 8 -3  3 8 3  -3 8 3 ]\nAttributeEnd\n"
    "Texture \"tiles\" \"spectrum\" \"checkerboard\" \"rgb tex1\" [ 0.9 0.5 0.1 ]\nMakeNamedMaterial \"m\" \"string type\" \"glass\"\n"
    "Material \"matte\" \"texture Kd\" \"tiles\"\nShape \"sphere\" \"float radius\" 1.5\nNamedMaterial \"m\"\n"
    "AttributeBegin\n Translate 2.5 0 0 Rotate -90 1 0 0\n Shape \"cylinder\" \"float radius\" 1.2 \"float zmin\" 0 \"float zmax\" 2.5 \"float phimax\" 200\n"
    " Shape \"disk\" \"float radius\" 1.2 \"float innerradius\" 0.3\n Shape \"plymesh\" \"string filename\" \"mesh.ply\"\nAttributeEnd\n"
    "Include \"medium.pbrt\"\nWorldEnd\n";
static const char* kMedium =
    "MakeNamedMedium \"smoke\" \"string type\" \"heterogeneous\" \"integer nx\" 2 \"integer ny\" 2 \"integer nz\" 2\n \"float density\" [ 0 1 .5 .25 1 1 0 0 ]\n";
static const char* kObj = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvn 0 0 1\nf 1/1/1 2/2/1 3/1/1 4/2/1\nf -4 -3 -2\n";

static std::string make_ply(int fmt) {      // 0 ascii, 1 little, 2 big endian
    const float P[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0.2f}, {0, 1, 0}};
    std::string s = "ply\nformat ";
    s += fmt == 0 ? "ascii" : fmt == 1 ? "binary_little_endian" : "binary_big_endian";
    s += " 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty uchar c\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n";
    auto put = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < n; ++k) s.push_back((char)b[fmt == 2 ? n - 1 - k : k]); };
    if (fmt == 0) { for (auto& p : P) { char l[96]; std::snprintf(l, sizeof l, "%g %g %g 7\n", p[0], p[1], p[2]); s += l; } s += "3 0 1 2\n4 0 1 2 3\n"; }
    else {
        for (auto& p : P) { for (float f : p) put(&f, 4); s.push_back(7); }
        const int tri[3] = {0, 1, 2}, quad[4] = {0, 1, 2, 3};
        s.push_back(3); for (int i : tri) put(&i, 4);
        s.push_back(4); for (int i : quad) put(&i, 4);
    }
    return s;
}
static std::string make_hdr() {
    std::string s = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 3 +X 10\n";
    for (int y = 0; y < 3; ++y) {
        s += std::string("\x02\x02\x00\x0a", 4);
        for (int c = 0; c < 4; ++c) { s.push_back((char)(128 + 6)); s.push_back((char)(40 * c + y)); s.push_back((char)4); for (int k = 0; k < 4; ++k) s.push_back((char)(100 + k + c)); }
    }
    return s;
}

struct Reader { const char* name; std::string file; int (*load)(const std::string&); };
static int load_scene(const std::string& p) {
    trc_host_scene* hs = nullptr; trc_Camera cam; trc_pbrt_info info; trc_pbrt_shape shapes[8];
    const trc_status st = trc_host_scene_load_pbrt(p.c_str(), &hs, &cam, &info, shapes, 8);
    if (st == TRC_OK) { trc_scene v; trc_host_scene_view(hs, &v); EXPECT(v.n_bvh >= 3); trc_host_scene_destroy(hs); }
    return st;
}
static int load_mesh_pbrt(const std::string& p) { trc_host_mesh* m = nullptr; const trc_status st = trc_host_mesh_load_pbrt(p.c_str(), &m); if (st == TRC_OK) trc_host_mesh_destroy(m); return st; }
static int load_obj(const std::string& p) { trc_host_mesh* m = nullptr; const trc_status st = trc_host_mesh_load_obj(p.c_str(), &m); if (st == TRC_OK) trc_host_mesh_destroy(m); return st; }
static int load_ply(const std::string& p) { trc_host_mesh* m = nullptr; const trc_status st = trc_host_mesh_load_ply(p.c_str(), &m); if (st == TRC_OK) trc_host_mesh_destroy(m); return st; }
static int load_density(const std::string& p) { uint32_t nx, ny, nz; float* g = nullptr; const trc_status st = trc_host_load_density_pbrt(p.c_str(), &nx, &ny, &nz, &g); if (st == TRC_OK) trc_host_free(g); return st; }
static int load_hdr(const std::string& p) { uint32_t w, h; float* g = nullptr; const trc_status st = trc_host_load_hdr(p.c_str(), &w, &h, &g); if (st == TRC_OK) trc_host_free(g); return st; }
static int load_png(const std::string& p) { uint32_t w, h; float* g = nullptr; const trc_status st = trc_host_load_png(p.c_str(), &w, &h, &g); if (st == TRC_OK) trc_host_free(g); return st; }

int main(int argc, char** argv) {
    int n_fuzz = 2000;
    std::string dir = "/tmp/trc_sanitize";
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--fuzz") && i + 1 < argc) n_fuzz = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--dir") && i + 1 < argc) dir = argv[++i];
    }
    (void)!std::system(("mkdir -p " + dir).c_str());

    std::thread other([] { build_and_render(true); });       // two SAH builds at once: the builder's threads + ours
    build_and_render(false);
    other.join();
    sppm_pass();
    pose_tables();
    skin_tables();
    morph_tables();
    normals_ranges();
    primitive_ranges();
    flagged_trees();
    { uint32_t m32[40 * 52]; trc_host_sobol_matrices32(m32); uint64_t a[52], b[52]; EXPECT(trc_host_sobol_interval_tables(11, a, b) == TRC_OK); }

    write_file(dir + "/scene.pbrt", kScene);
    write_file(dir + "/medium.pbrt", std::string("WorldBegin\n") + kMedium + "WorldEnd\n");
    write_file(dir + "/mesh.ply", make_ply(1));
    std::vector<Reader> readers = {
        {"pbrt scene", dir + "/scene.pbrt", load_scene}, {"pbrt meshes", dir + "/scene.pbrt", load_mesh_pbrt}, {"pbrt density", dir + "/medium.pbrt", load_density},
        {"ply ascii", dir + "/a.ply", load_ply}, {"ply little", dir + "/mesh.ply", load_ply}, {"ply big", dir + "/b.ply", load_ply},
        {"obj", dir + "/m.obj", load_obj}, {"hdr", dir + "/sky.hdr", load_hdr}, {"png", dir + "/tex.png", load_png}};
    write_file(dir + "/a.ply", make_ply(0)); write_file(dir + "/b.ply", make_ply(2));
    write_file(dir + "/m.obj", kObj); write_file(dir + "/sky.hdr", make_hdr());
    { std::vector<uint8_t> px(7 * 5 * 4); for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 37); EXPECT(trc_host_write_png((dir + "/tex.png").c_str(), px.data(), 7, 5) == TRC_OK); }
    for (const Reader& r : readers) { const int st = r.load(r.file); if (st != TRC_OK) { std::fprintf(stderr, "%s: well-formed file rejected (%d)\n", r.name, st); ++g_fail; } }

    std::mt19937 gen(12345);
    size_t loaded = 0, rejected = 0;
    for (const Reader& r : readers) {
        const std::string good = read_file(r.file);
        const std::string victim = dir + "/fuzz_input" + r.file.substr(r.file.find_last_of('.'));
        for (int k = 0; k < n_fuzz; ++k) {
            std::string m = good;
            const int edits = 1 + (int)(gen() % 4);
            for (int e = 0; e < edits && !m.empty(); ++e) {
                const size_t at = gen() % m.size();
                switch (gen() % 6) {
                    case 0: m[at] = (char)(gen() & 0xFF); break;                              // flip a byte
                    case 1: m.erase(at, 1 + gen() % 8); break;                                // drop a few
                    case 2: m.insert(at, std::string(1 + gen() % 6, (char)('0' + gen() % 10))); break;   // digits
                    case 3: m.resize(at); break;                                              // truncate
                    case 4: m.insert(at, m.substr(gen() % m.size(), gen() % 16)); break;      // duplicate a piece
                    default: m[at] = "[]\"-.e \n"[gen() % 8]; break;                          // a syntax character
                }
            }
            write_file(victim, m);
            if (r.load(victim) == TRC_OK) ++loaded; else ++rejected;
        }
    }
    std::printf("sanitize driver: %d expectation failures; fuzz: %zu mutated files loaded, %zu rejected with a status\n", g_fail, loaded, rejected);
    return g_fail ? 1 : 0;
}
