// trc_primitives.hip -- trc_update_primitives: spheres, squares and cubes of the uploaded scene replaced in place, on the interface of
// the moving-geometry family (trc_refit.hpp).  The caller's records travel once through the pinned staging path into a buffer the
// context keeps (RefitState::d_prim_stage); one kernel, a thread per primitive, then
//   - repacks the record into the blob's record with the bits fill_primitives (trc_scene_prep.hpp) gives for it, and
//   - writes the primitive's leaf box (dev_trileaf.hpp: primitive_leaf_box, BVH::buildNode) into its parent's slot of the fat node
//     that RefitState::Maps::d_primslot names; a primitive that no leaf names has no slot.
// The family's refit runs behind it (trc_refit_tail with an empty vertex range: no triangle record is rewritten): it recomputes every
// interior box, carries the leaf boxes into the records of a device-built tree, and sends the root box back.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "dev_trileaf.hpp"
#include "primitives_check.hpp"
#include "trc_refit.hpp"

namespace {

struct KPrimitives {
    uint32_t* blob; uint32_t off_spheres, off_squares, off_cubes, off_nodes, n_nodes;
    const trc_Sphere* spheres; uint32_t first_sphere, n_sphere;
    const trc_Square* squares; uint32_t first_square, n_square;
    const trc_Cube* cubes; uint32_t first_cube, n_cube;
    const uint32_t* primslot; uint32_t slot_squares, slot_cubes;      // the map's sections begin at 0 (spheres), slot_squares, slot_cubes
};

// 24 bytes of the parent's slot; two primitives may share a fat node, and a slot straddles its 16-byte quads: dword stores
__device__ __forceinline__ void store_leaf_box(const KPrimitives& p, uint32_t entry, const float mn[3], const float mx[3]) {
    const uint32_t at = p.primslot[entry];
    if (at == kTagNone || (at >> 1) >= p.n_nodes) return;
    float* q = reinterpret_cast<float*>(p.blob + p.off_nodes) + (size_t)kNodeDwords * (at >> 1) + 6u * (at & 1u);
    q[0] = mn[0]; q[1] = mn[1]; q[2] = mn[2]; q[3] = mx[0]; q[4] = mx[1]; q[5] = mx[2];
}

__global__ void __launch_bounds__(256) k_update_primitives(KPrimitives p) {
    uint32_t t = blockIdx.x * 256u + threadIdx.x;
    float mn[3], mx[3];
    if (t < p.n_sphere) {
        const trc_Sphere& sp = p.spheres[t];
        const uint32_t index = p.first_sphere + t;
        uint32_t* q = p.blob + p.off_spheres + (size_t)index * kSphereDwords;
        q[0] = __float_as_uint(sp.center.x); q[1] = __float_as_uint(sp.center.y); q[2] = __float_as_uint(sp.center.z); q[3] = __float_as_uint(sp.radius);
        q[4] = sp.material;
        primitive_leaf_box(sp.boundingBOX, sp.model_matrix, mn, mx);
        store_leaf_box(p, index, mn, mx);
        return;
    }
    t -= p.n_sphere;
    if (t < p.n_square) {
        const trc_Square& sq = p.squares[t];
        const uint32_t index = p.first_square + t;
        uint32_t* q = p.blob + p.off_squares + (size_t)index * kSquareDwords;
        // Square::area() = 2*i*j and aeraPDF() = 1/area (Square.hh:31-38) in binary32, as fill_primitives evaluates them
        const float di = sq.range_i.y - sq.range_i.x, dj = sq.range_j.y - sq.range_j.x;
        const float area = 2 * di * dj;
        const float pdf = 1 / area;
        q[0] = __float_as_uint(sq.range_i.x); q[1] = __float_as_uint(sq.range_i.y); q[2] = __float_as_uint(sq.range_j.x); q[3] = __float_as_uint(sq.range_j.y);
        q[4] = __float_as_uint(sq.value_k); q[5] = __float_as_uint(pdf);
        q[6] = (uint32_t)sq.axis_i | ((uint32_t)sq.axis_j << 2) | ((uint32_t)sq.axis_k << 4);
        q[7] = sq.material;
        primitive_leaf_box(sq.boundingBOX, sq.model_matrix, mn, mx);
        store_leaf_box(p, p.slot_squares + index, mn, mx);
        return;
    }
    t -= p.n_square;
    if (t >= p.n_cube) return;
    const trc_Cube& cb = p.cubes[t];
    const uint32_t index = p.first_cube + t;
    uint32_t* q = p.blob + p.off_cubes + (size_t)index * kCubeDwords;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        q[3 * c] = __float_as_uint(cb.inverse_matrix.columns[c].x); q[3 * c + 1] = __float_as_uint(cb.inverse_matrix.columns[c].y); q[3 * c + 2] = __float_as_uint(cb.inverse_matrix.columns[c].z);
        q[12 + 3 * c] = __float_as_uint(cb.model_matrix.columns[c].x); q[13 + 3 * c] = __float_as_uint(cb.model_matrix.columns[c].y); q[14 + 3 * c] = __float_as_uint(cb.model_matrix.columns[c].z);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[24 + 3 * c] = __float_as_uint(cb.normal_matrix.columns[c].x); q[25 + 3 * c] = __float_as_uint(cb.normal_matrix.columns[c].y); q[26 + 3 * c] = __float_as_uint(cb.normal_matrix.columns[c].z);
    }
    q[33] = __float_as_uint(cb.box.mini.x); q[34] = __float_as_uint(cb.box.mini.y); q[35] = __float_as_uint(cb.box.mini.z);
    q[36] = __float_as_uint(cb.box.maxi.x); q[37] = __float_as_uint(cb.box.maxi.y); q[38] = __float_as_uint(cb.box.maxi.z);
    q[39] = cb.material;
    primitive_leaf_box(cb.box, cb.model_matrix, mn, mx);
    store_leaf_box(p, p.slot_cubes + index, mn, mx);
}

}  // namespace

extern "C" trc_status trc_update_primitives(trc_ctx* ctx, const trc_primitive_ranges* r) {
    TRC_TRY(trc_enter_scene(ctx, "trc_update_primitives"));
    const DScene& sc = ctx->ks.sc;
    if (const char* why = trc_primitive_ranges_check(r, sc.n_spheres, sc.n_squares, sc.n_cubes, sc.n_materials)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_update_primitives: ") + why);
    const uint32_t total = r->n_sphere + r->n_square + r->n_cube;      // (each within the scene's count, all of them within 40 KB of records)
    if (total == 0) return TRC_OK;
    // one transfer: spheres, squares, cubes behind one another (272, 272 and 240 bytes apiece: every section begins 16-byte aligned)
    const size_t sphere_bytes = (size_t)r->n_sphere * sizeof(trc_Sphere), square_bytes = (size_t)r->n_square * sizeof(trc_Square), cube_bytes = (size_t)r->n_cube * sizeof(trc_Cube);
    std::vector<char> stage(sphere_bytes + square_bytes + cube_bytes);
    if (sphere_bytes) std::memcpy(stage.data(), r->spheres, sphere_bytes);
    if (square_bytes) std::memcpy(stage.data() + sphere_bytes, r->squares, square_bytes);
    if (cube_bytes) std::memcpy(stage.data() + sphere_bytes + square_bytes, r->cubes, cube_bytes);
    RefitState& rs = ctx->refit;
    TRC_TRY(trc_refit_begin(ctx, "trc_update_primitives"));
    TRC_TRY(trc_grow_buffer(ctx, rs.d_prim_stage, rs.prim_stage_bytes, stage.size(), "trc_update_primitives: hipMalloc record staging"));
    TRC_TRY(trc_copy_to_device(ctx, rs.d_prim_stage, stage.data(), stage.size(), ctx->stream));
    // from here on the scene changed
    trc_scene_changed(ctx, kScenePrimitivesMoved);
    KPrimitives p{};
    p.blob = ctx->d_blob; p.off_spheres = sc.off_spheres; p.off_squares = sc.off_squares; p.off_cubes = sc.off_cubes; p.off_nodes = sc.off_nodes; p.n_nodes = sc.n_nodes;
    char* const base = static_cast<char*>(rs.d_prim_stage);
    p.spheres = reinterpret_cast<const trc_Sphere*>(base); p.first_sphere = r->first_sphere; p.n_sphere = r->n_sphere;
    p.squares = reinterpret_cast<const trc_Square*>(base + sphere_bytes); p.first_square = r->first_square; p.n_square = r->n_square;
    p.cubes = reinterpret_cast<const trc_Cube*>(base + sphere_bytes + square_bytes); p.first_cube = r->first_cube; p.n_cube = r->n_cube;
    p.primslot = rs.maps.d_primslot; p.slot_squares = sc.n_spheres; p.slot_cubes = sc.n_spheres + sc.n_squares;
    TRC_TRY(trc_refit_open(ctx));
    hipLaunchKernelGGL(k_update_primitives, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, p);
    return trc_refit_tail(ctx, 0, 0, false);
}
