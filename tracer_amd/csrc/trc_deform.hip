// trc_deform.hip -- vertices computed on the device from the rest copy (RefitState::d_rest), in front of the refit's tail (trc_refit.hpp).
// trc_pose_vertices puts ranges of vertices under a matrix each:
//   k_pose_vertices     ONE launch for all ranges of a call: thread g of the concatenated ranges finds its range in the sorted pose
//                       table by bisection (the table's _pad[0] is the range's first g), reads the vertex from the rest copy
//                       and writes it, posed, to d_verts; two 16 B accesses per vertex each way
// trc_skin_vertices does the same for vertices that bend: trc_skin_bind has left four (bone, weight) influences per bound vertex on
// the device, the call brings the frame's bone palette and runs one of
//   k_skin_vertices_lds the palette's read columns staged in LDS once per workgroup, which then takes 256 bound vertices at a time
//   k_skin_vertices     the columns gathered from memory: palettes beyond kSkinLdsBones (skin_check.hpp), and knob skin_no_lds
// Both blend the four bones' matrices entry by entry and put the REST vertex under the blend as a pose does (pose_store).
// trc_morph_vertices adds weighted deltas to the rest vertex: trc_morph_bind has left n_targets deltas per bound vertex on the device,
// target-major, the call brings the frame's weights, compacted by the host into the active list (morph_check.hpp), and runs one of
//   k_morph_vertices       one thread per bound vertex: rest + the active targets' weighted deltas, in the list's order
//   k_morph_skin_vertices  with a palette: one thread per vertex of the hull of the morph and the skin binding; the morph where the
//                          vertex is morph-bound, then the skin's arithmetic on those values where it is skin-bound (columns gathered)
// Every kernel counts the positions it leaves non-finite or beyond 1e37 (count_overflow)
#include <hip/hip_runtime.h>

#include "morph_check.hpp"
#include "pose_ranges.hpp"
#include "skin_check.hpp"
#include "trc_refit.hpp"

namespace {

// the caller's contract, broken: counted, never an index.  (By reference: passed by value, the compiler orders the three tests' OR otherwise)
__device__ __forceinline__ void count_overflow(const float& x, const float& y, const float& z, uint32_t* __restrict__ overflows) {
    if (!(fabsf(x) <= 1e37f) || !(fabsf(y) <= 1e37f) || !(fabsf(z) <= 1e37f))
        __hip_atomic_fetch_add(overflows, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// verts[v] = the vertex (a, b: x y z nx | ny nz u v) under m: 4 columns of a model matrix, then the 3 of its normal matrix, in the
// operation order of include/tracer_abi.h
__device__ __forceinline__ void pose_store(const float4& a, const float4& b, const float4 (&m)[7], float4* __restrict__ verts, uint32_t v, uint32_t* __restrict__ overflows) {
    const float4 c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3], n0 = m[4], n1 = m[5], n2 = m[6];
    const float x = ((c0.x * a.x + c1.x * a.y) + c2.x * a.z) + c3.x;
    const float y = ((c0.y * a.x + c1.y * a.y) + c2.y * a.z) + c3.y;
    const float z = ((c0.z * a.x + c1.z * a.y) + c2.z * a.z) + c3.z;
    const float nx = (n0.x * a.w + n1.x * b.x) + n2.x * b.y;
    const float ny = (n0.y * a.w + n1.y * b.x) + n2.y * b.y;
    const float nz = (n0.z * a.w + n1.z * b.x) + n2.z * b.y;
    verts[2 * (size_t)v] = make_float4(x, y, z, nx);
    verts[2 * (size_t)v + 1] = make_float4(ny, nz, b.z, b.w);
    count_overflow(x, y, z, overflows);
}

// ---- the pose: verts[v] = M * rest[v] for every vertex of every range.
// table: the call's poses sorted by first, _pad[0] = the number of vertices in the ranges before (host, trc_pose_vertices); total: in all
__global__ void __launch_bounds__(256) k_pose_vertices(const float4* __restrict__ rest, float4* __restrict__ verts, uint32_t n_vertex,
                                                       const trc_pose* __restrict__ table, uint32_t n_poses, uint32_t total, uint32_t* __restrict__ overflows) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    uint32_t lo = 0, hi = n_poses;                                  // the last range that starts at or before g
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (table[mid]._pad[0] <= g) lo = mid; else hi = mid;
    }
    const uint32_t v = table[lo].first + (g - table[lo]._pad[0]);
    if (v >= n_vertex) return;                                      // (the host refused such a table)
    const float4* t = reinterpret_cast<const float4*>(&table[lo].model_matrix);      // 4 columns, then the normal matrix's
    const float4 m[7] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
    const float4 a = rest[2 * (size_t)v], b = rest[2 * (size_t)v + 1];
    pose_store(a, b, m, verts, v, overflows);
}

// ---- the skin: verts[first + i] = blend(influences[i], palette) * rest[first + i] for every bound vertex, in the operation order of
// include/tracer_abi.h: the four bones' columns blended entry by entry, then k_pose_vertices' expressions with the blend.  Every
// statement is one operation (the exact build compiles without contraction).  col(b, c): column c of bone b, 0..3 of its model matrix
// and 4..6 of its normal matrix.  The two kernels differ in where col reads from and in nothing else
__device__ __forceinline__ float skin_blend(const float4& w, float a0, float a1, float a2, float a3) {
    const float p0 = w.x * a0;
    const float p1 = w.y * a1;
    const float p2 = w.z * a2;
    const float p3 = w.w * a3;
    const float s01 = p0 + p1;
    const float s012 = s01 + p2;
    return s012 + p3;
}
template <class Col>
__device__ __forceinline__ void skin_vertex(const float4& __restrict__ a, const float4& __restrict__ b, float4* __restrict__ verts, uint32_t v, const uint4& bone, const float4& w,
                                            const Col& col, uint32_t* __restrict__ overflows) {      // a, b: x y z nx | ny nz u v, the values to skin
    float4 m[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const float4 m0 = col(bone.x, c), m1 = col(bone.y, c), m2 = col(bone.z, c), m3 = col(bone.w, c);
        m[c].x = skin_blend(w, m0.x, m1.x, m2.x, m3.x);
        m[c].y = skin_blend(w, m0.y, m1.y, m2.y, m3.y);
        m[c].z = skin_blend(w, m0.z, m1.z, m2.z, m3.z);
        m[c].w = 0.0f;
    }
    pose_store(a, b, m, verts, v, overflows);
}
struct KSkin {
    const float4* rest; float4* verts; uint32_t n_vertex;
    const uint4* influences; uint32_t first, count;     // influences: 2 x 16 B per bound vertex, the bones and then the weights
    const float4* palette; uint32_t n_bones;            // 8 columns per bone (trc_skin_bone)
    uint32_t* overflows;
};
// the bones and weights of bound vertex i; false: it names a bone beyond n_bones (the host refused such a table or palette: never)
__device__ __forceinline__ bool skin_influence(const uint4* influences, uint32_t i, uint32_t n_bones, uint4& bone, float4& w) {
    bone = influences[2 * (size_t)i];
    const uint4 wb = influences[2 * (size_t)i + 1];
    if (bone.x >= n_bones || bone.y >= n_bones || bone.z >= n_bones || bone.w >= n_bones) return false;
    w = make_float4(__uint_as_float(wb.x), __uint_as_float(wb.y), __uint_as_float(wb.z), __uint_as_float(wb.w));
    return true;
}
// bound vertex i of the binding
template <class Col>
__device__ __forceinline__ void skin_bound_vertex(const KSkin& p, uint32_t i, uint32_t n_bones, const Col& col) {
    const uint32_t v = p.first + i;
    if (v >= p.n_vertex) return;
    uint4 bone; float4 w;
    if (!skin_influence(p.influences, i, n_bones, bone, w)) return;
    skin_vertex(p.rest[2 * (size_t)v], p.rest[2 * (size_t)v + 1], p.verts, v, bone, w, col, p.overflows);
}
// gathered: one thread per bound vertex, the columns straight from the palette in memory (a palette is small: L2-resident)
__global__ void __launch_bounds__(256) k_skin_vertices(KSkin p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.count) return;
    const float4* palette = p.palette;
    skin_bound_vertex(p, i, p.n_bones, [palette](uint32_t b, int c) { return palette[8 * (size_t)b + c]; });
}
// staged: the read columns of every bone (112 of its 128 bytes) once per WORKGROUP into LDS, then the workgroup's threads take batches
// of 256 bound vertices until none is left, so a palette is loaded gridDim.x times and not count / 256 times.  n_bones <= kSkinLdsBones
__global__ void __launch_bounds__(256) k_skin_vertices_lds(KSkin p) {
    __shared__ float4 cols[7 * kSkinLdsBones];
    const uint32_t n_bones = p.n_bones < kSkinLdsBones ? p.n_bones : kSkinLdsBones;
    for (uint32_t k = threadIdx.x; k < 7u * n_bones; k += 256u) {
        const uint32_t b = k / 7u;
        cols[k] = p.palette[8 * (size_t)b + (k - 7u * b)];
    }
    __syncthreads();
    const float4* staged = cols;
    for (size_t base = (size_t)blockIdx.x * 256u; base < p.count; base += (size_t)gridDim.x * 256u) {      // (64 bits: base + the stride may pass 2^32)
        const size_t i = base + threadIdx.x;
        if (i < p.count) skin_bound_vertex(p, (uint32_t)i, n_bones, [staged](uint32_t b, int c) { return staged[7u * b + c]; });
    }
}
constexpr uint32_t kSkinWorkgroupsPerCu = 2;     // of the staged kernel: 512 threads of a CU's 2048, each workgroup ~4 batches on 0.5 M vertices

// ---- the morph: verts[first + i] = rest[first + i] + the weighted deltas of the active targets, in the operation order of
// include/tracer_abi.h: for every entry (k, w) of the active list in order and every component c, p = w * d[k][i].c; acc.c = acc.c + p.
// Every statement is one operation (the exact build compiles without contraction).  The list index is the same in every lane, so an
// entry is one scalar 8-byte load; a delta is three 8-byte loads (a record is 24 bytes from a hipMalloc base: 8-byte aligned)
struct KMorph {
    const float4* rest; float4* verts; uint32_t n_vertex;
    const float2* deltas; uint32_t n_targets, first, count;      // deltas: 3 x 8 B per bound vertex and target, target-major
    const uint2* active; uint32_t n_active;                      // trc_morph_active: the target, the weight's bits
    uint32_t* overflows;
};
__device__ __forceinline__ void morph_add(float (&acc)[6], float w, const float2& d0, const float2& d1, const float2& d2) {
    const float p0 = w * d0.x;
    const float p1 = w * d0.y;
    const float p2 = w * d1.x;
    const float p3 = w * d1.y;
    const float p4 = w * d2.x;
    const float p5 = w * d2.y;
    acc[0] = acc[0] + p0;
    acc[1] = acc[1] + p1;
    acc[2] = acc[2] + p2;
    acc[3] = acc[3] + p3;
    acc[4] = acc[4] + p4;
    acc[5] = acc[5] + p5;
}
// a, b: bound vertex i's rest values in, its morphed values out.  The six sums are serial chains by definition; the loop takes four
// entries at a time and loads their twelve 8-byte words before the first add, so that the memory latency of four targets overlaps --
// the order of the operations is the list's all the same.  false: an entry names a target the table does not hold (the host made
// the list from the binding's own n_targets: never)
__device__ __forceinline__ bool morph_bound_vertex(const KMorph& p, uint32_t i, float4& a, float4& b) {
    float acc[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
    const float2* __restrict__ deltas = p.deltas;
    const uint2* __restrict__ active = p.active;
    uint32_t j = 0;
    for (; j + 4u <= p.n_active; j += 4u) {
        const uint2 e0 = active[j], e1 = active[j + 1], e2 = active[j + 2], e3 = active[j + 3];
        if (e0.x >= p.n_targets || e1.x >= p.n_targets || e2.x >= p.n_targets || e3.x >= p.n_targets) return false;
        const float2* q0 = deltas + 3 * ((size_t)e0.x * p.count + i);      // (64 bits: n_targets * count passes 2^32)
        const float2* q1 = deltas + 3 * ((size_t)e1.x * p.count + i);
        const float2* q2 = deltas + 3 * ((size_t)e2.x * p.count + i);
        const float2* q3 = deltas + 3 * ((size_t)e3.x * p.count + i);
        const float2 d00 = q0[0], d01 = q0[1], d02 = q0[2];
        const float2 d10 = q1[0], d11 = q1[1], d12 = q1[2];
        const float2 d20 = q2[0], d21 = q2[1], d22 = q2[2];
        const float2 d30 = q3[0], d31 = q3[1], d32 = q3[2];
        morph_add(acc, __uint_as_float(e0.y), d00, d01, d02);
        morph_add(acc, __uint_as_float(e1.y), d10, d11, d12);
        morph_add(acc, __uint_as_float(e2.y), d20, d21, d22);
        morph_add(acc, __uint_as_float(e3.y), d30, d31, d32);
    }
    for (; j < p.n_active; ++j) {
        const uint2 e = active[j];
        if (e.x >= p.n_targets) return false;
        const float2* q = deltas + 3 * ((size_t)e.x * p.count + i);
        const float2 d0 = q[0], d1 = q[1], d2 = q[2];
        morph_add(acc, __uint_as_float(e.y), d0, d1, d2);
    }
    a = make_float4(acc[0], acc[1], acc[2], acc[3]);
    b = make_float4(acc[4], acc[5], b.z, b.w);
    return true;
}
__device__ __forceinline__ void morph_store(float4* __restrict__ verts, uint32_t v, const float4& a, const float4& b, uint32_t* __restrict__ overflows) {
    verts[2 * (size_t)v] = a;
    verts[2 * (size_t)v + 1] = b;
    count_overflow(a.x, a.y, a.z, overflows);
}
// morph only: one thread per bound vertex
__global__ void __launch_bounds__(256) k_morph_vertices(KMorph p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.count) return;
    const uint32_t v = p.first + i;
    if (v >= p.n_vertex) return;                                    // (the host refused such a table)
    float4 a = p.rest[2 * (size_t)v], b = p.rest[2 * (size_t)v + 1];              // x y z nx | ny nz u v
    if (!morph_bound_vertex(p, i, a, b)) return;
    morph_store(p.verts, v, a, b, p.overflows);
}
// the morph and the skin on top: one thread per vertex of [hull_first, hull_first + hull_count), the hull of the two bindings' ranges.
// A vertex of the morph binding is morphed, a vertex of the skin binding then skinned from what it has by then -- the morphed values
// or the rest values; a vertex in neither is not written.  s.first / s.count: the skin binding's own range
__global__ void __launch_bounds__(256) k_morph_skin_vertices(KMorph p, KSkin s, uint32_t hull_first, uint32_t hull_count) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= hull_count) return;
    const uint32_t v = hull_first + h;
    if (v >= p.n_vertex) return;
    const uint32_t im = v - p.first, is = v - s.first;             // (below `first`: wraps to a value >= count)
    const bool morphed = im < p.count, skinned = is < s.count;
    if (!morphed && !skinned) return;
    float4 a = p.rest[2 * (size_t)v], b = p.rest[2 * (size_t)v + 1];
    if (morphed && !morph_bound_vertex(p, im, a, b)) return;
    if (!skinned) { morph_store(p.verts, v, a, b, p.overflows); return; }
    uint4 bone; float4 w;
    if (!skin_influence(s.influences, is, s.n_bones, bone, w)) return;
    const float4* palette = s.palette;
    skin_vertex(a, b, s.verts, v, bone, w, [palette](uint32_t bn, int c) { return palette[8 * (size_t)bn + c]; }, s.overflows);
}

// the skin binding and the palette of n_bones bones in d_palette, as the kernels take them
KSkin skin_params(trc_ctx* ctx, uint32_t n_bones) {
    const RefitState& r = ctx->refit;
    KSkin k{};
    k.rest = reinterpret_cast<const float4*>(r.d_rest); k.verts = reinterpret_cast<float4*>(ctx->d_verts); k.n_vertex = ctx->n_vertex;
    k.influences = reinterpret_cast<const uint4*>(r.skin.d_influences); k.first = r.skin.first; k.count = r.skin.count;
    k.palette = reinterpret_cast<const float4*>(r.d_palette); k.n_bones = n_bones; k.overflows = trc_overflow_counter(ctx);
    return k;
}
// ... and the morph binding and the active list of n_active entries in d_morph_active
KMorph morph_params(trc_ctx* ctx, uint32_t n_active) {
    const RefitState& r = ctx->refit;
    KMorph m{};
    m.rest = reinterpret_cast<const float4*>(r.d_rest); m.verts = reinterpret_cast<float4*>(ctx->d_verts); m.n_vertex = ctx->n_vertex;
    m.deltas = reinterpret_cast<const float2*>(r.morph.d_deltas); m.n_targets = r.morph.n_targets; m.first = r.morph.first; m.count = r.morph.count;
    m.active = static_cast<const uint2*>(r.d_morph_active); m.n_active = n_active; m.overflows = trc_overflow_counter(ctx);
    return m;
}
inline uint32_t batches_of(uint32_t count) { return (uint32_t)(((size_t)count + 255) / 256); }
// A binding's table of `bytes` bytes (0: none) in `slot`: the old one goes only when the new one is on the device
template <class T> trc_status bind_table(trc_ctx* ctx, T*& slot, const T* host, size_t bytes, const char* what) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf table;
    if (bytes != 0) {
        TRC_TRY(table.alloc(ctx, bytes, what));
        TRC_TRY(trc_copy_to_device(ctx, table.p, host, bytes, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // a skin or a morph still in flight reads the table that goes
    (void)hipFree(slot);
    slot = static_cast<T*>(table.release());
    return TRC_OK;
}

}  // namespace

extern "C" {

// [first, first + count) of the tail: the hull of the call's ranges
trc_status trc_pose_vertices(trc_ctx* ctx, const trc_pose* poses, uint32_t n_poses) {
    TRC_TRY(trc_enter_scene(ctx, "trc_pose_vertices"));
    if (n_poses == 0) return TRC_OK;
    if (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_pose_vertices: the scene has no triangles");
    std::vector<uint32_t> order;
    if (const char* why = trc_pose_table_check(poses, n_poses, ctx->n_vertex, order)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_pose_vertices: ") + why);
    // the kernel's table: sorted by first, every range with the number of vertices before it (no two overlap: the sum is <= n_vertex)
    std::vector<trc_pose> table(n_poses);
    uint32_t total = 0;
    for (uint32_t i = 0; i < n_poses; ++i) {
        table[i] = poses[order[i]];
        table[i]._pad[0] = total; table[i]._pad[1] = 0;
        total += table[i].count;
    }
    const uint32_t hull_first = table.front().first, hull_count = table.back().first - hull_first + table.back().count;
    RefitState& r = ctx->refit;
    TRC_TRY(trc_refit_begin(ctx, "trc_pose_vertices"));
    TRC_TRY(trc_grow_buffer(ctx, r.d_pose_table, r.pose_table_bytes, table.size() * sizeof(trc_pose), "trc_pose_vertices: hipMalloc pose table"));
    TRC_TRY(trc_rest_ensure(ctx, "rest vertices (trc_pose_vertices)"));
    TRC_TRY(trc_copy_to_device(ctx, r.d_pose_table, table.data(), table.size() * sizeof(trc_pose), ctx->stream));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    TRC_TRY(trc_refit_open(ctx));
    hipLaunchKernelGGL(k_pose_vertices, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(r.d_rest),
                       reinterpret_cast<float4*>(ctx->d_verts), ctx->n_vertex, r.d_pose_table, n_poses, total, trc_overflow_counter(ctx));
    return trc_refit_tail(ctx, hull_first, hull_count, true);
}

trc_status trc_skin_bind(trc_ctx* ctx, const trc_skin_influence* influences, uint32_t first, uint32_t count) {
    TRC_TRY(trc_enter_scene(ctx, "trc_skin_bind"));
    if (count != 0 && (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_skin_bind: the scene has no triangles");
    uint32_t max_bone = 0;
    if (const char* why = trc_skin_influence_check(influences, first, count, ctx->n_vertex, &max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_skin_bind: ") + why);
    RefitState::Skin& s = ctx->refit.skin;
    TRC_TRY(bind_table(ctx, s.d_influences, influences, (size_t)count * sizeof(trc_skin_influence), "influence table (trc_skin_bind)"));
    s.first = count ? first : 0u; s.count = count; s.max_bone = max_bone;
    return TRC_OK;
}

// [first, first + count) of the tail: the binding's range
trc_status trc_skin_vertices(trc_ctx* ctx, const trc_skin_bone* bones, uint32_t n_bones) {
    TRC_TRY(trc_enter_scene(ctx, "trc_skin_vertices"));
    if (n_bones == 0) return TRC_OK;
    RefitState& r = ctx->refit;
    if (!r.skin.d_influences || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_skin_vertices: no binding (trc_skin_bind)");
    if (const char* why = trc_skin_palette_check(bones, n_bones, r.skin.max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_skin_vertices: ") + why);
    TRC_TRY(trc_refit_begin(ctx, "trc_skin_vertices"));
    const size_t bytes = (size_t)n_bones * sizeof(trc_skin_bone);
    TRC_TRY(trc_grow_buffer(ctx, r.d_palette, r.palette_bytes, bytes, "trc_skin_vertices: hipMalloc bone palette"));
    TRC_TRY(trc_rest_ensure(ctx, "rest vertices (trc_skin_vertices)"));
    TRC_TRY(trc_copy_to_device(ctx, r.d_palette, bones, bytes, ctx->stream));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    TRC_TRY(trc_refit_open(ctx));
    const uint32_t batches = batches_of(r.skin.count);
    if (n_bones <= kSkinLdsBones && !ctx->knobs.skin_no_lds)
        hipLaunchKernelGGL(k_skin_vertices_lds, dim3(std::min(batches, kSkinWorkgroupsPerCu * (uint32_t)ctx->cu_count)), dim3(256), 0, ctx->stream, skin_params(ctx, n_bones));
    else
        hipLaunchKernelGGL(k_skin_vertices, dim3(batches), dim3(256), 0, ctx->stream, skin_params(ctx, n_bones));
    return trc_refit_tail(ctx, r.skin.first, r.skin.count, true);
}

trc_status trc_morph_bind(trc_ctx* ctx, const trc_morph_delta* deltas, uint32_t n_targets, uint32_t first, uint32_t count) {
    TRC_TRY(trc_enter_scene(ctx, "trc_morph_bind"));
    const bool empty = trc_morph_table_empty(n_targets, count);
    if (!empty && (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_bind: the scene has no triangles");
    if (const char* why = trc_morph_table_check(deltas, n_targets, first, count, ctx->n_vertex)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_bind: ") + why);
    RefitState::Morph& m = ctx->refit.morph;
    const size_t bytes = empty ? 0 : (size_t)n_targets * count * sizeof(trc_morph_delta);      // (size_t: the product passes 2^32)
    TRC_TRY(bind_table(ctx, m.d_deltas, deltas, bytes, "delta table (trc_morph_bind)"));
    m.first = empty ? 0u : first; m.count = empty ? 0u : count; m.n_targets = empty ? 0u : n_targets;
    return TRC_OK;
}

// [first, first + count) of the tail: the morph binding's range, or with a palette the hull of the morph and the skin binding
trc_status trc_morph_vertices(trc_ctx* ctx, const float* weights, uint32_t n_weights, const trc_skin_bone* bones, uint32_t n_bones) {
    TRC_TRY(trc_enter_scene(ctx, "trc_morph_vertices"));
    RefitState& r = ctx->refit;
    if (!r.morph.d_deltas || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_vertices: no binding (trc_morph_bind)");
    std::vector<trc_morph_active> active;
    if (const char* why = trc_morph_weights_check(weights, n_weights, r.morph.n_targets, active)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_vertices: ") + why);
    uint32_t first = r.morph.first, count = r.morph.count;
    if (n_bones != 0) {
        if (!r.skin.d_influences) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_vertices: n_bones > 0 without a skin binding (trc_skin_bind)");
        if (const char* why = trc_skin_palette_check(bones, n_bones, r.skin.max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_vertices: ") + why);
        // the hull of the two ranges; both end within n_vertex, so neither sum wraps
        const uint32_t end = std::max(first + count, r.skin.first + r.skin.count);
        first = std::min(first, r.skin.first);
        count = end - first;
    }
    TRC_TRY(trc_refit_begin(ctx, "trc_morph_vertices"));
    const size_t list_bytes = active.size() * sizeof(trc_morph_active), palette_bytes = (size_t)n_bones * sizeof(trc_skin_bone);
    TRC_TRY(trc_grow_buffer(ctx, r.d_morph_active, r.morph_active_bytes, list_bytes, "trc_morph_vertices: hipMalloc active list"));
    if (n_bones != 0) TRC_TRY(trc_grow_buffer(ctx, r.d_palette, r.palette_bytes, palette_bytes, "trc_morph_vertices: hipMalloc bone palette"));
    TRC_TRY(trc_rest_ensure(ctx, "rest vertices (trc_morph_vertices)"));
    if (list_bytes != 0) TRC_TRY(trc_copy_to_device(ctx, r.d_morph_active, active.data(), list_bytes, ctx->stream));
    if (n_bones != 0) TRC_TRY(trc_copy_to_device(ctx, r.d_palette, bones, palette_bytes, ctx->stream));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    TRC_TRY(trc_refit_open(ctx));
    const KMorph m = morph_params(ctx, (uint32_t)active.size());
    if (n_bones != 0)
        hipLaunchKernelGGL(k_morph_skin_vertices, dim3(batches_of(count)), dim3(256), 0, ctx->stream, m, skin_params(ctx, n_bones), first, count);
    else
        hipLaunchKernelGGL(k_morph_vertices, dim3(batches_of(count)), dim3(256), 0, ctx->stream, m);
    return trc_refit_tail(ctx, first, count, true);
}

}  // extern "C"
