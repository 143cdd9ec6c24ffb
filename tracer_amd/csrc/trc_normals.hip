// trc_normals.hip -- trc_recompute_normals: the normals of a vertex range replaced by area-weighted smooth normals of the mesh as it
// stands.  Nothing moves.  The first call of a scene sorts the corners of the index list by their vertex (k_adj_keys, trc_lbvh.hip's
// radix sort, k_adj_offsets: the adjacency, kept with the scene); every call then runs
//   k_vertex_normals       one thread per vertex of the range: the cross products of its corners' triangles, read from the 48 B position
//                          records, summed in corner order, put on the side of the normal it holds, normalised
// and the refit's record rewrite behind it (trc_refit.hpp: trc_refit_launch_triangles).  No box changes, so nothing else of the refit runs
#include <hip/hip_runtime.h>

#include <cmath>

#include "normals_check.hpp"
#include "trc_refit.hpp"

namespace {

// ---- the vertex -> corner adjacency of the index list, once per scene, and the gather behind it, in the operation order of
// include/tracer_abi.h.  Corner k of the index list belongs to triangle k / 3 and names vertex idx[k]
__global__ void __launch_bounds__(256) k_adj_keys(const uint32_t* __restrict__ idx, uint32_t n_index, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_index) return;
    keys[k] = idx[k];
    vals[k] = k;
}
// offsets[v] = the first position of the sorted keys that holds a vertex >= v: position k writes it for every v in (keys[k - 1], keys[k]]
// (from 0 at k == 0), the last position also for (keys[n_index - 1], n_vertex].  n_vertex + 1 stores in all, each by one thread; a
// key is clamped to n_vertex (the upload refused an index >= n_vertex: never), so that no store leaves offsets[0 .. n_vertex].  A run of
// vertices that no triangle names is written by the one thread behind it: once per scene, whatever its length
__global__ void __launch_bounds__(256) k_adj_offsets(const uint32_t* __restrict__ keys, uint32_t n_index, uint32_t n_vertex, uint32_t* __restrict__ offsets) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_index) return;
    const uint32_t key = keys[k] < n_vertex ? keys[k] : n_vertex;
    const uint32_t prev = k == 0 ? 0u : (keys[k - 1] < n_vertex ? keys[k - 1] : n_vertex);
    for (uint32_t v = k == 0 ? 0u : prev + 1u; v <= key; ++v) offsets[v] = k;
    if (k == n_index - 1)
        for (uint32_t v = key + 1u; v <= n_vertex; ++v) offsets[v] = n_index;
}

struct KNormals {
    float4* verts; uint32_t n_vertex;                                        // x y z nx | ny nz u v
    const uint32_t* offsets; const uint32_t* corners; uint32_t n_index;      // the adjacency
    const uint32_t* tripos; uint32_t n_tri;                                  // the 48 B position records (blob + off_tripos)
    uint32_t first, count;
};
// s = s + cross(p1 - p0, p2 - p0) for the three float4 of a triangle's position record (as dev_meshlight.hpp's mesh_tri_load reads them):
// dev_vec.hpp's cross on the e1, e2 of mesh_tri_area.  Every statement is one operation (the exact build compiles without contraction)
__device__ __forceinline__ void normals_add(F3& s, const float4& a, const float4& b, const float4& c) {
    const F3 n = cross(f3(b.x, b.y, b.z) - f3(a.x, a.y, a.z), f3(c.x, c.y, c.z) - f3(a.x, a.y, a.z));
    s.x = s.x + n.x;
    s.y = s.y + n.y;
    s.z = s.z + n.z;
}
// one thread per vertex of the range.  The sum is a serial chain by definition; the loop takes four corners at a time and loads their
// twelve 16-byte words before the first add, so that the latency of four records overlaps -- the order of the operations is the corner
// list's all the same.  The positions come from the position records, which this kernel does not write: no thread reads what another
// writes.  A corner whose triangle lies beyond n_tri (never: the adjacency is made from the kept index list) leaves the vertex as it is
__global__ void __launch_bounds__(256) k_vertex_normals(KNormals p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.count) return;
    const uint32_t v = p.first + i;
    if (v >= p.n_vertex) return;                                    // (the host refused such a range)
    const float4* __restrict__ rec = reinterpret_cast<const float4*>(p.tripos);
    const uint32_t* __restrict__ corners = p.corners;
    uint32_t k = p.offsets[v], end = p.offsets[v + 1];
    if (end > p.n_index) end = p.n_index;
    const float4 va = p.verts[2 * (size_t)v], vb = p.verts[2 * (size_t)v + 1];
    F3 s = f3(0.0f, 0.0f, 0.0f);
    for (; k + 4u <= end; k += 4u) {                                 // (n_index <= 3 * 2^28: k + 4 does not wrap)
        const uint32_t t0 = corners[k] / 3u, t1 = corners[k + 1] / 3u, t2 = corners[k + 2] / 3u, t3 = corners[k + 3] / 3u;
        if (t0 >= p.n_tri || t1 >= p.n_tri || t2 >= p.n_tri || t3 >= p.n_tri) return;
        const float4 a0 = rec[3 * (size_t)t0], b0 = rec[3 * (size_t)t0 + 1], c0 = rec[3 * (size_t)t0 + 2];
        const float4 a1 = rec[3 * (size_t)t1], b1 = rec[3 * (size_t)t1 + 1], c1 = rec[3 * (size_t)t1 + 2];
        const float4 a2 = rec[3 * (size_t)t2], b2 = rec[3 * (size_t)t2 + 1], c2 = rec[3 * (size_t)t2 + 2];
        const float4 a3 = rec[3 * (size_t)t3], b3 = rec[3 * (size_t)t3 + 1], c3 = rec[3 * (size_t)t3 + 2];
        normals_add(s, a0, b0, c0);
        normals_add(s, a1, b1, c1);
        normals_add(s, a2, b2, c2);
        normals_add(s, a3, b3, c3);
    }
    for (; k < end; ++k) {
        const uint32_t t = corners[k] / 3u;
        if (t >= p.n_tri) return;
        normals_add(s, rec[3 * (size_t)t], rec[3 * (size_t)t + 1], rec[3 * (size_t)t + 2]);
    }
    const float d = (s.x * va.w + s.y * vb.x) + s.z * vb.y;         // the side of the normal the vertex holds
    if (d < 0.0f) s = -s;
    const float q = (s.x * s.x + s.y * s.y) + s.z * s.z;
    const float l = sqrtf(q);
    if (!(l > 0.0f && l <= FLT_MAX)) return;                        // no corner, no area, q beyond the range: the vertex keeps its bits
    const float nx = s.x / l;
    const float ny = s.y / l;
    const float nz = s.z / l;
    p.verts[2 * (size_t)v] = make_float4(va.x, va.y, va.z, nx);
    p.verts[2 * (size_t)v + 1] = make_float4(ny, nz, vb.z, vb.w);
}

// The adjacency of the scene's index list (RefitState: d_adj_offsets, d_adj_corners), behind whatever the stream still holds.  The corners
// are sorted by their vertex with the tree builds' stable LSD radix sort over the bits n_vertex needs: stable, so every vertex's corners
// stay ascending, which is the order the definition sums in -- a count / scan / fill-by-atomics build would leave every list in the
// order the atomics happened to resolve and need a sort per list behind it.  Everything is allocated before anything runs:
// TRC_ERR_OOM leaves nothing behind.  Waits for the device once, because the temporaries go when it returns
trc_status normals_adjacency(trc_ctx* ctx) {
    if (ctx->refit.d_adj_offsets) return TRC_OK;
    const uint32_t n_index = 3u * ctx->ks.sc.n_triangles, n_vertex = ctx->n_vertex;
    hipStream_t st = ctx->stream;
    DevBuf offsets, corners;
    DevBufs tmp;
    const char* const what = "trc_recompute_normals: adjacency";
    TRC_TRY(offsets.alloc(ctx, ((size_t)n_vertex + 1) * 4, what));
    TRC_TRY(corners.alloc(ctx, (size_t)n_index * 4, what));
    const uint32_t hist_words = trc_sort_hist_words(n_index);
    tmp.reserve(4 * ((size_t)n_index * 4 + 256) + (size_t)hist_words * 4 + 256 * 4 + 512);
    uint32_t *keys[2] = {}, *vals[2] = {}, *hist = nullptr, *digit_base = nullptr;
    for (uint32_t** q : {&keys[0], &keys[1], &vals[0], &vals[1]}) TRC_TRY(tmp.alloc(ctx, q, n_index, what));
    TRC_TRY(tmp.alloc(ctx, &hist, hist_words, what));
    TRC_TRY(tmp.alloc(ctx, &digit_base, 256, what));
    const dim3 grid((n_index + 255) / 256), b256(256);
    hipLaunchKernelGGL(k_adj_keys, grid, b256, 0, st, ctx->d_idx, n_index, keys[0], vals[0]);
    int cur = 0;
    trc_sort_pairs(st, keys, vals, hist, digit_base, n_index, trc_normals_key_bits(n_vertex), &cur);
    hipLaunchKernelGGL(k_adj_offsets, grid, b256, 0, st, keys[cur], n_index, n_vertex, offsets.as<uint32_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(corners.p, vals[cur], (size_t)n_index * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->refit.d_adj_offsets = static_cast<uint32_t*>(offsets.release());
    ctx->refit.d_adj_corners = static_cast<uint32_t*>(corners.release());
    return TRC_OK;
}

}  // namespace

// No vertex moves, so no box changes: the gather, then the attribute records of the triangles that name a vertex of the range, and that
// is the chain -- no k_refit_level, no root read-back, RefitState::pending stays what it was (before the first refit of a scene the root
// box on the device holds zeros, which must never reach ks.root_box), and no refit maps are made or waited for
extern "C" trc_status trc_recompute_normals(trc_ctx* ctx, uint32_t first, uint32_t count) {
    TRC_TRY(trc_enter_scene(ctx, "trc_recompute_normals"));
    if (count == 0) return TRC_OK;
    const DScene& sc = ctx->ks.sc;
    if (sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_recompute_normals: the scene has no triangles");
    if (const char* why = trc_normals_range_check(first, count, ctx->n_vertex)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_recompute_normals: ") + why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(trc_refit_events(ctx, "trc_recompute_normals"));
    TRC_TRY(normals_adjacency(ctx));
    KNormals p{};
    p.verts = reinterpret_cast<float4*>(ctx->d_verts); p.n_vertex = ctx->n_vertex;
    p.offsets = ctx->refit.d_adj_offsets; p.corners = ctx->refit.d_adj_corners; p.n_index = 3u * sc.n_triangles;
    p.tripos = ctx->d_blob + sc.off_tripos; p.n_tri = sc.n_triangles; p.first = first; p.count = count;
    TRC_TRY(trc_refit_open(ctx));
    hipLaunchKernelGGL(k_vertex_normals, dim3((uint32_t)(((size_t)count + 255) / 256)), dim3(256), 0, ctx->stream, p);
    // from here on the scene changed: what was derived from the old normals goes (the G-buffer's normal plane, the denoiser's history)
    trc_scene_changed(ctx, kSceneNormalsChanged);
    trc_refit_launch_triangles(ctx, first, count);
    TRC_TRY(trc_refit_close(ctx));
    if (ctx->cost_valid) { ctx->plan_streak = 0; ctx->cost_fresh_next = true; }      // as after trc_update_vertices: the block costs stay
    return TRC_OK;
}
