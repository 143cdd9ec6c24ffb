// trc_abi.hip -- the C ABI of libtracer_amd.so (gfx950 only): contexts, uploads with their setup kernels, the frame, the output stage, trc_trace_rays.
//
// Replaces, for the path-tracing hot path, the reference's Metal host glue
// (-[AAPLRenderer render:] AAPLRenderer.mm:1134-1196) and kernelPathTracing
// (RT_Metal/Metal/Render.metal:495-558).  See include/tracer_abi.h for the boundary and
// DESIGN.md for the data layout and kernel design.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "trc_ctx.hpp"
#include "trc_render_config.hpp"
#include "trc_scene_prep.hpp"

// deterministic stand-in for fillRNG (AAPLRenderer.mm:296-344): texel p = 4 outputs of
// pcg32_srandom_r(seed, p)
__global__ void __launch_bounds__(256) k_seed(uint32_t* rng, uint32_t n_pixels, uint64_t seed) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    Pcg r;
    r.state = 0;
    r.inc = ((uint64_t)p << 1u) | 1u;
    pcg_next(r);
    r.state += seed;
    pcg_next(r);
    uint4 out;
    out.x = pcg_next(r); out.y = pcg_next(r); out.z = pcg_next(r); out.w = pcg_next(r);
    reinterpret_cast<uint4*>(rng)[p] = out;
}

// blob triangle records from the caller's arrays (trc_scene_prep.hpp): one thread per triangle, 3 gathered 32-byte
// vertices in, 7 float4 out.  The attribute record's last dword is the triangle's material: 19 (Triangle.hh:82) until
// trc_upload_triangle_materials says otherwise
constexpr uint32_t kTriangleMaterial = 19u;
__global__ void __launch_bounds__(256) k_repack_triangles(const trc_TriangleVertex* __restrict__ verts, const uint32_t* __restrict__ idx,
                                                          uint32_t n_tri, float4* __restrict__ tripos, float4* __restrict__ triattr) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    const trc_TriangleVertex a = verts[idx[3 * t]], b = verts[idx[3 * t + 1]], c = verts[idx[3 * t + 2]];
    tripos[3 * (size_t)t] = make_float4(a.v[0], a.v[1], a.v[2], 0.0f);
    tripos[3 * (size_t)t + 1] = make_float4(b.v[0], b.v[1], b.v[2], 0.0f);
    tripos[3 * (size_t)t + 2] = make_float4(c.v[0], c.v[1], c.v[2], 0.0f);
    triattr[4 * (size_t)t] = make_float4(a.n[0], a.n[1], a.n[2], b.n[0]);
    triattr[4 * (size_t)t + 1] = make_float4(b.n[1], b.n[2], c.n[0], c.n[1]);
    triattr[4 * (size_t)t + 2] = make_float4(c.n[2], a.uv[0], a.uv[1], b.uv[0]);
    triattr[4 * (size_t)t + 3] = make_float4(b.uv[1], c.uv[0], c.uv[1], __uint_as_float(kTriangleMaterial));
}

// trc_upload_triangle_materials: dword 15 of every triangle's attribute record, from the caller's array (checked on the host:
// every index below n_material) or 19 for all (material == nullptr)
__global__ void __launch_bounds__(256) k_triangle_materials(const uint32_t* __restrict__ material, uint32_t n_tri, uint32_t* __restrict__ triattr) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    triattr[(size_t)t * kTriAttrDwords + 15u] = material ? material[t] : kTriangleMaterial;
}

// BVH::buildNode for the triangles (AAPLRenderer.mm:575-589 + BVH.hh:273-314): the box of the three vertices -- std::max({a, b, c}) /
// std::min({a, b, c}) keep the first of equals -- taken corner by corner through the identity matrix (column sums in the reference's
// order, so a -0 comes out as the host's arithmetic leaves it) into fmin / fmax from +-FLT_MAX (the second operand on a tie, as the
// host's minss / maxss).  One thread per triangle, one 64-byte leaf record out.
// dev_trileaf.hpp triangle_leaf_box restates this arithmetic as a function for trc_update_vertices: keep the two alike
// (tests/test_gpu_update_vertices_single.py holds them together).
__global__ void __launch_bounds__(256) k_triangle_leaves(const trc_TriangleVertex* __restrict__ verts, const uint32_t* __restrict__ idx,
                                                         uint32_t n_tri, trc_BVH* __restrict__ leaves) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    const trc_TriangleVertex a = verts[idx[3 * t]], b = verts[idx[3 * t + 1]], c = verts[idx[3 * t + 2]];
    float ele[2][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float hi = a.v[k]; if (hi < b.v[k]) hi = b.v[k]; if (hi < c.v[k]) hi = c.v[k];
        float lo = a.v[k]; if (b.v[k] < lo) lo = b.v[k]; if (c.v[k] < lo) lo = c.v[k];
        ele[0][k] = lo; ele[1][k] = hi;
    }
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float x = ele[i][0], y = ele[j][1], z = ele[k][2];
                const float w[3] = {1.0f * x + 0.0f * y + 0.0f * z + 0.0f * 1.0f, 0.0f * x + 1.0f * y + 0.0f * z + 0.0f * 1.0f,
                                    0.0f * x + 0.0f * y + 1.0f * z + 0.0f * 1.0f};
#pragma unroll
                for (int q = 0; q < 3; ++q) { mn[q] = mn[q] < w[q] ? mn[q] : w[q]; mx[q] = mx[q] > w[q] ? mx[q] : w[q]; }
            }
    trc_BVH r;
    memset(&r, 0, sizeof r);
    r.pType = TRC_PRIM_TRIANGLE; r.pIndex = t;
    r.bBOX.mini.x = mn[0]; r.bBOX.mini.y = mn[1]; r.bBOX.mini.z = mn[2];
    r.bBOX.maxi.x = mx[0]; r.bBOX.maxi.y = mx[1]; r.bBOX.maxi.z = mx[2];
    leaves[t] = r;
}

trc_status trc_repack_triangles(trc_ctx* ctx, const trc_scene* s, const DScene& sc, uint32_t* d_blob, trc_BVH* d_tri_leaves) {
    const uint32_t n_tri = s->n_index / 3;
    if (n_tri == 0) return TRC_OK;
    // the vertex and index arrays stay on the device beside the blob (32 B per vertex + 12 B per triangle): trc_update_vertices
    // rewrites the triangle records and the leaf boxes from them
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_verts, (size_t)s->n_vertex * sizeof(trc_TriangleVertex)));
    if (hipMalloc((void**)&ctx->d_idx, (size_t)s->n_index * 4) != hipSuccess) { trc_refit_free(ctx); return trc_fail(ctx, TRC_ERR_OOM, "hipMalloc triangle indices"); }
    ctx->n_vertex = s->n_vertex;
    auto failed = [&](const char* what) { trc_refit_free(ctx); return trc_fail(ctx, TRC_ERR_HIP, what); };      // the kept arrays belong to the context: freed first
    if (trc_copy_to_device(ctx, ctx->d_verts, s->triList, (size_t)s->n_vertex * sizeof(trc_TriangleVertex), ctx->stream) != TRC_OK ||
        trc_copy_to_device(ctx, ctx->d_idx, s->idxList, (size_t)s->n_index * 4, ctx->stream) != TRC_OK) return failed("H2D triangles");
    hipLaunchKernelGGL(k_repack_triangles, dim3((n_tri + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_verts, ctx->d_idx, n_tri,
                       reinterpret_cast<float4*>(d_blob + sc.off_tripos), reinterpret_cast<float4*>(d_blob + sc.off_triattr));
    if (d_tri_leaves) hipLaunchKernelGGL(k_triangle_leaves, dim3((n_tri + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_verts, ctx->d_idx, n_tri, d_tri_leaves);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return failed("k_repack_triangles");
    return TRC_OK;
}

// the counters' rows (stat_row) summed into one row
__global__ void __launch_bounds__(64) k_stats_sum(const unsigned long long* rows, unsigned long long* sum) {
    const uint32_t c = threadIdx.x;
    if (c >= kStatRowStride) return;
    unsigned long long v = 0;
    for (uint32_t r = 0; r < kStatRows; ++r) v += rows[(size_t)r * kStatRowStride + c];
    sum[c] = v;
}
trc_status trc_read_stats_sum(trc_ctx* ctx, unsigned long long* h, size_t count) {
    hipLaunchKernelGGL(k_stats_sum, dim3(1), dim3(64), 0, ctx->stream, ctx->d_stats, ctx->d_stats_sum);
    return trc_read_to_host(ctx, ctx->stream, "stats sum", {{h, ctx->d_stats_sum, count * sizeof *h}});
}

// ---- output stage (fragmentShader, Render.metal:29-75): exposure sums, then ACES to 8 bit
__global__ void __launch_bounds__(256) k_tonemap_sum(const float4* accum, uint32_t n, unsigned long long* sums /* [3] */) {
    unsigned long long s[3] = {0, 0, 0};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float4 px = accum[i];
        const float c[3] = {px.x, px.y, px.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = c[k];
            if (!(v > 0.0f)) v = 0.0f;
            if (v > 1048576.0f) v = 1048576.0f;
            s[k] += (unsigned long long)(v * 65536.0f + 0.5f);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off, 64);
        if ((threadIdx.x & 63u) == 0) atomicAdd(&sums[k], s[k]);
    }
}
__global__ void __launch_bounds__(256) k_tonemap(const float4* accum, uint32_t W, uint32_t H, float expose, uchar4* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t y = i / W, x = i - y * W;
    const float4 px = accum[(size_t)(H - 1u - y) * W + x];
    const float A = 2.51f, B = 0.03f, Cc = 2.43f, D = 0.59f, E = 0.14f;
    const float c[3] = {px.x, px.y, px.z};
    uint32_t o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float col = c[k] * expose;
        float t = (col * (A * col + B)) / (col * (Cc * col + D) + E);        // ACESTone, Render.hh:78-89
        if (!(t > 0.0f)) t = 0.0f;
        if (t > 1.0f) t = 1.0f;
        o[k] = (uint32_t)(t * 255.0f + 0.5f);
    }
    out[i] = make_uchar4((unsigned char)o[0], (unsigned char)o[1], (unsigned char)o[2], 255);
}

// Scene::hit test hook: one lane per ray, full HitRecord + per-ray traversal counters.  STATS = true is the plain
// round with the exact counters; STATS = false is the traversal the render kernels run (speculative round,
// dev_intersect.hpp::trav_iter), counters left at zero.
template <bool LDS, bool ANY, bool STATS>
__global__ void __launch_bounds__(kBlock) k_trace(const KTrace kp) {
    const DScene& sc = kp.ks.sc;
    const uint32_t* small_base = stage_scene(sc);
    uint32_t* stack = lane_stack(sc);
    uint32_t* lvstack = lane_lvstack(sc);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= kp.n) return;
    const trc_ray in = kp.rays[i];
    SceneRef S = make_scene_ref(sc, small_base);
    Ray ray = make_ray(f3(in.origin[0], in.origin[1], in.origin[2]), f3(in.direction[0], in.direction[1], in.direction[2]));
    HitRec rec;
    hit_init(rec);
    TravCounters cnt;
    counters_zero(cnt);
    constexpr bool kOrderFree = ANY && !STATS;      // the production kernels' shadow-ray walk: only the answer is defined
    const F3 root_min = f3(kp.ks.root_box[0], kp.ks.root_box[1], kp.ks.root_box[2]), root_max = f3(kp.ks.root_box[3], kp.ks.root_box[4], kp.ks.root_box[5]);
    bool h;
    if (kOrderFree) h = scene_occluded<LDS, false, false>(S, root_min, root_max, ray, in.tmax, stack, sc.stack_lds);
    else h = scene_hit<LDS, STATS, ANY, true, false, false, (STATS || ANY) ? 0 : (LDS ? TRC_DEFER_LDS : TRC_DEFER_GLOBAL)>(S, root_min, root_max, ray, rec, in.tmax, stack, lvstack, cnt);
    trc_hit o;
    memset(&o, 0, sizeof o);
    o.hit = h ? 1 : 0;
    o.pType = -1;
    if (h && !kOrderFree) {
        o.pType = (int32_t)(rec.tag >> kTagIndexBits);
        o.pIndex = rec.tag & kTagIndexMask;
        o.t = rec.t;
        o.p[0] = rec.p.x; o.p[1] = rec.p.y; o.p[2] = rec.p.z;
        o.gn[0] = rec.gn.x; o.gn[1] = rec.gn.y; o.gn[2] = rec.gn.z;
        o.sn[0] = rec.sn.x; o.sn[1] = rec.sn.y; o.sn[2] = rec.sn.z;
        o.uv[0] = rec.uv.x; o.uv[1] = rec.uv.y;
        o.material = rec.material;
        o.PDF = rec.PDF;
    }
    o.n_descend = cnt.n_descend;
    o.n_return = cnt.n_return;
    o.n_leaf = cnt.leaf[0] + cnt.leaf[1] + cnt.leaf[2] + cnt.leaf[3];
    kp.hits[i] = o;
}

// ======================================================================= host side
// folds the per-launch event pairs that have already completed into kernel_ms without waiting (oldest first; the
// stream is in order, so the first unfinished pair ends the scan).  Called from trc_render, so a host that never
// synchronises through trc_synchronize / trc_get_stats (one launch + one download per frame, the reference's own
// pattern) keeps a bounded list.
using EventPairs = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
static void collect_finished(trc_ctx* ctx, EventPairs& list, double& ms_sum) {
    size_t done = 0;
    for (; done < list.size(); ++done) {
        const hipError_t q = hipEventQuery(list[done].second);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); break; }      // "not ready" is reported through the sticky error too
        if (q != hipSuccess) break;                                        // a real error stays for the caller's next check
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, list[done].first, list[done].second) == hipSuccess) ms_sum += ms;
        ctx->event_pool.push_back(list[done].first);
        ctx->event_pool.push_back(list[done].second);
    }
    list.erase(list.begin(), list.begin() + (ptrdiff_t)done);
}
void trc_collect_finished_events(trc_ctx* ctx) {
    collect_finished(ctx, ctx->pending, ctx->kernel_ms);
    collect_finished(ctx, ctx->pending_sched, ctx->schedule_ms);      // the launch-list kernels' pairs
}

namespace {

// drains every per-launch event pair into kernel_ms / schedule_ms (call after a stream sync)
void collect_events(trc_ctx* ctx) {
    auto drain = [&](EventPairs& list, double& ms_sum) {
        for (auto& pr : list) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) ms_sum += ms;
            ctx->event_pool.push_back(pr.first);
            ctx->event_pool.push_back(pr.second);
        }
        list.clear();
    };
    drain(ctx->pending, ctx->kernel_ms);
    drain(ctx->pending_sched, ctx->schedule_ms);
}

// Repack the reference arrays into the device layout (dev_scene.hpp) and validate the tree.
trc_status build_blob(trc_ctx* ctx, const trc_scene* s, std::vector<uint32_t>& blob, uint64_t& blob_total, KScene& ks) {
    if (!s || !s->bvhList || s->n_bvh < 3 || (s->n_bvh & 1u) == 0) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "scene: need >= 2 leaves (n_bvh odd, >= 3)");
    TRC_TRY(validate_primitives(ctx, s));
    const trc_BVH* nodes = s->bvhList;
    const uint32_t n = s->n_bvh;
    if (nodes[0].pType != TRC_PRIM_BVH) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: root is not an interior node");

    // BFS over interior nodes: compact ids, depth, validation
    std::vector<uint32_t> interior_id(n, 0xFFFFFFFFu), order, depth_of(n, 0);
    order.reserve(n / 2 + 1);
    order.push_back(0);
    interior_id[0] = 0;
    uint32_t visited = 1, max_leaf_depth = 0;
    for (size_t h = 0; h < order.size(); ++h) {
        const uint32_t i = order[h];
        const uint32_t kids[2] = {nodes[i].left, nodes[i].right};
        if (kids[0] == kids[1]) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: left == right");
        for (uint32_t c : kids) {
            if (c == 0 || c >= n) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: child index out of range");
            if (++visited > n) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: cycle");
            depth_of[c] = depth_of[i] + 1;
            if (nodes[c].pType == TRC_PRIM_BVH) {
                if (interior_id[c] != 0xFFFFFFFFu) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: node reached twice");
                interior_id[c] = (uint32_t)order.size();
                order.push_back(c);
            } else {
                max_leaf_depth = std::max(max_leaf_depth, depth_of[c]);
                TRC_TRY(validate_leaf(ctx, s, nodes[c]));
            }
        }
    }
    if (visited != n) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: unreachable nodes");
    if (max_leaf_depth > TRC_MAX_BVH_DEPTH) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "bvh: deeper than TRC_MAX_BVH_DEPTH");

    const uint32_t n_interior = (uint32_t)order.size();
    DScene sc{};
    uint64_t total = 0;
    TRC_TRY(layout_scene(ctx, s, n_interior, sc, total));
    plan_lds(sc, max_leaf_depth, true);
    blob.assign((size_t)sc.off_tripos, 0u);      // analytic primitives, materials, fat nodes; triangle records are made on the device
    blob_total = total;

    auto tag_of = [&](uint32_t c) -> uint32_t {
        if (nodes[c].pType == TRC_PRIM_BVH) return (kTagInterior << kTagIndexBits) | interior_id[c];
        return ((uint32_t)nodes[c].pType << kTagIndexBits) | nodes[c].pIndex;
    };
    prep_parallel_for(n_interior, [&](size_t kb, size_t ke) {
        for (size_t k = kb; k < ke; ++k) {
            const trc_BVH& nd = nodes[order[k]];
            const trc_AABB& L = nodes[nd.left].bBOX;
            const trc_AABB& R = nodes[nd.right].bBOX;
            uint32_t* q = &blob[sc.off_nodes + k * kNodeDwords];
            q[0] = f2u(L.mini.x); q[1] = f2u(L.mini.y); q[2] = f2u(L.mini.z); q[3] = f2u(L.maxi.x);
            q[4] = f2u(L.maxi.y); q[5] = f2u(L.maxi.z); q[6] = f2u(R.mini.x); q[7] = f2u(R.mini.y);
            q[8] = f2u(R.mini.z); q[9] = f2u(R.maxi.x); q[10] = f2u(R.maxi.y); q[11] = f2u(R.maxi.z);
            q[12] = 0; q[13] = 0; q[14] = tag_of(nd.left); q[15] = tag_of(nd.right);
        }
    });
    fill_primitives(s, sc, blob.data());
    ks.sc = sc;
    const trc_AABB& rb = nodes[0].bBOX;
    ks.root_box[0] = rb.mini.x; ks.root_box[1] = rb.mini.y; ks.root_box[2] = rb.mini.z;
    ks.root_box[3] = rb.maxi.x; ks.root_box[4] = rb.maxi.y; ks.root_box[5] = rb.maxi.z;
    return TRC_OK;
}

}  // namespace

hipEvent_t trc_get_event(trc_ctx* ctx) {
    if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// ----------------------------------------------------------------------- transfers through pinned staging (trc_ctx.hpp)
static trc_status xfer_ready(trc_ctx* ctx) {
    if (ctx->h_xfer) return TRC_OK;
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_xfer, 2 * kXferChunk, hipHostMallocDefault));
    for (hipEvent_t& e : ctx->ev_xfer) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return TRC_OK;
}
trc_status trc_copy_to_host(trc_ctx* ctx, void* host, const void* dev, size_t bytes, hipStream_t st) {
    if (bytes == 0) return TRC_OK;
    TRC_TRY(xfer_ready(ctx));
    size_t prev_off = 0, prev_n = 0;
    int slot = 0;
    for (size_t off = 0; off < bytes; off += kXferChunk, slot ^= 1) {
        const size_t n = std::min(kXferChunk, bytes - off);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_xfer + slot * kXferChunk, static_cast<const char*>(dev) + off, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_xfer[slot], st));
        if (prev_n) {                                     // the chunk before, while this one is on its way
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev_xfer[slot ^ 1]));
            std::memcpy(static_cast<char*>(host) + prev_off, ctx->h_xfer + (slot ^ 1) * kXferChunk, prev_n);
        }
        prev_off = off; prev_n = n;
    }
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_xfer[slot ^ 1]));
    std::memcpy(static_cast<char*>(host) + prev_off, ctx->h_xfer + (slot ^ 1) * kXferChunk, prev_n);
    return TRC_OK;
}
trc_status trc_copy_to_device(trc_ctx* ctx, void* dev, const void* host, size_t bytes, hipStream_t st) {
    if (bytes == 0) return TRC_OK;
    TRC_TRY(xfer_ready(ctx));
    int slot = 0;
    bool used[2] = {false, false};
    for (size_t off = 0; off < bytes; off += kXferChunk, slot ^= 1) {
        const size_t n = std::min(kXferChunk, bytes - off);
        if (used[slot]) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_xfer[slot]));       // the copy that last read this half has finished
        std::memcpy(ctx->h_xfer + slot * kXferChunk, static_cast<const char*>(host) + off, n);
        HIP_TRY(ctx, hipMemcpyAsync(static_cast<char*>(dev) + off, ctx->h_xfer + slot * kXferChunk, n, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_xfer[slot], st));
        used[slot] = true;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return TRC_OK;
}

trc_status trc_read_to_host(trc_ctx* ctx, hipStream_t st, const char* what, std::initializer_list<trc_read_item> items) {
    TRC_TRY(xfer_ready(ctx));
    hipError_t e = hipGetLastError();
    size_t off = 0;
    for (const trc_read_item& it : items) {
        if (e == hipSuccess) e = off + it.bytes <= kXferChunk ? hipMemcpyAsync(ctx->h_xfer + off, it.dev, it.bytes, hipMemcpyDeviceToHost, st) : hipErrorInvalidValue;
        off += (it.bytes + 15u) & ~(size_t)15u;
    }
    const hipError_t sync = hipStreamSynchronize(st);      // also after a failure: nothing of this call is in flight on return
    if (e == hipSuccess) e = sync;
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    off = 0;
    for (const trc_read_item& it : items) { std::memcpy(it.host, ctx->h_xfer + off, it.bytes); off += (it.bytes + 15u) & ~(size_t)15u; }
    return TRC_OK;
}

// ----------------------------------------------------------------------- what is stale now, and who frees what (trc_ctx.hpp)
void trc_release_scene(trc_ctx* ctx) {
    (void)hipFree(ctx->d_blob); ctx->d_blob = nullptr;
    (void)hipFree(ctx->d_bvh_ref); ctx->d_bvh_ref = nullptr; ctx->n_bvh_ref = 0;
    (void)hipFree(ctx->d_vis); ctx->d_vis = nullptr;      // trc_set_triangle_visibility: the next tree defines the mask again
    ctx->has_scene = false;
    trc_mesh_light_free(ctx);
    trc_material_params_release(ctx);      // the table of TRC_FLAG_MATERIAL_PARAMS names this scene's materials
    trc_refit_free(ctx);
    trc_denoise_scene_released(ctx);
}

void trc_adopt_scene(trc_ctx* ctx, KScene ks, const trc_scene* s) {
    ks.sc.blob = ctx->d_blob;
    ctx->ks = ks;
    ctx->lds_scene = ks.sc.n_lds_nodes == ks.sc.n_nodes;      // whole tree staged in LDS
    ctx->lds_prefix_ok = ctx->has_scene = true;
    ctx->scene_min_image = trc_scene_min_image(s);
}

void trc_scene_changed(trc_ctx* ctx, SceneChange kind) {
    const bool in_place = kind == kSceneVerticesMoved || kind == kSceneNormalsChanged || kind == kSceneTreeRebuilt || kind == kScenePrimitivesMoved;
    if (in_place) trc_denoise_moved(ctx, kind == kSceneVerticesMoved || kind == kScenePrimitivesMoved);
    else trc_picture_changed(ctx);
    if (!in_place) trc_forget_costs(ctx);
    if (kind == kSceneTreeRebuilt) trc_refit_free_maps(ctx);
    if (kind != kSceneReplaced) { trc_mesh_light_free(ctx); return; }
    ctx->tri_materials = false;
    trc_release_scene(ctx);
}

void trc_release_frame(trc_ctx* ctx) {
    (void)hipFree(ctx->d_rng); (void)hipFree(ctx->d_accum); (void)hipFree(ctx->d_accum_alt); (void)hipFree(ctx->d_reduce_recv);
    ctx->d_rng = nullptr; ctx->d_accum = nullptr; ctx->d_accum_alt = nullptr; ctx->d_composed = nullptr; ctx->d_reduce_recv = nullptr;
    (void)hipFree(ctx->d_shard_in); (void)hipFree(ctx->d_shard_out); (void)hipFree(ctx->d_shard_src);
    ctx->d_shard_in = ctx->d_shard_out = ctx->d_shard_src = nullptr; ctx->shard_px = 0; ctx->shard_nranks = 0; ctx->snapshot_busy = false;
    ctx->busy = ctx->busy_alt = false;
    trc_sppm_release(ctx);          // per-pixel camera records depend on the frame size
    trc_denoise_release(ctx);       // ... and so do the denoiser's planes
    trc_adaptive_release(ctx);      // ... the tile mask, the snapshot and the per-tile estimate
    trc_camera_rays_release(ctx);   // ... and the ray sets of TRC_FLAG_CAMERA_RAYS
    trc_release_tiles(ctx);
    ctx->n_tiles = 0;
    ctx->width = ctx->height = 0;
}

static void release_density(trc_ctx* ctx) {
    (void)hipFree(ctx->d_density); ctx->d_density = nullptr;
    (void)hipFree(ctx->d_occupancy); ctx->d_occupancy = nullptr;
    ctx->dinfo = trc_GridDensityInfo{};
}
static void release_environment_map(trc_ctx* ctx) {
    (void)hipFree(ctx->d_envmap); ctx->d_envmap = nullptr; ctx->env_w = ctx->env_h = 0;
    trc_env_light_free(ctx);                                             // TRC_FLAG_ENV_LIGHT: rebuilt for the new map when a launch asks
}
static void release_textures(trc_ctx* ctx) {
    (void)hipFree(ctx->d_tex_texels); (void)hipFree(ctx->d_tex_desc);
    ctx->d_tex_texels = nullptr; ctx->d_tex_desc = nullptr; ctx->n_tex = 0;
}

// The knobs (trc_ctx::Knobs) by name, each once: what trc_debug_set calls it, its member, and the environment variable trc_create reads
// its default from (null: none) -- a flag (1 when the variable is present) or a number (max(0, atoi)).  The list in tracer_abi.h
// (trc_debug_set) describes them to a caller.
struct KnobEntry { const char* name; int trc_ctx::Knobs::*slot; const char* env; bool env_flag; };
static const KnobEntry kKnobs[] = {
    {"no_lds_fit", &trc_ctx::Knobs::no_lds_fit, "TRC_NO_LDS_FIT", true},
    {"stack_lds_levels", &trc_ctx::Knobs::stack_lds_levels, "TRC_STACK_LDS_LEVELS", false},
    {"strip_len", &trc_ctx::Knobs::strip_len, "TRC_STRIP_LEN", false},
    {"no_pwg", &trc_ctx::Knobs::no_pwg, "TRC_NO_PWG", true},
    {"sppm_serial_camera", &trc_ctx::Knobs::sppm_serial_camera, "TRC_SPPM_SERIAL_CAMERA", true},
    {"sppm_timing", &trc_ctx::Knobs::sppm_timing, nullptr, false},
    {"force_blk_shift", &trc_ctx::Knobs::force_blk_shift, nullptr, false},
    {"no_split", &trc_ctx::Knobs::no_split, nullptr, false},
    {"no_cost_filter", &trc_ctx::Knobs::no_cost_filter, "TRC_NO_COST_FILTER", true},
    {"no_cold_probe", &trc_ctx::Knobs::no_cold_probe, "TRC_NO_COLD_PROBE", true},
    {"probe_spp", &trc_ctx::Knobs::probe_spp, "TRC_PROBE_SPP", false},
    {"no_plan_reuse", &trc_ctx::Knobs::no_plan_reuse, "TRC_NO_PLAN_REUSE", true},
    {"no_coalesce", &trc_ctx::Knobs::no_coalesce, "TRC_NO_COALESCE", true},
    {"no_dense", &trc_ctx::Knobs::no_dense, "TRC_NO_DENSE", true},
    {"head_stages", &trc_ctx::Knobs::head_stages, "TRC_HEAD_STAGES", false},
    {"descend_min", &trc_ctx::Knobs::descend_min, nullptr, false},
    {"camera_policy", &trc_ctx::Knobs::camera_policy, nullptr, false},
    {"no_primary_replay", &trc_ctx::Knobs::no_primary_replay, nullptr, false},
    {"replay_min_lanes", &trc_ctx::Knobs::replay_min_lanes, nullptr, false},
    {"replay_chain", &trc_ctx::Knobs::replay_chain, nullptr, false},
    {"mesh_light_pick", &trc_ctx::Knobs::mesh_light_pick, nullptr, false},
    {"refit_single", &trc_ctx::Knobs::refit_single, nullptr, false},
    {"skin_no_lds", &trc_ctx::Knobs::skin_no_lds, nullptr, false},
    {"strip_force", &trc_ctx::Knobs::strip_force, nullptr, false},
    {"mask_forgets_costs", &trc_ctx::Knobs::mask_forgets_costs, nullptr, false},
};

// ======================================================================= C ABI
extern "C" {

uint32_t trc_abi_version(void) { return TRC_ABI_VERSION; }

const char* trc_build_flavor(void) {
#ifdef TRC_FAST_MATH
    return "fast-math";
#else
    return "exact";
#endif
}

const char* trc_status_string(trc_status s) {
    switch (s) {
        case TRC_OK: return "ok";
        case TRC_ERR_INVALID_ARG: return "invalid argument";
        case TRC_ERR_NO_DEVICE: return "no usable HIP device";
        case TRC_ERR_HIP: return "HIP runtime error";
        case TRC_ERR_NO_SCENE: return "no scene uploaded";
        case TRC_ERR_NO_FRAME: return "no frame allocated (trc_resize)";
        case TRC_ERR_BVH_INVALID: return "invalid BVH";
        case TRC_ERR_UNSUPPORTED: return "unsupported";
        case TRC_ERR_RCCL: return "RCCL error";
        case TRC_ERR_OOM: return "out of memory";
        default: return "unknown status";
    }
}

const char* trc_last_error(const trc_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

trc_status trc_create(int device, trc_ctx** out) {
    if (!out) return TRC_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return TRC_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return TRC_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return TRC_ERR_NO_DEVICE;
    trc_ctx* ctx = new (std::nothrow) trc_ctx();
    if (!ctx) return TRC_ERR_OOM;
    ctx->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) ctx->cu_count = cus; }
    if (ctx->cu_count <= 0) ctx->cu_count = 256;
    for (const KnobEntry& k : kKnobs)
        if (const char* v = k.env ? std::getenv(k.env) : nullptr) ctx->knobs.*k.slot = k.env_flag ? 1 : std::max(0, std::atoi(v));
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&ctx->d_stats, sizeof(unsigned long long) * kStatRows * kStatRowStride) != hipSuccess ||
        hipMalloc((void**)&ctx->d_stats_sum, sizeof(unsigned long long) * kStatRowStride) != hipSuccess ||
        hipMemsetAsync(ctx->d_stats, 0, sizeof(unsigned long long) * kStatRows * kStatRowStride, ctx->stream) != hipSuccess) {
        trc_destroy(ctx);
        return TRC_ERR_HIP;
    }
    *out = ctx;
    return TRC_OK;
}

void trc_destroy(trc_ctx* ctx) {
    if (!ctx) return;
    // nobody can read the frame of a kept launch after this call: it is dropped, not launched (trc_synchronize, a download or
    // trc_get_stats before trc_destroy launches it and reports its status)
    ctx->has_deferred = false;
    if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
    trc_release_frame(ctx);
    collect_events(ctx);
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    trc_release_scene(ctx); release_density(ctx); release_environment_map(ctx); release_textures(ctx);
    (void)hipFree(ctx->d_sobol32); (void)hipFree(ctx->d_sobol_vdc); (void)hipFree(ctx->d_stats); (void)hipFree(ctx->d_stats_sum); (void)hipFree(ctx->d_plan);
    (void)hipFree(ctx->d_stack_ovf); (void)hipFree(ctx->d_memo); (void)hipFree(ctx->d_queue);
    if (ctx->ev_snapshot_free) (void)hipEventDestroy(ctx->ev_snapshot_free);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->h_xfer) (void)hipHostFree(ctx->h_xfer);
    for (hipEvent_t e : ctx->ev_xfer) if (e) (void)hipEventDestroy(e);
    if (ctx->h_readback) (void)hipHostFree(ctx->h_readback);
    for (hipEvent_t e : {ctx->ev_rendered, ctx->ev_busy, ctx->ev_busy_alt}) if (e) (void)hipEventDestroy(e);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

trc_status trc_upload_scene(trc_ctx* ctx, const trc_scene* scene) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> blob;
    uint64_t blob_total = 0;
    KScene ks{};
    TRC_TRY(build_blob(ctx, scene, blob, blob_total, ks));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    trc_scene_changed(ctx, kSceneReplaced);      // another scene: the old one goes, with everything derived from it
    ctx->blob_bytes = (size_t)blob_total * 4;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_blob, ctx->blob_bytes));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_blob, blob.data(), blob.size() * 4, ctx->stream));
    TRC_TRY(trc_repack_triangles(ctx, scene, ks.sc, ctx->d_blob, nullptr));      // synchronous, as the copy before it
    trc_adopt_scene(ctx, ks, scene);
    return TRC_OK;
}

trc_status trc_upload_density(trc_ctx* ctx, const trc_GridDensityInfo* info, const float* density) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    release_density(ctx);
    if (!info && !density) return TRC_OK;                                  // cleared
    if (!info || !density || info->nx == 0 || info->ny == 0 || info->nz == 0) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_density: empty grid");
    const uint64_t count = (uint64_t)info->nx * info->ny * info->nz;
    if (count > (1ull << 31)) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_upload_density: more than 2^31 cells");
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_density, count * sizeof(float)));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_density, density, count * sizeof(float), ctx->stream));
    // occupancy of 4x4x4 bricks: brick b covers lookups whose base cell i = floor(p*n - 0.5) has (i + 1) >> 2 == b, i.e.
    // the cells 4b-1 .. 4b+3 and their +1 neighbours; nonzero = any of them holds a value other than +0
    const int nx = (int)info->nx, ny = (int)info->ny, nz = (int)info->nz;
    const int nbx = (nx + 4) >> 2, nby = (ny + 4) >> 2, nbz = (nz + 4) >> 2;
    std::vector<uint8_t> occ((size_t)nbx * nby * nbz, 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const float v = density[((size_t)z * ny + y) * nx + x];
                uint32_t bits; std::memcpy(&bits, &v, 4);
                if (bits == 0u) continue;                                   // exactly +0: interpolates to +0
                // cell c is touched by base cells c-1 and c: bricks (c >> 2) and ((c + 1) >> 2)
                for (int bz = z >> 2; bz <= (z + 1) >> 2; ++bz)
                    for (int by = y >> 2; by <= (y + 1) >> 2; ++by)
                        for (int bx = x >> 2; bx <= (x + 1) >> 2; ++bx) occ[((size_t)bz * nby + by) * nbx + bx] = 1;
            }
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_occupancy, occ.size()));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_occupancy, occ.data(), occ.size(), ctx->stream));
    ctx->dinfo = *info;
    return TRC_OK;
}

trc_status trc_set_camera(trc_ctx* ctx, const trc_Camera* c) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !c) return TRC_ERR_INVALID_ARG;
    const DCamera before = ctx->cam;
    DCamera& d = ctx->cam;
    const trc_float3* src[6] = {&c->lookFrom, &c->u, &c->v, &c->vertical, &c->horizontal, &c->cornerLowLeft};
    float* dst[6] = {d.lookFrom, d.u, d.v, d.vertical, d.horizontal, d.cornerLowLeft};
    for (int i = 0; i < 6; ++i) { dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z; }
    d.lenRadius = c->lenRadius;
    // another view: the blocks' recorded costs are another picture's (the next launch measures afresh: trc_render's head)
    // (the old view's launch order survives as a PRIOR for the head of the next launch: a camera usually moves a little)
    // Round 6 (tools/moving_camera.py, profiles/r06/moving_camera.txt): a camera that moves a LITTLE -- a drag, frame after frame -- keeps the
    // recorded costs: the next launch is ordered and planned by them as one pass, taking the last launch's RAW durations (the filter follows
    // a block that got heavier by 1.6 % per launch only).  Under a camera that moves 0.5 degrees per frame that costs 4-8 % over a settled
    // launch where forgetting the costs (head + rest on every view) costs 8-24 %.  A camera that JUMPS -- the view direction turns by more
    // than 5 degrees or the eye moves by more than 5 % of the scene's diagonal -- looks at another picture: the costs are forgotten as before.
    // Knob camera_policy: 0 = this rule, 1 = always forget, 2 = always keep (filtered costs), 3 = always keep (raw durations).
    if (!ctx->has_camera || std::memcmp(&before, &d, sizeof d) != 0) {
        auto centre = [](const DCamera& c, float out[3]) {      // direction of the view's centre ray
            float n = 0.0f;
            for (int k = 0; k < 3; ++k) { out[k] = c.cornerLowLeft[k] + 0.5f * c.horizontal[k] + 0.5f * c.vertical[k] - c.lookFrom[k]; n += out[k] * out[k]; }
            n = n > 0.0f ? 1.0f / std::sqrt(n) : 0.0f;
            for (int k = 0; k < 3; ++k) out[k] *= n;
        };
        bool small = false;
        if (ctx->has_camera && ctx->has_scene) {
            float a[3], b[3], cosang = 0.0f, shift = 0.0f, diag = 0.0f;
            centre(before, a); centre(d, b);
            for (int k = 0; k < 3; ++k) {
                cosang += a[k] * b[k];
                shift += (d.lookFrom[k] - before.lookFrom[k]) * (d.lookFrom[k] - before.lookFrom[k]);
                diag += (ctx->ks.root_box[3 + k] - ctx->ks.root_box[k]) * (ctx->ks.root_box[3 + k] - ctx->ks.root_box[k]);
            }
            small = cosang >= 0.9961947f /* cos 5 degrees */ && shift <= 0.0025f * diag;
        }
        const int policy = ctx->knobs.camera_policy;
        const bool keep = ctx->cost_valid && (policy == 0 ? small : policy >= 2);
        if (keep) { ctx->plan_streak = 0; ctx->cost_fresh_next = policy != 2; }
        else { if (ctx->cost_valid) ctx->d_stale_order = ctx->d_last_order; ctx->cost_valid = false; ctx->d_last_order = nullptr; }
    }
    ctx->has_camera = true;
    return TRC_OK;
}

trc_status trc_set_environment(trc_ctx* ctx, const float rgb[3]) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !rgb) return TRC_ERR_INVALID_ARG;
    ctx->ambient[0] = rgb[0]; ctx->ambient[1] = rgb[1]; ctx->ambient[2] = rgb[2];
    trc_picture_changed(ctx);
    return TRC_OK;
}

trc_status trc_set_environment_map(trc_ctx* ctx, uint32_t w, uint32_t h, const float* rgb) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    release_environment_map(ctx);
    trc_picture_changed(ctx);
    if (!rgb) return TRC_OK;                                             // back to the constant environment
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 28)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_set_environment_map: bad size");
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_envmap, bytes));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_envmap, rgb, bytes, ctx->stream));
    ctx->env_w = w; ctx->env_h = h;
    return TRC_OK;
}

// image textures: all images in one pool of RGB float texels (3 per texel, each image's rows bottom-up, the layout the caller
// gives), and a descriptor {first texel, w, h, 0} per image; hit_color<true> (dev_integrator.hpp) reads both
trc_status trc_upload_textures(trc_ctx* ctx, const trc_image* images, uint32_t n) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (n && !images) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_textures: images == NULL");
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const trc_image& im = images[i];
        if (im.width == 0 || im.height == 0 || !im.rgb) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_textures: zero size or NULL rgb");
        if ((uint64_t)im.width * im.height > (1ull << 28)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_textures: image larger than 2^28 texels");
        const size_t count = (size_t)im.width * im.height * 3;
        for (size_t k = 0; k < count; ++k)
            if (!std::isfinite(im.rgb[k])) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_textures: non-finite texel");
        total += (uint64_t)im.width * im.height;
    }
    if (total > 0xFFFFFFFFull) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_textures: more than 2^32 texels in all");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    release_textures(ctx);
    trc_picture_changed(ctx);
    if (n == 0) return TRC_OK;
    std::vector<uint4> desc(n);
    uint64_t first = 0;
    for (uint32_t i = 0; i < n; ++i) {
        desc[i] = make_uint4((uint32_t)first, images[i].width, images[i].height, 0u);
        first += (uint64_t)images[i].width * images[i].height;
    }
    if (hipMalloc((void**)&ctx->d_tex_texels, (size_t)total * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&ctx->d_tex_desc, n * sizeof(uint4)) != hipSuccess) {
        (void)hipGetLastError();
        release_textures(ctx);
        return trc_fail(ctx, TRC_ERR_OOM, "trc_upload_textures: device allocation failed");
    }
    trc_status cs = trc_copy_to_device(ctx, ctx->d_tex_desc, desc.data(), n * sizeof(uint4), ctx->stream);
    for (uint32_t i = 0; i < n && cs == TRC_OK; ++i)
        cs = trc_copy_to_device(ctx, ctx->d_tex_texels + 3 * (size_t)desc[i].x, images[i].rgb, (size_t)images[i].width * images[i].height * 3 * sizeof(float), ctx->stream);
    if (cs == TRC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) cs = trc_fail(ctx, TRC_ERR_HIP, "trc_upload_textures: copy");
    if (cs != TRC_OK) { release_textures(ctx); return cs; }
    ctx->n_tex = n;
    return TRC_OK;
}

// per-triangle materials: dword 15 of the triangle attribute records (dev_scene.hpp), which every scene upload sets to 19
trc_status trc_upload_triangle_materials(trc_ctx* ctx, const uint32_t* material, uint32_t n_triangles) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_upload_triangle_materials: no scene");
    const DScene& sc = ctx->ks.sc;
    if (material || n_triangles) {
        if (!material) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_triangle_materials: material == NULL with n_triangles > 0");
        if (n_triangles != sc.n_triangles) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_triangle_materials: n_triangles != the scene's n_index / 3");
        for (uint32_t t = 0; t < n_triangles; ++t)
            if (material[t] >= sc.n_materials) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_triangle_materials: material index out of range");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sc.n_triangles) {
        DevBuf mat;                 // stays null for "19 for all"
        if (material) {
            TRC_TRY(mat.alloc(ctx, (size_t)sc.n_triangles * 4, "triangle materials"));
            TRC_TRY(trc_copy_to_device(ctx, mat.p, material, (size_t)sc.n_triangles * 4, ctx->stream));
        }
        hipLaunchKernelGGL(k_triangle_materials, dim3((sc.n_triangles + 255) / 256), dim3(256), 0, ctx->stream, mat.as<uint32_t>(), sc.n_triangles,
                           ctx->d_blob + sc.off_triattr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, "k_triangle_materials");
    }
    ctx->tri_materials = material != nullptr && sc.n_triangles != 0;
    // what the frame shows changed, and with it the set of emissive triangles; the recorded block costs are another picture's
    // (as after trc_upload_scene)
    trc_scene_changed(ctx, kSceneMaterials);
    return TRC_OK;
}

trc_status trc_resize(trc_ctx* ctx, uint32_t width, uint32_t height) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || width == 0 || height == 0 || width > 65535u * 8u || height > 65535u * 8u) return TRC_ERR_INVALID_ARG;
    // pixel indices are 32-bit in the seed / tonemap / strip / SPPM kernels
    if ((uint64_t)width * height >= (1ull << 32)) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_resize: 2^32 pixels or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));
    trc_release_frame(ctx);
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_rng, n * 16));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_accum, n * 16));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_rng, 0, n * 16, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_accum, 0, n * 16, ctx->stream));
    ctx->width = width; ctx->height = height;
    return TRC_OK;
}

trc_status trc_seed(trc_ctx* ctx, uint64_t seed) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_rng) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_seed before trc_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n = ctx->width * ctx->height;
    trc_sppm_order_after_camera(ctx);
    hipLaunchKernelGGL(k_seed, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_rng, n, seed);
    HIP_TRY(ctx, hipGetLastError());
    return TRC_OK;
}

static trc_status copy_frame(trc_ctx* ctx, void* dev, void* host, bool to_device) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !host) return TRC_ERR_INVALID_ARG;
    if (!dev) return trc_fail(ctx, TRC_ERR_NO_FRAME, "frame buffers not allocated (trc_resize)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->width * ctx->height * 16;
    trc_sppm_order_after_camera(ctx);
    TRC_TRY(to_device ? trc_copy_to_device(ctx, dev, host, bytes, ctx->stream) : trc_copy_to_host(ctx, host, dev, bytes, ctx->stream));
    collect_events(ctx);
    return TRC_OK;
}
trc_status trc_upload_rng(trc_ctx* ctx, const uint32_t* rgba) { return copy_frame(ctx, ctx ? ctx->d_rng : nullptr, (void*)rgba, true); }
trc_status trc_download_rng(trc_ctx* ctx, uint32_t* rgba) { return copy_frame(ctx, ctx ? ctx->d_rng : nullptr, rgba, false); }
trc_status trc_upload_accum(trc_ctx* ctx, const float* rgba) { return copy_frame(ctx, ctx ? ctx->d_accum : nullptr, (void*)rgba, true); }
trc_status trc_download_accum(trc_ctx* ctx, float* rgba) { return copy_frame(ctx, ctx ? ctx->d_accum : nullptr, rgba, false); }

trc_status trc_clear_accum(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_clear_accum before trc_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_accum, 0, (size_t)ctx->width * ctx->height * 16, ctx->stream));
    return TRC_OK;
}

trc_status trc_tonemap(trc_ctx* ctx, uint8_t* rgba8, float* exposure_out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !rgba8) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_tonemap before trc_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_tonemap_plane(ctx, ctx->d_accum, rgba8, exposure_out);
}
}  // extern "C"

trc_status trc_tonemap_plane(trc_ctx* ctx, const float* plane, uint8_t* rgba8, float* exposure_out) {
    const uint32_t n = ctx->width * ctx->height;
    DevBuf d_sums, d_out;
    TRC_TRY(d_sums.alloc(ctx, 3 * sizeof(unsigned long long), "tonemap"));
    TRC_TRY(d_out.alloc(ctx, (size_t)n * 4, "tonemap"));
    unsigned long long sums[3];
    if (hipMemsetAsync(d_sums.p, 0, sizeof sums, ctx->stream) != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, "tonemap memset");
    hipLaunchKernelGGL(k_tonemap_sum, dim3(std::min<uint32_t>((n + 255) / 256, 2048u)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float4*>(plane), n, d_sums.as<unsigned long long>());
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "tonemap sums", {{sums, d_sums.p, sizeof sums}}));
    // same binary32 / binary64 steps as oracle/oracle.cpp orc_tonemap (exp through trc_detmath.h)
    float mean[3];
    for (int c = 0; c < 3; ++c) mean[c] = (float)((double)sums[c] / 65536.0 / (double)n);
    const float luma = (mean[0] * 0.2126f + mean[1] * 0.7152f) + mean[2] * 0.0722f;
    float mapped = 1 - dm_expf(-1.0f * luma);
    mapped = std::fmin(std::fmax(mapped, 0.0f), 0.9999f);
    const float expose = 1.0f - mapped;
    if (exposure_out) *exposure_out = expose;
    hipLaunchKernelGGL(k_tonemap, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(plane),
                       ctx->width, ctx->height, expose, d_out.as<uchar4>());
    if (hipGetLastError() != hipSuccess || trc_copy_to_host(ctx, rgba8, d_out.p, (size_t)n * 4, ctx->stream) != TRC_OK) return trc_fail(ctx, TRC_ERR_HIP, "tonemap kernel");
    return TRC_OK;
}

extern "C" {
trc_status trc_synchronize(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));
    collect_events(ctx);
    return TRC_OK;
}

trc_status trc_trace_rays(trc_ctx* ctx, const trc_ray* rays, size_t n, trc_hit* out, int any_hit) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || (n && (!rays || !out))) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_trace_rays before trc_upload_scene");
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "too many rays in one call");
    if (any_hit & ~(TRC_TRACE_ANY_HIT | TRC_TRACE_PRODUCTION)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_trace_rays: unknown mode bits");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d_rays, d_hits;
    TRC_TRY(d_rays.alloc(ctx, n * sizeof(trc_ray), "rays"));
    TRC_TRY(d_hits.alloc(ctx, n * sizeof(trc_hit), "hits"));
    if (trc_copy_to_device(ctx, d_rays.p, rays, n * sizeof(trc_ray), ctx->stream) != TRC_OK) return trc_fail(ctx, TRC_ERR_HIP, "H2D rays");
    KTrace kp{};
    kp.ks = ctx->ks; kp.rays = d_rays.as<trc_ray>(); kp.hits = d_hits.as<trc_hit>(); kp.n = (uint32_t)n;
    const size_t lds = trc_dyn_lds_bytes(ctx, true);
    dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    const bool any = (any_hit & TRC_TRACE_ANY_HIT) != 0, prod = (any_hit & TRC_TRACE_PRODUCTION) != 0;
#define TRC_LAUNCH_TRACE(L, A, S) hipLaunchKernelGGL((k_trace<L, A, S>), grid, block, lds, ctx->stream, kp)
    if (ctx->lds_scene) {
        if (prod) { if (any) TRC_LAUNCH_TRACE(true, true, false); else TRC_LAUNCH_TRACE(true, false, false); }
        else      { if (any) TRC_LAUNCH_TRACE(true, true, true);  else TRC_LAUNCH_TRACE(true, false, true); }
    } else {
        if (prod) { if (any) TRC_LAUNCH_TRACE(false, true, false); else TRC_LAUNCH_TRACE(false, false, false); }
        else      { if (any) TRC_LAUNCH_TRACE(false, true, true);  else TRC_LAUNCH_TRACE(false, false, true); }
    }
#undef TRC_LAUNCH_TRACE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("k_trace launch: ") + hipGetErrorString(e));
    if (trc_copy_to_host(ctx, out, d_hits.p, n * sizeof(trc_hit), ctx->stream) != TRC_OK) return trc_fail(ctx, TRC_ERR_HIP, "D2H hits");
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("k_trace: ") + hipGetErrorString(e));
    return TRC_OK;
}

trc_status trc_get_stats(trc_ctx* ctx, trc_stats* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long h[kStatCount];
    TRC_TRY(trc_read_stats_sum(ctx, h, kStatCount));
    collect_events(ctx);
    std::memset(out, 0, sizeof *out);
    out->paths = h[kStatPaths]; out->rays = h[kStatRays]; out->shaded = h[kStatShaded];
    out->n_descend = h[kStatDescend]; out->n_return = h[kStatReturn];
    out->n_leaf_sphere = h[kStatLeafSphere]; out->n_leaf_square = h[kStatLeafSquare];
    out->n_leaf_cube = h[kStatLeafCube]; out->n_leaf_triangle = h[kStatLeafTriangle];
    out->n_hit_triangle = h[kStatHitTriangle]; out->n_hit_cube = h[kStatHitCube];
    out->launches = ctx->launches;
    out->kernel_ms = ctx->kernel_ms;
    out->schedule_ms = ctx->schedule_ms;
    return TRC_OK;
}

trc_status trc_reset_stats(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    collect_events(ctx);
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, sizeof(unsigned long long) * kStatRows * kStatRowStride, ctx->stream));
    ctx->launches = 0;
    ctx->kernel_ms = 0.0;
    ctx->schedule_ms = 0.0;
    return TRC_OK;
}

trc_status trc_device_info(trc_ctx* ctx, char* name, size_t name_len, int* cu_count, size_t* hbm_bytes) {
    if (!ctx) return TRC_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
    if (name && name_len) { std::snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName); }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return TRC_OK;
}

trc_status trc_device_pci_bus_id(trc_ctx* ctx, char* out, size_t out_len) {
    if (!ctx || !out || out_len < 16) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipDeviceGetPCIBusId(out, (int)out_len, ctx->device));
    return TRC_OK;
}

trc_status trc_debug_set(trc_ctx* ctx, const char* knob, int value) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !knob) return TRC_ERR_INVALID_ARG;
    const KnobEntry* entry = std::find_if(std::begin(kKnobs), std::end(kKnobs), [&](const KnobEntry& k) { return std::strcmp(k.name, knob) == 0; });
    if (entry == std::end(kKnobs)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_debug_set: unknown knob ") + knob);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));       // a launch in flight keeps the plan it was made with
    ctx->knobs.*entry->slot = value < 0 ? 0 : value;
    trc_forget_costs(ctx);                                 // block costs recorded under another launch geometry say nothing
    ctx->plan_streak = 0;
    return TRC_OK;
}

}  // extern "C"
