// trc_refit.hip -- the tree refitted in place around vertices that moved: trc_update_vertices, which receives them, and the tail that
// trc_deform.hip's calls, which compute them on the device, run behind their own kernel (trc_refit.hpp); the family's state and its
// lifetime (trc_ctx.hpp: RefitState), trc_download_vertices and the two debug getters.
//
// The topology stays: every fat node (dev_scene.hpp) keeps its tags, every record of a device-built tree its links.  What changes
// is 24 bytes per child slot: a triangle leaf's box is BVH::buildNode of its three current vertices (dev_trileaf.hpp: the arithmetic
// of the upload's k_triangle_leaves restated as a function), an interior child's box the union of that child's two slots, the boxes of the analytic primitives stay.
//
//   k_refit_triangles   the 48 B position and 64 B attribute record of every triangle that names a changed vertex; dword 15 of the
//                       attribute record (the material, trc_upload_triangle_materials) is read back and kept
//   k_refit_level       one launch per depth of the tree, deepest first.  The fat nodes are numbered by depth (build_blob's BFS,
//                       k_lbvh_emit's rank), so a depth is a RANGE of the array and a launch touches that range only; launch
//                       boundaries are the only synchronisation (trc_lbvh.hip k_lbvh_refit_pass says why)
//   k_refit_climb       the same in one launch (knob refit_single): the threads of the nodes without an interior child start, the
//                       second arrival at a node with two of them goes on; agent-scope release before the counter, acquire after
//
// A union keeps the RIGHT child's bound when the two compare equal (-0 against +0): minss / maxss of box_union(left, right), what
// the host builder and the device SAH build leave in a record.  The maps (parent of every fat node, its record in d_bvh_ref, the
// first node of every depth) are made by the first call of a scene that refits and freed with its blob, or when its tree is rebuilt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "dev_trileaf.hpp"
#include "trc_refit.hpp"

namespace {

constexpr uint32_t kRefitMaxLevels = TRC_MAX_BVH_DEPTH + 1;     // interior nodes have depth 0 .. TRC_MAX_BVH_DEPTH - 1
constexpr uint32_t kRefitBad = kRefitMaxLevels;                 // word of the level table: the numbering is not by depth
constexpr uint32_t kRefitRootWords = 12;                        // Maps::d_root: the box in 0..5, 6 and 7 zeroed by the root's store, the counter in kPoseCountWord

__device__ __forceinline__ float keep_right_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float keep_right_max(float a, float b) { return a > b ? a : b; }

// ---- maps, once per scene
__global__ void __launch_bounds__(256) k_refit_parents(const uint4* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ parent) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    if (k == 0) parent[0] = 0;
    const uint4 q3 = nodes[4 * (size_t)k + 3];
    const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if ((tag[s] >> kTagIndexBits) == kTagInterior) {
            const uint32_t c = tag[s] & kTagIndexMask;
            if (c > 0 && c < n_nodes) parent[c] = k;
        }
}
// level[d] = first node of depth d; level[kRefitBad] != 0: a node is numbered before a shallower one, or deeper than the limit
__global__ void __launch_bounds__(256) k_refit_levels(const uint32_t* __restrict__ parent, uint32_t n_nodes, uint32_t* __restrict__ level) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    uint32_t d = 0, dp = 0;
    for (uint32_t j = k; j != 0u && d < kRefitMaxLevels; j = parent[j]) ++d;
    if (k > 0) for (uint32_t j = k - 1; j != 0u && dp < kRefitMaxLevels; j = parent[j]) ++dp;
    if (d >= kRefitMaxLevels || dp > d) { level[kRefitBad] = 1u; return; }
    if (k == 0 || dp != d) level[d] = k;
}
// refnode[child] = the child's record in the reference-layout array; one launch per depth, root first
__global__ void __launch_bounds__(256) k_refit_refnodes(const uint4* __restrict__ nodes, const trc_BVH* __restrict__ ref, uint32_t first, uint32_t end,
                                                        uint32_t n_nodes, uint32_t* __restrict__ refnode) {
    const uint32_t k = first + blockIdx.x * 256u + threadIdx.x;
    if (k >= end) return;
    const uint32_t r = k == 0 ? 0u : refnode[k];
    const uint4 q3 = nodes[4 * (size_t)k + 3];
    const uint4 hd = *reinterpret_cast<const uint4*>(&ref[r]);      // parent, left, right, axis
    const uint32_t tag[2] = {q3.z, q3.w}, rec[2] = {hd.y, hd.z};
    if (k == 0) refnode[0] = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if ((tag[s] >> kTagIndexBits) == kTagInterior) {
            const uint32_t c = tag[s] & kTagIndexMask;
            if (c > 0 && c < n_nodes) refnode[c] = rec[s];
        }
}
// primslot[section of the type + index] = 2 * k + slot for every slot of fat node k that is the leaf of a sphere, a square or a cube
// (trc_update_primitives); first[type]: where the type's section begins, n[type]: its length.  The array starts out as kTagNone
struct PrimSections { uint32_t first[3], n[3]; };
__global__ void __launch_bounds__(256) k_refit_primslots(const uint4* __restrict__ nodes, uint32_t n_nodes, PrimSections sec, uint32_t* __restrict__ primslot) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    const uint4 q3 = nodes[4 * (size_t)k + 3];
    const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t type = tag[s] >> kTagIndexBits, index = tag[s] & kTagIndexMask;
        if (type < kTagTriangle && index < sec.n[type]) primslot[sec.first[type] + index] = 2u * k + s;
    }
}

// ---- the update
struct KRefit {
    uint4* nodes; uint32_t n_nodes;
    const trc_TriangleVertex* verts; const uint32_t* idx; uint32_t n_tri;
    trc_BVH* ref; const uint32_t* refnode; uint32_t n_ref;      // null / 0: a host tree
    float* root;
};

__global__ void __launch_bounds__(256) k_refit_triangles(const trc_TriangleVertex* __restrict__ verts, const uint32_t* __restrict__ idx, uint32_t n_tri,
                                                         uint32_t first, uint32_t count, float4* __restrict__ tripos, float4* __restrict__ triattr) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    const uint32_t i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
    if (i0 - first >= count && i1 - first >= count && i2 - first >= count) return;      // none of its vertices changed
    const trc_TriangleVertex a = verts[i0], b = verts[i1], c = verts[i2];
    const float material = triattr[4 * (size_t)t + 3].w;                                 // dword 15 stays
    tripos[3 * (size_t)t] = make_float4(a.v[0], a.v[1], a.v[2], 0.0f);
    tripos[3 * (size_t)t + 1] = make_float4(b.v[0], b.v[1], b.v[2], 0.0f);
    tripos[3 * (size_t)t + 2] = make_float4(c.v[0], c.v[1], c.v[2], 0.0f);
    triattr[4 * (size_t)t] = make_float4(a.n[0], a.n[1], a.n[2], b.n[0]);
    triattr[4 * (size_t)t + 1] = make_float4(b.n[1], b.n[2], c.n[0], c.n[1]);
    triattr[4 * (size_t)t + 2] = make_float4(c.n[2], a.uv[0], a.uv[1], b.uv[0]);
    triattr[4 * (size_t)t + 3] = make_float4(b.uv[1], c.uv[0], c.uv[1], material);
}

// both child boxes of fat node k from what lies below it; every access to a fat node is 16 bytes wide
__device__ __forceinline__ void refit_node(const KRefit& p, uint32_t k) {
    uint4* nd = p.nodes + 4 * (size_t)k;
    const uint4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
    float box[2][6] = {{__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)},
                       {__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z), __uint_as_float(q2.w)}};
    const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t type = tag[s] >> kTagIndexBits, index = tag[s] & kTagIndexMask;
        if (type == kTagInterior && index < p.n_nodes) {
            const uint4* ch = p.nodes + 4 * (size_t)index;
            const uint4 c0 = ch[0], c1 = ch[1], c2 = ch[2];
            box[s][0] = keep_right_min(__uint_as_float(c0.x), __uint_as_float(c1.z)); box[s][1] = keep_right_min(__uint_as_float(c0.y), __uint_as_float(c1.w));
            box[s][2] = keep_right_min(__uint_as_float(c0.z), __uint_as_float(c2.x)); box[s][3] = keep_right_max(__uint_as_float(c0.w), __uint_as_float(c2.y));
            box[s][4] = keep_right_max(__uint_as_float(c1.x), __uint_as_float(c2.z)); box[s][5] = keep_right_max(__uint_as_float(c1.y), __uint_as_float(c2.w));
        } else if (type == kTagTriangle && index < p.n_tri) {
            const trc_TriangleVertex a = p.verts[p.idx[3 * index]], b = p.verts[p.idx[3 * index + 1]], c = p.verts[p.idx[3 * index + 2]];
            triangle_leaf_box(a, b, c, &box[s][0], &box[s][3]);
        }
    }
    nd[0] = make_uint4(__float_as_uint(box[0][0]), __float_as_uint(box[0][1]), __float_as_uint(box[0][2]), __float_as_uint(box[0][3]));
    nd[1] = make_uint4(__float_as_uint(box[0][4]), __float_as_uint(box[0][5]), __float_as_uint(box[1][0]), __float_as_uint(box[1][1]));
    nd[2] = make_uint4(__float_as_uint(box[1][2]), __float_as_uint(box[1][3]), __float_as_uint(box[1][4]), __float_as_uint(box[1][5]));
    float root[6];
    if (k == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { root[a] = keep_right_min(box[0][a], box[1][a]); root[3 + a] = keep_right_max(box[0][3 + a], box[1][3 + a]); }
        reinterpret_cast<float4*>(p.root)[0] = make_float4(root[0], root[1], root[2], root[3]);
        reinterpret_cast<float4*>(p.root)[1] = make_float4(root[4], root[5], 0.0f, 0.0f);
    }
    if (p.ref) {              // the same boxes in the records of trc_download_bvh (the padding lane of a rewritten corner is 0)
        const uint32_t r = p.refnode[k];
        if (r >= p.n_ref) return;
        const uint4 hd = *reinterpret_cast<const uint4*>(&p.ref[r]);
        const uint32_t rec[2] = {hd.y, hd.z};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (rec[s] >= p.n_ref) continue;
            float4* bb = reinterpret_cast<float4*>(&p.ref[rec[s]].bBOX);
            bb[0] = make_float4(box[s][0], box[s][1], box[s][2], 0.0f);
            bb[1] = make_float4(box[s][3], box[s][4], box[s][5], 0.0f);
        }
        if (k == 0) {
            float4* bb = reinterpret_cast<float4*>(&p.ref[0].bBOX);
            bb[0] = make_float4(root[0], root[1], root[2], 0.0f);
            bb[1] = make_float4(root[3], root[4], root[5], 0.0f);
        }
    }
}

__global__ void __launch_bounds__(256) k_refit_level(KRefit p, uint32_t first, uint32_t end) {
    const uint32_t k = first + blockIdx.x * 256u + threadIdx.x;
    if (k < end) refit_node(p, k);
}

__device__ __forceinline__ uint32_t interior_children(const uint4& q3) {
    return ((q3.z >> kTagIndexBits) == kTagInterior ? 1u : 0u) + ((q3.w >> kTagIndexBits) == kTagInterior ? 1u : 0u);
}
// one launch: a thread starts at every node without an interior child and climbs.  At a node with two interior children the first
// arrival ends, the second sees both (release before the counter, acquire after it, agent scope: the children may have been
// written under another L2) and puts the counter back to zero for the next update
__global__ void __launch_bounds__(256) k_refit_climb(KRefit p, const uint32_t* __restrict__ parent, uint32_t* __restrict__ arrive) {
    uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.n_nodes || interior_children(p.nodes[4 * (size_t)k + 3]) != 0u) return;
    for (uint32_t step = 0; step <= kRefitMaxLevels; ++step) {
        refit_node(p, k);
        if (k == 0) return;
        const uint32_t up = parent[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (interior_children(p.nodes[4 * (size_t)up + 3]) == 2u) {
            if (__hip_atomic_fetch_add(&arrive[up], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
            __hip_atomic_store(&arrive[up], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        k = up;
    }
}

// The maps of the uploaded tree (RefitState::Maps), behind whatever the stream still holds.  They reach the context once all of them
// exist: a failure leaves it as it was.  The overflow counter lives in the root buffer and starts again at zero with it
trc_status refit_make_maps(trc_ctx* ctx) {
    RefitState::Maps& m = ctx->refit.maps;
    if (!m.levels.empty()) return TRC_OK;
    const DScene& sc = ctx->ks.sc;
    const uint32_t n = sc.n_nodes;
    const uint4* nodes = reinterpret_cast<const uint4*>(ctx->d_blob + sc.off_nodes);
    const dim3 grid((n + 255) / 256), b256(256);
    hipStream_t st = ctx->stream;
    DevBuf parent, arrive, root, level_buf, refnode, primslot;
    const PrimSections sec{{0u, sc.n_spheres, sc.n_spheres + sc.n_squares}, {sc.n_spheres, sc.n_squares, sc.n_cubes}};
    const size_t n_prims = (size_t)sc.n_spheres + sc.n_squares + sc.n_cubes;      // (their records fit 40 KB: no wrap)
    uint32_t level[kRefitMaxLevels + 1];
    TRC_TRY(parent.alloc(ctx, (size_t)n * 4, "trc_update_vertices: parent map"));
    TRC_TRY(arrive.alloc(ctx, (size_t)n * 4, "trc_update_vertices: arrival counters"));
    TRC_TRY(root.alloc(ctx, kRefitRootWords * sizeof(float), "trc_update_vertices: root box"));
    TRC_TRY(level_buf.alloc(ctx, sizeof level, "trc_update_vertices: level table"));
    if (ctx->d_bvh_ref) TRC_TRY(refnode.alloc(ctx, (size_t)n * 4, "trc_update_vertices: record map"));
    if (n_prims) {
        TRC_TRY(primslot.alloc(ctx, n_prims * 4, "trc_update_primitives: leaf map"));
        HIP_TRY(ctx, hipMemsetAsync(primslot.p, 0xFF, n_prims * 4, st));
    }
    HIP_TRY(ctx, hipMemsetAsync(parent.p, 0, (size_t)n * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(arrive.p, 0, (size_t)n * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(level_buf.p, 0, sizeof level, st));
    HIP_TRY(ctx, hipMemsetAsync(root.p, 0, kRefitRootWords * sizeof(float), st));
    hipLaunchKernelGGL(k_refit_parents, grid, b256, 0, st, nodes, n, parent.as<uint32_t>());
    hipLaunchKernelGGL(k_refit_levels, grid, b256, 0, st, parent.as<uint32_t>(), n, level_buf.as<uint32_t>());
    if (n_prims) hipLaunchKernelGGL(k_refit_primslots, grid, b256, 0, st, nodes, n, sec, primslot.as<uint32_t>());
    HIP_TRY(ctx, hipGetLastError());
    TRC_TRY(trc_read_to_host(ctx, st, "trc_update_vertices: level table", {{level, level_buf.p, sizeof level}}));
    if (level[kRefitBad]) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_update_vertices: the fat nodes are not numbered by depth");
    std::vector<uint32_t> levels{0u};
    for (uint32_t d = 1; d < kRefitMaxLevels && level[d] != 0u; ++d) levels.push_back(level[d]);
    levels.push_back(n);
    if (ctx->d_bvh_ref) {
        for (size_t d = 0; d + 1 < levels.size(); ++d)
            hipLaunchKernelGGL(k_refit_refnodes, dim3((levels[d + 1] - levels[d] + 255) / 256), b256, 0, st, nodes, ctx->d_bvh_ref, levels[d], levels[d + 1],
                               n, refnode.as<uint32_t>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    m.d_parent = static_cast<uint32_t*>(parent.release()); m.d_arrive = static_cast<uint32_t*>(arrive.release());
    m.d_root = static_cast<float*>(root.release()); m.d_refnode = static_cast<uint32_t*>(refnode.release());
    m.d_primslot = static_cast<uint32_t*>(primslot.release());
    m.count_seen = 0; m.levels = std::move(levels);
    return TRC_OK;
}

}  // namespace

trc_status trc_refit_events(trc_ctx* ctx, const char* who) {
    for (hipEvent_t& e : ctx->refit.ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return trc_fail(ctx, TRC_ERR_HIP, std::string(who) + ": hipEventCreate"); }
    return TRC_OK;
}
trc_status trc_refit_begin(trc_ctx* ctx, const char* who) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(trc_readback_alloc(ctx));
    TRC_TRY(refit_make_maps(ctx));
    return trc_refit_events(ctx, who);
}

// neither a pose, a skin nor a morph has written d_verts yet, so they are the caller's values
trc_status trc_rest_ensure(trc_ctx* ctx, const char* what) {
    if (ctx->refit.d_rest) return TRC_OK;
    const size_t bytes = (size_t)ctx->n_vertex * sizeof(trc_TriangleVertex);
    DevBuf rest;
    TRC_TRY(rest.alloc(ctx, bytes, what));
    HIP_TRY(ctx, hipMemcpyAsync(rest.p, ctx->d_verts, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->refit.d_rest = static_cast<trc_TriangleVertex*>(rest.release());
    return TRC_OK;
}

trc_status trc_refit_close(trc_ctx* ctx) {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->refit.ev[1], ctx->stream));
    ctx->refit.timed = true;
    return TRC_OK;
}
void trc_refit_launch_triangles(trc_ctx* ctx, uint32_t first, uint32_t count) {
    const DScene& sc = ctx->ks.sc;
    hipLaunchKernelGGL(k_refit_triangles, dim3((sc.n_triangles + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_verts, ctx->d_idx, sc.n_triangles, first, count,
                       reinterpret_cast<float4*>(ctx->d_blob + sc.off_tripos), reinterpret_cast<float4*>(ctx->d_blob + sc.off_triattr));
}

trc_status trc_refit_tail(trc_ctx* ctx, uint32_t first, uint32_t count, bool counted) {
    const DScene& sc = ctx->ks.sc;
    RefitState& r = ctx->refit;
    hipStream_t st = ctx->stream;
    KRefit p{};
    p.nodes = reinterpret_cast<uint4*>(ctx->d_blob + sc.off_nodes); p.n_nodes = sc.n_nodes;
    p.verts = ctx->d_verts; p.idx = ctx->d_idx; p.n_tri = sc.n_triangles;
    p.ref = ctx->d_bvh_ref; p.refnode = r.maps.d_refnode; p.n_ref = ctx->d_bvh_ref ? ctx->n_bvh_ref : 0u; p.root = r.maps.d_root;
    if (count != 0 && sc.n_triangles != 0) trc_refit_launch_triangles(ctx, first, count);      // (trc_update_primitives: no vertex changed)
    if (ctx->knobs.refit_single) {
        hipLaunchKernelGGL(k_refit_climb, dim3((sc.n_nodes + 255) / 256), dim3(256), 0, st, p, r.maps.d_parent, r.maps.d_arrive);
    } else {
        const std::vector<uint32_t>& lv = r.maps.levels;
        for (size_t d = lv.size() - 1; d-- > 0;)
            hipLaunchKernelGGL(k_refit_level, dim3((lv[d + 1] - lv[d] + 255) / 256), dim3(256), 0, st, p, lv[d], lv[d + 1]);
    }
    TRC_TRY(trc_refit_close(ctx));
    // the root box is a kernel PARAMETER of every launch (KScene): it is copied back behind the refit and read by the next entry
    // point that is entered (trc_refit_settle, at the top of trc_flush and render_pass), so this call does not wait for the device
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_readback, r.maps.d_root, (counted ? kPoseCountWord + 1 : 6) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(r.ev[2], st));
    r.pending = true; r.posed = counted;
    // the picture changed a little, as under a camera that moves a little (trc_set_camera): the recorded block costs stay, and the
    // next ordered launch is one pass on the last launch's raw durations
    if (ctx->cost_valid) { ctx->plan_streak = 0; ctx->cost_fresh_next = true; }
    return TRC_OK;
}

trc_status trc_refit_read_time(trc_ctx* ctx) {
    RefitState& r = ctx->refit;
    if (!r.timed) return TRC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(r.ev[1]));
    (void)hipEventElapsedTime(&r.ms, r.ev[0], r.ev[1]);
    r.timed = false;
    return TRC_OK;
}

// the root box of the last refit into ks (a kernel PARAMETER of every launch), its overflow count and its time; waits for them
trc_status trc_refit_settle_pending(trc_ctx* ctx) {
    RefitState& r = ctx->refit;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(r.ev[2]));      // on an error the box stays pending: no launch runs on the old one
    std::memcpy(ctx->ks.root_box, ctx->h_readback, 6 * sizeof(float));
    r.pending = false;
    if (r.posed) {
        r.overflows = ctx->h_readback[kPoseCountWord] - r.maps.count_seen;      // (modulo 2^32, as the counter itself)
        r.maps.count_seen = ctx->h_readback[kPoseCountWord];
        r.posed = false;
    }
    return trc_refit_read_time(ctx);
}

// freed with the scene and by trc_rebuild_tree; a pending read-back has been settled by the caller's trc_flush
void trc_refit_free_maps(trc_ctx* ctx) {
    RefitState::Maps& m = ctx->refit.maps;
    for (void* q : {(void*)m.d_parent, (void*)m.d_arrive, (void*)m.d_root, (void*)m.d_refnode, (void*)m.d_primslot}) (void)hipFree(q);
    m = RefitState::Maps{};
}

void trc_refit_free(trc_ctx* ctx) {
    RefitState& r = ctx->refit;
    for (hipEvent_t e : r.ev) if (e) (void)hipEventDestroy(e);
    trc_refit_free_maps(ctx);
    for (void* q : {(void*)r.d_adj_offsets, (void*)r.d_adj_corners, (void*)r.d_rest, (void*)r.d_pose_table, (void*)r.skin.d_influences, (void*)r.d_palette,
                    (void*)r.morph.d_deltas, r.d_morph_active, r.d_prim_stage, (void*)ctx->d_verts, (void*)ctx->d_idx}) (void)hipFree(q);
    const float ms = r.ms; r = RefitState{}; r.ms = ms;      // (trc_debug_refit_ms goes on reporting the last call's time)
    ctx->d_verts = nullptr; ctx->d_idx = nullptr; ctx->n_vertex = 0;
}

extern "C" {

trc_status trc_update_vertices(trc_ctx* ctx, const trc_TriangleVertex* vertices, uint32_t first, uint32_t count) {
    TRC_TRY(trc_enter_scene(ctx, "trc_update_vertices"));
    if (count == 0) return TRC_OK;
    if (!vertices) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: vertices == NULL with count > 0");
    if (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: the scene has no triangles");
    if (first > ctx->n_vertex || count > ctx->n_vertex - first) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: first + count > n_vertex");
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(vertices[i].v[k]) <= 1e37f)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: position not finite or beyond 1e37");
    TRC_TRY(trc_refit_begin(ctx, "trc_update_vertices"));
    hipStream_t st = ctx->stream;
    // from here on the scene changed: what was derived from the old geometry goes -- said in front of the copy, which writes the vertices
    // (trc_denoise_track_motion: the snapshot is of the vertices as they still stand)
    trc_scene_changed(ctx, kSceneVerticesMoved);     // (TRC_FLAG_MESH_LIGHTS: the areas changed)
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_verts + first, vertices, (size_t)count * sizeof(trc_TriangleVertex), st));
    // a scene that has been posed keeps rest vertices: these are the caller's last values for the range
    if (ctx->refit.d_rest) HIP_TRY(ctx, hipMemcpyAsync(ctx->refit.d_rest + first, ctx->d_verts + first, (size_t)count * sizeof(trc_TriangleVertex), hipMemcpyDeviceToDevice, st));
    TRC_TRY(trc_refit_open(ctx));
    return trc_refit_tail(ctx, first, count, false);
}

trc_status trc_download_vertices(trc_ctx* ctx, trc_TriangleVertex* out, uint32_t first, uint32_t count) {
    TRC_TRY(trc_enter_scene(ctx, "trc_download_vertices"));
    if (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_vertices: the scene has no triangles");
    if (first > ctx->n_vertex || count > ctx->n_vertex - first) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_vertices: first + count > n_vertex");
    if (count == 0) return TRC_OK;
    if (!out) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_vertices: out == NULL with count > 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(trc_copy_to_host(ctx, out, ctx->d_verts + first, (size_t)count * sizeof(trc_TriangleVertex), ctx->stream));
    return TRC_OK;
}

trc_status trc_debug_pose_overflows(trc_ctx* ctx, uint32_t* n) {
    if (!ctx || !n) return TRC_ERR_INVALID_ARG;
    TRC_TRY(trc_flush(ctx));
    *n = ctx->refit.overflows;
    return TRC_OK;
}

trc_status trc_debug_refit_ms(trc_ctx* ctx, float* ms) {
    if (!ctx || !ms) return TRC_ERR_INVALID_ARG;
    TRC_TRY(trc_flush(ctx));
    TRC_TRY(trc_refit_read_time(ctx));      // a trc_recompute_normals reads nothing back: its events are waited for here
    *ms = ctx->refit.ms;
    return TRC_OK;
}

}  // extern "C"
