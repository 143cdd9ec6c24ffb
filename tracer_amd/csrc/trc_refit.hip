// trc_refit.hip -- trc_update_vertices: new vertices for the uploaded mesh, and the tree refitted in place.
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
// first node of every depth) are made by the first update of a scene and freed with its blob.
//
// trc_pose_vertices computes the new vertices on the device instead of receiving them, and then runs the same tail (refit_run):
//   k_pose_vertices     ONE launch for all ranges of a call: thread g of the concatenated ranges finds its range in the sorted pose
//                       table by bisection (the table's _pad[0] is the range's first g), reads the vertex from the rest copy d_rest
//                       and writes it, posed, to d_verts; two 16 B accesses per vertex each way
//
// trc_skin_vertices does the same for vertices that bend: trc_skin_bind has left four (bone, weight) influences per bound vertex on
// the device, the call brings the frame's bone palette, and in front of the same tail runs one of
//   k_skin_vertices_lds the palette's read columns staged in LDS once per workgroup, which then takes 256 bound vertices at a time
//   k_skin_vertices     the columns gathered from memory: palettes beyond kSkinLdsBones (skin_check.hpp), and knob skin_no_lds
// Both blend the four bones' matrices entry by entry and put the REST vertex under the blend with k_pose_vertices' expressions.
//
// trc_morph_vertices adds weighted deltas to the rest vertex: trc_morph_bind has left n_targets deltas per bound vertex on the device,
// target-major, the call brings the frame's weights, compacted by the host into the active list (morph_check.hpp), and in front of the
// same tail runs one of
//   k_morph_vertices       one thread per bound vertex: rest + the active targets' weighted deltas, in the list's order
//   k_morph_skin_vertices  with a palette: one thread per vertex of the hull of the morph and the skin binding; the morph where the
//                          vertex is morph-bound, then the skin's arithmetic on those values where it is skin-bound (columns gathered)
//
// trc_recompute_normals moves nothing: it replaces the normals of a vertex range by area-weighted smooth normals of the mesh as it
// stands.  The first call of a scene sorts the corners of the index list by their vertex (k_adj_keys, trc_lbvh.hip's radix sort,
// k_adj_offsets: the adjacency, kept with the scene); every call then runs
//   k_vertex_normals       one thread per vertex of the range: the cross products of its corners' triangles, read from the 48 B position
//                          records, summed in corner order, put on the side of the normal it holds, normalised
// and k_refit_triangles behind it.  No box changes, so nothing of the refit proper runs
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "dev_trileaf.hpp"
#include "morph_check.hpp"
#include "normals_check.hpp"
#include "pose_ranges.hpp"
#include "skin_check.hpp"
#include "trc_ctx.hpp"

namespace {

constexpr uint32_t kRefitMaxLevels = TRC_MAX_BVH_DEPTH + 1;     // interior nodes have depth 0 .. TRC_MAX_BVH_DEPTH - 1
constexpr uint32_t kRefitBad = kRefitMaxLevels;                 // word of the level table: the numbering is not by depth
constexpr uint32_t kRefitRootWords = 12;                        // d_refit_root: the box in 0..5, 6 and 7 zeroed by the root's store, ...
constexpr uint32_t kPoseCountWord = 8;                          // ... and the running count of pose overflows (trc_ctx.hpp)

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

// ---- the pose: verts[v] = M * rest[v] for every vertex of every range, in the operation order of include/tracer_abi.h.
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
    const float4* m = reinterpret_cast<const float4*>(&table[lo].model_matrix);      // 4 columns, then the normal matrix's
    const float4 c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3], n0 = m[4], n1 = m[5], n2 = m[6];
    const float4 a = rest[2 * (size_t)v], b = rest[2 * (size_t)v + 1];              // x y z nx | ny nz u v
    const float x = ((c0.x * a.x + c1.x * a.y) + c2.x * a.z) + c3.x;
    const float y = ((c0.y * a.x + c1.y * a.y) + c2.y * a.z) + c3.y;
    const float z = ((c0.z * a.x + c1.z * a.y) + c2.z * a.z) + c3.z;
    const float nx = (n0.x * a.w + n1.x * b.x) + n2.x * b.y;
    const float ny = (n0.y * a.w + n1.y * b.x) + n2.y * b.y;
    const float nz = (n0.z * a.w + n1.z * b.x) + n2.z * b.y;
    verts[2 * (size_t)v] = make_float4(x, y, z, nx);
    verts[2 * (size_t)v + 1] = make_float4(ny, nz, b.z, b.w);
    if (!(fabsf(x) <= 1e37f) || !(fabsf(y) <= 1e37f) || !(fabsf(z) <= 1e37f))      // the caller's contract, broken: counted, never an index
        __hip_atomic_fetch_add(overflows, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    const float4 c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3], n0 = m[4], n1 = m[5], n2 = m[6];
    const float x = ((c0.x * a.x + c1.x * a.y) + c2.x * a.z) + c3.x;
    const float y = ((c0.y * a.x + c1.y * a.y) + c2.y * a.z) + c3.y;
    const float z = ((c0.z * a.x + c1.z * a.y) + c2.z * a.z) + c3.z;
    const float nx = (n0.x * a.w + n1.x * b.x) + n2.x * b.y;
    const float ny = (n0.y * a.w + n1.y * b.x) + n2.y * b.y;
    const float nz = (n0.z * a.w + n1.z * b.x) + n2.z * b.y;
    verts[2 * (size_t)v] = make_float4(x, y, z, nx);
    verts[2 * (size_t)v + 1] = make_float4(ny, nz, b.z, b.w);
    if (!(fabsf(x) <= 1e37f) || !(fabsf(y) <= 1e37f) || !(fabsf(z) <= 1e37f))      // the caller's contract, broken: counted, never an index
        __hip_atomic_fetch_add(overflows, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
struct KSkin {
    const float4* rest; float4* verts; uint32_t n_vertex;
    const uint4* influences; uint32_t first, count;     // influences: 2 x 16 B per bound vertex, the bones and then the weights
    const float4* palette; uint32_t n_bones;            // 8 columns per bone (trc_skin_bone)
    uint32_t* overflows;
};
// bound vertex i of the binding (the host refused a table or a palette that these tests would catch)
template <class Col>
__device__ __forceinline__ void skin_bound_vertex(const KSkin& p, uint32_t i, uint32_t n_bones, const Col& col) {
    const uint32_t v = p.first + i;
    if (v >= p.n_vertex) return;
    const uint4 bone = p.influences[2 * (size_t)i];
    const uint4 wb = p.influences[2 * (size_t)i + 1];
    if (bone.x >= n_bones || bone.y >= n_bones || bone.z >= n_bones || bone.w >= n_bones) return;
    const float4 w = make_float4(__uint_as_float(wb.x), __uint_as_float(wb.y), __uint_as_float(wb.z), __uint_as_float(wb.w));
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
    if (!(fabsf(a.x) <= 1e37f) || !(fabsf(a.y) <= 1e37f) || !(fabsf(a.z) <= 1e37f))      // the caller's contract, broken: counted, never an index
        __hip_atomic_fetch_add(overflows, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    const uint4 bone = s.influences[2 * (size_t)is];
    const uint4 wb = s.influences[2 * (size_t)is + 1];
    if (bone.x >= s.n_bones || bone.y >= s.n_bones || bone.z >= s.n_bones || bone.w >= s.n_bones) return;
    const float4 w = make_float4(__uint_as_float(wb.x), __uint_as_float(wb.y), __uint_as_float(wb.z), __uint_as_float(wb.w));
    const float4* palette = s.palette;
    skin_vertex(a, b, s.verts, v, bone, w, [palette](uint32_t bn, int c) { return palette[8 * (size_t)bn + c]; }, s.overflows);
}

// ---- the normals: the vertex -> corner adjacency of the index list, once per scene, and the gather behind it, in the operation
// order of include/tracer_abi.h.  Corner k of the index list belongs to triangle k / 3 and names vertex idx[k]
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

// The adjacency of the scene's index list (trc_ctx: d_adj_offsets, d_adj_corners), behind whatever the stream still holds.  The corners
// are sorted by their vertex with the tree builds' stable LSD radix sort over the bits n_vertex needs: stable, so every vertex's corners
// stay ascending, which is the order the definition sums in -- a count / scan / fill-by-atomics build would leave every list in the
// order the atomics happened to resolve and need a sort per list behind it.  Everything is allocated before anything runs:
// TRC_ERR_OOM leaves nothing behind.  Waits for the device once, because the temporaries go when it returns
trc_status normals_adjacency(trc_ctx* ctx) {
    if (ctx->d_adj_offsets) return TRC_OK;
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
    ctx->d_adj_offsets = static_cast<uint32_t*>(offsets.release());
    ctx->d_adj_corners = static_cast<uint32_t*>(corners.release());
    return TRC_OK;
}

// the maps themselves (refit_prepare frees what a failure leaves half made)
trc_status refit_make_maps(trc_ctx* ctx) {
    const DScene& sc = ctx->ks.sc;
    const uint32_t n = sc.n_nodes;
    const uint4* nodes = reinterpret_cast<const uint4*>(ctx->d_blob + sc.off_nodes);
    const dim3 grid((n + 255) / 256), b256(256);
    hipStream_t st = ctx->stream;
    DevBuf level_buf;
    uint32_t level[kRefitMaxLevels + 1];
#define REFIT_TRY(expr, what)                                                                                                  \
    do {                                                                                                                       \
        const hipError_t e_ = (expr);                                                                                          \
        if (e_ != hipSuccess)                                                                                                  \
            return trc_fail(ctx, e_ == hipErrorOutOfMemory ? TRC_ERR_OOM : TRC_ERR_HIP, std::string("trc_update_vertices: ") + what + ": " + hipGetErrorString(e_)); \
    } while (0)
    REFIT_TRY(hipMalloc((void**)&ctx->d_refit_parent, (size_t)n * 4), "parent map");
    REFIT_TRY(hipMalloc((void**)&ctx->d_refit_arrive, (size_t)n * 4), "arrival counters");
    REFIT_TRY(hipMalloc((void**)&ctx->d_refit_root, kRefitRootWords * sizeof(float)), "root box");
    ctx->pose_count_seen = 0;
    TRC_TRY(level_buf.alloc(ctx, sizeof level, "level table"));
    uint32_t* const d_level = level_buf.as<uint32_t>();
    if (ctx->d_bvh_ref) REFIT_TRY(hipMalloc((void**)&ctx->d_refit_refnode, (size_t)n * 4), "record map");
    REFIT_TRY(hipMemsetAsync(ctx->d_refit_parent, 0, (size_t)n * 4, st), "memset");
    REFIT_TRY(hipMemsetAsync(ctx->d_refit_arrive, 0, (size_t)n * 4, st), "memset");
    REFIT_TRY(hipMemsetAsync(d_level, 0, sizeof level, st), "memset");
    REFIT_TRY(hipMemsetAsync(ctx->d_refit_root, 0, kRefitRootWords * sizeof(float), st), "memset");
    hipLaunchKernelGGL(k_refit_parents, grid, b256, 0, st, nodes, n, ctx->d_refit_parent);
    hipLaunchKernelGGL(k_refit_levels, grid, b256, 0, st, ctx->d_refit_parent, n, d_level);
    REFIT_TRY(hipGetLastError(), "map kernels");
    TRC_TRY(trc_read_to_host(ctx, st, "trc_update_vertices: level table", {{level, d_level, sizeof level}}));
    if (level[kRefitBad]) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_update_vertices: the fat nodes are not numbered by depth");
    std::vector<uint32_t> levels{0u};
    for (uint32_t d = 1; d < kRefitMaxLevels && level[d] != 0u; ++d) levels.push_back(level[d]);
    levels.push_back(n);
    if (ctx->d_bvh_ref) {
        for (size_t d = 0; d + 1 < levels.size(); ++d)
            hipLaunchKernelGGL(k_refit_refnodes, dim3((levels[d + 1] - levels[d] + 255) / 256), b256, 0, st, nodes, ctx->d_bvh_ref, levels[d], levels[d + 1],
                               n, ctx->d_refit_refnode);
        REFIT_TRY(hipGetLastError(), "record map");
        REFIT_TRY(hipStreamSynchronize(st), "record map");
    }
#undef REFIT_TRY
    ctx->refit_levels = std::move(levels);
    return TRC_OK;
}

// maps of the uploaded scene (trc_ctx: d_refit_*, refit_levels), behind whatever the stream still holds; the only part of an update
// that waits for the device, once per scene
trc_status refit_prepare(trc_ctx* ctx) {
    if (!ctx->refit_levels.empty()) return TRC_OK;
    const trc_status rs = refit_make_maps(ctx);
    if (rs != TRC_OK) trc_refit_free_maps(ctx);
    return rs;
}

// What both entry points do before anything changes: the pinned read-back buffer, the maps, the events.  `who` names the caller
trc_status refit_begin(trc_ctx* ctx, const char* who) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(trc_readback_alloc(ctx));
    TRC_TRY(refit_prepare(ctx));
    for (hipEvent_t& e : ctx->refit_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return trc_fail(ctx, TRC_ERR_HIP, std::string(who) + ": hipEventCreate"); }
    return TRC_OK;
}

// The rest copy, made by the first pose or skin of a scene: neither has written d_verts yet, so they are the caller's values
trc_status rest_ensure(trc_ctx* ctx, const char* what) {
    if (ctx->d_rest) return TRC_OK;
    const size_t bytes = (size_t)ctx->n_vertex * sizeof(trc_TriangleVertex);
    DevBuf rest;
    TRC_TRY(rest.alloc(ctx, bytes, what));
    HIP_TRY(ctx, hipMemcpyAsync(rest.p, ctx->d_verts, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->d_rest = static_cast<trc_TriangleVertex*>(rest.release());
    return TRC_OK;
}

// ... and behind their vertices, on the context's stream: [the kernel in front,] the records of the triangles that name a vertex of
// [first, first + count), every box of the tree, the root box on its way back.  Where the range is a hull, a triangle of the hull that
// no vertex of the call touched gets the bits it had, and keeps its material.  RefitFront names the kernel in front:
//   kFrontNone   trc_update_vertices: the vertices came by copy
//   kFrontPose   trc_pose_vertices, whose sorted table of n_poses ranges (pose_total vertices in all) is in d_pose_table; [first,
//                first + count) is the hull of its ranges
//   kFrontSkin   trc_skin_vertices, whose palette of n_bones bones is in d_skin_palette; [first, first + count) is the binding's range
//   kFrontMorph  trc_morph_vertices, whose active list of n_active entries is in d_morph_active; [first, first + count) is the morph
//                binding's range, or with n_bones != 0 (the palette in d_skin_palette) the hull of the morph and the skin binding
struct RefitFront {
    enum Kind { kFrontNone, kFrontPose, kFrontSkin, kFrontMorph } kind = kFrontNone;
    uint32_t n_poses = 0, pose_total = 0;
    uint32_t n_bones = 0;
    uint32_t n_active = 0;
};
trc_status refit_run(trc_ctx* ctx, uint32_t first, uint32_t count, const RefitFront& front = RefitFront{}) {
    const DScene& sc = ctx->ks.sc;
    hipEvent_t e0 = ctx->refit_ev[0], e1 = ctx->refit_ev[1];
    hipStream_t st = ctx->stream;
    KRefit p{};
    p.nodes = reinterpret_cast<uint4*>(ctx->d_blob + sc.off_nodes); p.n_nodes = sc.n_nodes;
    p.verts = ctx->d_verts; p.idx = ctx->d_idx; p.n_tri = sc.n_triangles;
    p.ref = ctx->d_bvh_ref; p.refnode = ctx->d_refit_refnode; p.n_ref = ctx->d_bvh_ref ? ctx->n_bvh_ref : 0u;
    p.root = ctx->d_refit_root;
    const dim3 b256(256);
    HIP_TRY(ctx, hipEventRecord(e0, st));
    const uint32_t batches = (uint32_t)(((size_t)count + 255) / 256);
    KSkin k{};
    if (front.n_bones) {      // a skin, or the skin on top of a morph: the skin binding's own range
        k.rest = reinterpret_cast<const float4*>(ctx->d_rest); k.verts = reinterpret_cast<float4*>(ctx->d_verts); k.n_vertex = ctx->n_vertex;
        k.influences = reinterpret_cast<const uint4*>(ctx->d_skin_influences); k.first = ctx->skin_first; k.count = ctx->skin_count;
        k.palette = reinterpret_cast<const float4*>(ctx->d_skin_palette); k.n_bones = front.n_bones;
        k.overflows = reinterpret_cast<uint32_t*>(ctx->d_refit_root) + kPoseCountWord;
    }
    if (front.kind == RefitFront::kFrontPose)
        hipLaunchKernelGGL(k_pose_vertices, dim3((front.pose_total + 255) / 256), b256, 0, st, reinterpret_cast<const float4*>(ctx->d_rest),
                           reinterpret_cast<float4*>(ctx->d_verts), ctx->n_vertex, ctx->d_pose_table, front.n_poses, front.pose_total,
                           reinterpret_cast<uint32_t*>(ctx->d_refit_root) + kPoseCountWord);
    if (front.kind == RefitFront::kFrontSkin) {
        if (front.n_bones <= kSkinLdsBones && !ctx->knobs.skin_no_lds)
            hipLaunchKernelGGL(k_skin_vertices_lds, dim3(std::min(batches, kSkinWorkgroupsPerCu * (uint32_t)ctx->cu_count)), b256, 0, st, k);
        else
            hipLaunchKernelGGL(k_skin_vertices, dim3(batches), b256, 0, st, k);
    }
    if (front.kind == RefitFront::kFrontMorph) {
        KMorph m{};
        m.rest = reinterpret_cast<const float4*>(ctx->d_rest); m.verts = reinterpret_cast<float4*>(ctx->d_verts); m.n_vertex = ctx->n_vertex;
        m.deltas = reinterpret_cast<const float2*>(ctx->d_morph_deltas); m.n_targets = ctx->morph_targets;
        m.first = ctx->morph_first; m.count = ctx->morph_count;
        m.active = static_cast<const uint2*>(ctx->d_morph_active); m.n_active = front.n_active;
        m.overflows = reinterpret_cast<uint32_t*>(ctx->d_refit_root) + kPoseCountWord;
        if (front.n_bones)
            hipLaunchKernelGGL(k_morph_skin_vertices, dim3(batches), b256, 0, st, m, k, first, count);
        else
            hipLaunchKernelGGL(k_morph_vertices, dim3(batches), b256, 0, st, m);
    }
    const bool counted = front.kind != RefitFront::kFrontNone;
    hipLaunchKernelGGL(k_refit_triangles, dim3((sc.n_triangles + 255) / 256), b256, 0, st, ctx->d_verts, ctx->d_idx, sc.n_triangles, first, count,
                       reinterpret_cast<float4*>(ctx->d_blob + sc.off_tripos), reinterpret_cast<float4*>(ctx->d_blob + sc.off_triattr));
    if (ctx->knobs.refit_single) {
        hipLaunchKernelGGL(k_refit_climb, dim3((sc.n_nodes + 255) / 256), b256, 0, st, p, ctx->d_refit_parent, ctx->d_refit_arrive);
    } else {
        const std::vector<uint32_t>& lv = ctx->refit_levels;
        for (size_t d = lv.size() - 1; d-- > 0;)
            hipLaunchKernelGGL(k_refit_level, dim3((lv[d + 1] - lv[d] + 255) / 256), b256, 0, st, p, lv[d], lv[d + 1]);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(e1, st));
    // the root box is a kernel PARAMETER of every launch (KScene): it is copied back behind the refit and read by the next entry
    // point that is entered (trc_refit_settle, at the top of trc_flush and render_pass), so this call does not wait for the device.
    // A pose's or a skin's overflow count travels with it
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_readback, ctx->d_refit_root, (counted ? kPoseCountWord + 1 : 6) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(ctx->refit_ev[2], st));
    ctx->refit_pending = true;
    ctx->refit_posed = counted;
    // the picture changed a little, as under a camera that moves a little (trc_set_camera): the recorded block costs stay, and the
    // next ordered launch is one pass on the last launch's raw durations
    if (ctx->cost_valid) { ctx->plan_streak = 0; ctx->cost_fresh_next = true; }
    return TRC_OK;
}

}  // namespace

// the root box of the last update into ks (a kernel PARAMETER of every launch) and the device time of its kernels; waits for them
trc_status trc_refit_settle_pending(trc_ctx* ctx) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->refit_ev[2]));      // on an error the box stays pending: no launch runs on the old one
    std::memcpy(ctx->ks.root_box, ctx->h_readback, 6 * sizeof(float));
    ctx->refit_pending = false;
    if (ctx->refit_posed) {
        ctx->pose_overflows = ctx->h_readback[kPoseCountWord] - ctx->pose_count_seen;      // (modulo 2^32, as the counter itself)
        ctx->pose_count_seen = ctx->h_readback[kPoseCountWord];
        ctx->refit_posed = false;
    }
    (void)hipEventElapsedTime(&ctx->refit_ms, ctx->refit_ev[0], ctx->refit_ev[1]);
    ctx->normals_timed = false;      // this refit came after any trc_recompute_normals (whose own trc_flush settles what came before it): its time is the last
    return TRC_OK;
}

// the maps follow the tree's topology and numbering: made by refit_prepare, freed with the scene and by trc_rebuild_tree.  The overflow
// counter lives in d_refit_root and starts again at zero with it; a pending read-back has been settled by the caller's trc_flush
void trc_refit_free_maps(trc_ctx* ctx) {
    (void)hipFree(ctx->d_refit_parent); (void)hipFree(ctx->d_refit_arrive); (void)hipFree(ctx->d_refit_root); (void)hipFree(ctx->d_refit_refnode);
    ctx->d_refit_parent = ctx->d_refit_arrive = ctx->d_refit_refnode = nullptr; ctx->d_refit_root = nullptr;
    ctx->pose_count_seen = 0;
    ctx->refit_levels.clear();
}

void trc_refit_free(trc_ctx* ctx) {
    for (hipEvent_t& e : ctx->refit_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    for (hipEvent_t& e : ctx->normals_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    ctx->refit_pending = ctx->refit_posed = ctx->normals_timed = false;
    trc_refit_free_maps(ctx);
    (void)hipFree(ctx->d_adj_offsets); (void)hipFree(ctx->d_adj_corners);
    ctx->d_adj_offsets = ctx->d_adj_corners = nullptr;
    (void)hipFree(ctx->d_verts); (void)hipFree(ctx->d_idx);
    (void)hipFree(ctx->d_rest); (void)hipFree(ctx->d_pose_table);
    ctx->d_rest = nullptr; ctx->d_pose_table = nullptr; ctx->pose_table_bytes = 0;
    ctx->pose_count_seen = ctx->pose_overflows = 0;
    (void)hipFree(ctx->d_skin_influences); (void)hipFree(ctx->d_skin_palette);
    ctx->d_skin_influences = nullptr; ctx->d_skin_palette = nullptr; ctx->skin_palette_bytes = 0;
    ctx->skin_first = ctx->skin_count = ctx->skin_max_bone = 0;
    (void)hipFree(ctx->d_morph_deltas); (void)hipFree(ctx->d_morph_active);
    ctx->d_morph_deltas = nullptr; ctx->d_morph_active = nullptr; ctx->morph_active_bytes = 0;
    ctx->morph_first = ctx->morph_count = ctx->morph_targets = 0;
    ctx->d_verts = nullptr; ctx->d_idx = nullptr; ctx->n_vertex = 0;
}

extern "C" {

trc_status trc_update_vertices(trc_ctx* ctx, const trc_TriangleVertex* vertices, uint32_t first, uint32_t count) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_update_vertices: no scene");
    if (count == 0) return TRC_OK;
    if (!vertices) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: vertices == NULL with count > 0");
    const DScene& sc = ctx->ks.sc;
    if (sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: the scene has no triangles");
    if (first > ctx->n_vertex || count > ctx->n_vertex - first) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: first + count > n_vertex");
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(vertices[i].v[k]) <= 1e37f)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_update_vertices: position not finite or beyond 1e37");
    TRC_TRY(refit_begin(ctx, "trc_update_vertices"));

    hipStream_t st = ctx->stream;
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_verts + first, vertices, (size_t)count * sizeof(trc_TriangleVertex), st));
    // the copy is queued, so from here on the scene changed: what was derived from the old geometry goes
    trc_scene_changed(ctx, kSceneVerticesMoved);     // (TRC_FLAG_MESH_LIGHTS: the areas changed)
    // a scene that has been posed keeps rest vertices: these are the caller's last values for the range
    if (ctx->d_rest) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rest + first, ctx->d_verts + first, (size_t)count * sizeof(trc_TriangleVertex), hipMemcpyDeviceToDevice, st));
    return refit_run(ctx, first, count);
}

trc_status trc_pose_vertices(trc_ctx* ctx, const trc_pose* poses, uint32_t n_poses) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_pose_vertices: no scene");
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
    TRC_TRY(refit_begin(ctx, "trc_pose_vertices"));
    TRC_TRY(trc_grow_buffer(ctx, ctx->d_pose_table, ctx->pose_table_bytes, table.size() * sizeof(trc_pose), "trc_pose_vertices: hipMalloc pose table"));
    hipStream_t st = ctx->stream;
    TRC_TRY(rest_ensure(ctx, "rest vertices (trc_pose_vertices)"));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_pose_table, table.data(), table.size() * sizeof(trc_pose), st));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    RefitFront front;
    front.kind = RefitFront::kFrontPose; front.n_poses = n_poses; front.pose_total = total;
    return refit_run(ctx, hull_first, hull_count, front);
}

trc_status trc_skin_bind(trc_ctx* ctx, const trc_skin_influence* influences, uint32_t first, uint32_t count) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_skin_bind: no scene");
    if (count != 0 && (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_skin_bind: the scene has no triangles");
    uint32_t max_bone = 0;
    if (const char* why = trc_skin_influence_check(influences, first, count, ctx->n_vertex, &max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_skin_bind: ") + why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf table;
    if (count != 0) {
        TRC_TRY(table.alloc(ctx, (size_t)count * sizeof(trc_skin_influence), "influence table (trc_skin_bind)"));
        TRC_TRY(trc_copy_to_device(ctx, table.p, influences, (size_t)count * sizeof(trc_skin_influence), st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));      // a skin still in flight reads the table that goes
    (void)hipFree(ctx->d_skin_influences);
    ctx->d_skin_influences = static_cast<trc_skin_influence*>(table.release());
    ctx->skin_first = count ? first : 0u; ctx->skin_count = count; ctx->skin_max_bone = max_bone;
    return TRC_OK;
}

trc_status trc_skin_vertices(trc_ctx* ctx, const trc_skin_bone* bones, uint32_t n_bones) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_skin_vertices: no scene");
    if (n_bones == 0) return TRC_OK;
    if (!ctx->d_skin_influences || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_skin_vertices: no binding (trc_skin_bind)");
    if (const char* why = trc_skin_palette_check(bones, n_bones, ctx->skin_max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_skin_vertices: ") + why);
    TRC_TRY(refit_begin(ctx, "trc_skin_vertices"));
    const size_t bytes = (size_t)n_bones * sizeof(trc_skin_bone);
    TRC_TRY(trc_grow_buffer(ctx, ctx->d_skin_palette, ctx->skin_palette_bytes, bytes, "trc_skin_vertices: hipMalloc bone palette"));
    TRC_TRY(rest_ensure(ctx, "rest vertices (trc_skin_vertices)"));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_skin_palette, bones, bytes, ctx->stream));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    RefitFront front;
    front.kind = RefitFront::kFrontSkin; front.n_bones = n_bones;
    return refit_run(ctx, ctx->skin_first, ctx->skin_count, front);
}

trc_status trc_morph_bind(trc_ctx* ctx, const trc_morph_delta* deltas, uint32_t n_targets, uint32_t first, uint32_t count) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_morph_bind: no scene");
    const bool empty = trc_morph_table_empty(n_targets, count);
    if (!empty && (ctx->ks.sc.n_triangles == 0 || !ctx->d_verts)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_bind: the scene has no triangles");
    if (const char* why = trc_morph_table_check(deltas, n_targets, first, count, ctx->n_vertex)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_bind: ") + why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf table;
    if (!empty) {
        const size_t bytes = (size_t)n_targets * count * sizeof(trc_morph_delta);      // (size_t: the product passes 2^32)
        TRC_TRY(table.alloc(ctx, bytes, "delta table (trc_morph_bind)"));
        TRC_TRY(trc_copy_to_device(ctx, table.p, deltas, bytes, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));      // a morph still in flight reads the table that goes
    (void)hipFree(ctx->d_morph_deltas);
    ctx->d_morph_deltas = static_cast<trc_morph_delta*>(table.release());
    ctx->morph_first = empty ? 0u : first; ctx->morph_count = empty ? 0u : count; ctx->morph_targets = empty ? 0u : n_targets;
    return TRC_OK;
}

trc_status trc_morph_vertices(trc_ctx* ctx, const float* weights, uint32_t n_weights, const trc_skin_bone* bones, uint32_t n_bones) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_morph_vertices: no scene");
    if (!ctx->d_morph_deltas || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_vertices: no binding (trc_morph_bind)");
    std::vector<trc_morph_active> active;
    if (const char* why = trc_morph_weights_check(weights, n_weights, ctx->morph_targets, active)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_vertices: ") + why);
    uint32_t first = ctx->morph_first, count = ctx->morph_count;
    if (n_bones != 0) {
        if (!ctx->d_skin_influences) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_morph_vertices: n_bones > 0 without a skin binding (trc_skin_bind)");
        if (const char* why = trc_skin_palette_check(bones, n_bones, ctx->skin_max_bone)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_morph_vertices: ") + why);
        // the hull of the two ranges; both end within n_vertex, so neither sum wraps
        const uint32_t end = std::max(first + count, ctx->skin_first + ctx->skin_count);
        first = std::min(first, ctx->skin_first);
        count = end - first;
    }
    TRC_TRY(refit_begin(ctx, "trc_morph_vertices"));
    const size_t list_bytes = active.size() * sizeof(trc_morph_active), palette_bytes = (size_t)n_bones * sizeof(trc_skin_bone);
    TRC_TRY(trc_grow_buffer(ctx, ctx->d_morph_active, ctx->morph_active_bytes, list_bytes, "trc_morph_vertices: hipMalloc active list"));
    if (n_bones != 0) TRC_TRY(trc_grow_buffer(ctx, ctx->d_skin_palette, ctx->skin_palette_bytes, palette_bytes, "trc_morph_vertices: hipMalloc bone palette"));
    TRC_TRY(rest_ensure(ctx, "rest vertices (trc_morph_vertices)"));
    if (list_bytes != 0) TRC_TRY(trc_copy_to_device(ctx, ctx->d_morph_active, active.data(), list_bytes, ctx->stream));
    if (n_bones != 0) TRC_TRY(trc_copy_to_device(ctx, ctx->d_skin_palette, bones, palette_bytes, ctx->stream));
    trc_scene_changed(ctx, kSceneVerticesMoved);
    RefitFront front;
    front.kind = RefitFront::kFrontMorph; front.n_active = (uint32_t)active.size(); front.n_bones = n_bones;
    return refit_run(ctx, first, count, front);
}

// No vertex moves, so no box changes: the gather, then the attribute records of the triangles that name a vertex of the range, and that
// is the chain -- no k_refit_level, no root read-back, refit_pending stays what it was (before the first refit of a scene d_refit_root
// holds zeros, which must never reach ks.root_box), and no refit maps are made or waited for
trc_status trc_recompute_normals(trc_ctx* ctx, uint32_t first, uint32_t count) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_recompute_normals: no scene");
    if (count == 0) return TRC_OK;
    const DScene& sc = ctx->ks.sc;
    if (sc.n_triangles == 0 || !ctx->d_verts) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_recompute_normals: the scene has no triangles");
    if (const char* why = trc_normals_range_check(first, count, ctx->n_vertex)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string("trc_recompute_normals: ") + why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (hipEvent_t& e : ctx->normals_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return trc_fail(ctx, TRC_ERR_HIP, "trc_recompute_normals: hipEventCreate"); }
    TRC_TRY(normals_adjacency(ctx));

    hipStream_t st = ctx->stream;
    KNormals p{};
    p.verts = reinterpret_cast<float4*>(ctx->d_verts); p.n_vertex = ctx->n_vertex;
    p.offsets = ctx->d_adj_offsets; p.corners = ctx->d_adj_corners; p.n_index = 3u * sc.n_triangles;
    p.tripos = ctx->d_blob + sc.off_tripos; p.n_tri = sc.n_triangles;
    p.first = first; p.count = count;
    HIP_TRY(ctx, hipEventRecord(ctx->normals_ev[0], st));
    hipLaunchKernelGGL(k_vertex_normals, dim3((uint32_t)(((size_t)count + 255) / 256)), dim3(256), 0, st, p);
    // from here on the scene changed: what was derived from the old normals goes (the G-buffer's normal plane, the denoiser's history)
    trc_scene_changed(ctx, kSceneVerticesMoved);
    hipLaunchKernelGGL(k_refit_triangles, dim3((sc.n_triangles + 255) / 256), dim3(256), 0, st, ctx->d_verts, ctx->d_idx, sc.n_triangles, first, count,
                       reinterpret_cast<float4*>(ctx->d_blob + sc.off_tripos), reinterpret_cast<float4*>(ctx->d_blob + sc.off_triattr));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->normals_ev[1], st));
    ctx->normals_timed = true;
    if (ctx->cost_valid) { ctx->plan_streak = 0; ctx->cost_fresh_next = true; }      // as after trc_update_vertices: the block costs stay
    return TRC_OK;
}

trc_status trc_download_vertices(trc_ctx* ctx, trc_TriangleVertex* out, uint32_t first, uint32_t count) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_download_vertices: no scene");
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
    *n = ctx->pose_overflows;
    return TRC_OK;
}

trc_status trc_debug_refit_ms(trc_ctx* ctx, float* ms) {
    if (!ctx || !ms) return TRC_ERR_INVALID_ARG;
    TRC_TRY(trc_flush(ctx));
    if (ctx->normals_timed) {      // the family's last call was a trc_recompute_normals, which reads nothing back: its events are waited for here
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipEventSynchronize(ctx->normals_ev[1]));
        (void)hipEventElapsedTime(&ctx->refit_ms, ctx->normals_ev[0], ctx->normals_ev[1]);
        ctx->normals_timed = false;
    }
    *ms = ctx->refit_ms;
    return TRC_OK;
}

}  // extern "C"
