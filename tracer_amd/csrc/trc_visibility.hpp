// trc_visibility.hpp -- trc_set_triangle_visibility / trc_download_triangle_visibility (tracer_abi.h): which of the
// mesh's triangles have a leaf.  Part of trc_lbvh.hip (included inside its unnamed namespace, like trc_sah_build.hpp): the call is a
// third way into the tree build's steps, and it shares their sort.
//
//   k_vis_from_tree        first call of a scene: the mask from the fat nodes' leaf tags, one byte per triangle (atomicOr on the word that
//                          holds it); a triangle named twice, or a triangle tag that names none: the `bad` word
//   k_vis_stamp            one workgroup per piece of a range (<= kVisPiece triangles): atomicMax of (range number + 1) << 1 | visible on a
//                          4-byte stamp per triangle -- the LAST range that covers a triangle wins whatever order the workgroups run in
//   k_vis_apply            four triangles per thread: stamp -> mask byte, and the partition's key (0 visible, 1 hidden) and value (t)
//   radix_pass             ONE stable 8-bit pass of the builds' sort over that key: the visible triangles in front, ascending; the pass's
//                          digit table holds their count (digit_base[1])
//   k_vis_leaf_keys        the same partition over the leaf records the rebuild would start from: key 1 for a triangle's leaf
//   k_vis_gather_leaves    the analytic leaves' 64-byte records in that order into slots 1..na of the new array, four lanes per record
//   k_vis_triangle_leaves  one 64-byte record per visible triangle behind them: triangle_leaf_box of its three current vertices
//
// Streaming passes over at most 64 B per leaf, every access to a record, a key or a stamp 16 bytes wide.  From there rebuild_from_records
// runs the builds' own steps with n = n'.
#pragma once

constexpr uint32_t kVisPiece = 65536;      // triangles of a range that one workgroup of k_vis_stamp stamps: 256 per thread
struct VisPiece { uint32_t first, count, stamp; };
inline size_t vis_mask_bytes(uint32_t n_tri) { return ((size_t)n_tri + 15u) & ~(size_t)15u; }

__global__ void __launch_bounds__(256) k_vis_from_tree(const uint4* __restrict__ nodes, uint32_t n_nodes, uint32_t n_tri, uint32_t* __restrict__ mask_words,
                                                       uint32_t* __restrict__ bad) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    const uint4 q3 = nodes[4 * (size_t)k + 3];
    const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if ((tag[s] >> kTagIndexBits) != kTagTriangle) continue;
        const uint32_t t = tag[s] & kTagIndexMask;
        if (t >= n_tri) { atomicOr(bad, 1u); continue; }
        const uint32_t bit = 1u << (8u * (t & 3u));
        if (atomicOr(&mask_words[t >> 2], bit) & bit) atomicOr(bad, 2u);
    }
}

__global__ void __launch_bounds__(256) k_vis_stamp(const VisPiece* __restrict__ pieces, uint32_t n_tri, uint32_t* __restrict__ stamp) {
    const VisPiece p = pieces[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < p.count; i += 256u) {
        const uint32_t t = p.first + i;
        if (t < n_tri) atomicMax(&stamp[t], p.stamp);
    }
}

// the arrays are padded to a multiple of four triangles; a lane past n_tri is hidden and takes no part in the sort (it sorts n_tri keys)
__global__ void __launch_bounds__(256) k_vis_apply(uint32_t* __restrict__ mask_words, uint32_t n_tri, const uint4* __restrict__ stamp,
                                                   uint4* __restrict__ keys, uint4* __restrict__ vals) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, t0 = 4u * w;
    if (t0 >= n_tri) return;
    const uint32_t m = mask_words[w];
    const uint4 st = stamp ? stamp[w] : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t s[4] = {st.x, st.y, st.z, st.w};
    uint32_t v[4], out = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        v[j] = s[j] ? (s[j] & 1u) : ((m >> (8u * j)) & 1u);
        if (t0 + j >= n_tri) v[j] = 0u;
        out |= v[j] << (8u * j);
    }
    mask_words[w] = out;
    keys[w] = make_uint4(1u - v[0], 1u - v[1], 1u - v[2], 1u - v[3]);
    vals[w] = make_uint4(t0, t0 + 1u, t0 + 2u, t0 + 3u);
}

__global__ void __launch_bounds__(256) k_vis_leaf_keys(const trc_BVH* __restrict__ leaves, uint32_t n, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 r1 = reinterpret_cast<const uint4*>(&leaves[i])[1];      // pType, pIndex, padding
    keys[i] = r1.x == (uint32_t)TRC_PRIM_TRIANGLE ? 1u : 0u;
    vals[i] = i;
}

__global__ void __launch_bounds__(256) k_vis_gather_leaves(const trc_BVH* __restrict__ src, const uint32_t* __restrict__ order, uint32_t n_src, uint32_t n,
                                                           trc_BVH* __restrict__ dst) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, i = g >> 2, q = g & 3u;
    if (i >= n) return;
    const uint32_t from = order[i];
    if (from >= n_src) return;
    reinterpret_cast<uint4*>(&dst[i])[q] = reinterpret_cast<const uint4*>(&src[from])[q];
}

__global__ void __launch_bounds__(256) k_vis_triangle_leaves(const trc_TriangleVertex* __restrict__ verts, const uint32_t* __restrict__ idx, uint32_t n_tri,
                                                             const uint32_t* __restrict__ visible, uint32_t n_visible, trc_BVH* __restrict__ dst) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_visible) return;
    const uint32_t t = visible[i];
    if (t >= n_tri) return;
    const trc_TriangleVertex a = verts[idx[3 * (size_t)t]], b = verts[idx[3 * (size_t)t + 1]], c = verts[idx[3 * (size_t)t + 2]];
    float mn[3], mx[3];
    triangle_leaf_box(a, b, c, mn, mx);
    uint4* r = reinterpret_cast<uint4*>(&dst[i]);               // links + axis | pType, pIndex, padding | mini | maxi (k_canonical_leaves)
    r[0] = make_uint4(0u, 0u, 0u, 0u);
    r[1] = make_uint4((uint32_t)TRC_PRIM_TRIANGLE, t, 0u, 0u);
    r[2] = make_uint4(__float_as_uint(mn[0]), __float_as_uint(mn[1]), __float_as_uint(mn[2]), 0u);
    r[3] = make_uint4(__float_as_uint(mx[0]), __float_as_uint(mx[1]), __float_as_uint(mx[2]), 0u);
}

// the mask the tree in use defines, into `mask` (vis_mask_bytes, zeroed here); what is wrong with the tree into *bad (zeroed by the caller)
inline trc_status vis_mask_from_tree(trc_ctx* ctx, hipStream_t st, void* mask, uint32_t* bad) {
    const DScene& sc = ctx->ks.sc;
    HIP_TRY(ctx, hipMemsetAsync(mask, 0, vis_mask_bytes(sc.n_triangles), st));
    hipLaunchKernelGGL(k_vis_from_tree, dim3((sc.n_nodes + 255) / 256), dim3(256), 0, st, reinterpret_cast<const uint4*>(ctx->d_blob + sc.off_nodes), sc.n_nodes,
                       sc.n_triangles, static_cast<uint32_t*>(mask), bad);
    return TRC_OK;
}
inline trc_status vis_refuse_tree(trc_ctx* ctx, const char* who) {
    return trc_fail(ctx, TRC_ERR_UNSUPPORTED, std::string(who) + ": two leaves of the tree name the same triangle");
}

// trc_download_triangle_visibility on a scene whose mask is still implicit
trc_status vis_make_explicit(trc_ctx* ctx, const char* who) {
    DevBuf mask, bad;
    uint32_t flags = 0;
    TRC_TRY(mask.alloc(ctx, vis_mask_bytes(ctx->ks.sc.n_triangles), "triangle visibility: mask"));
    TRC_TRY(bad.alloc(ctx, 256, "triangle visibility: mask"));
    HIP_TRY(ctx, hipMemsetAsync(bad.p, 0, 4, ctx->stream));
    TRC_TRY(vis_mask_from_tree(ctx, ctx->stream, mask.p, bad.as<uint32_t>()));
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "triangle visibility: mask", {{&flags, bad.p, 4}}));
    if (flags) return vis_refuse_tree(ctx, who);
    ctx->d_vis = static_cast<uint8_t*>(mask.release());
    return TRC_OK;
}

// The third way into the steps.  The ranges have been checked; b.sah / b.sah3 are set.  Everything up to rebuild_from_records writes into
// arrays of its own -- a copy of the mask, a new reference-layout array -- so a refusal leaves mask and tree as they were
trc_status set_visibility(TreeBuild& b, const std::vector<VisPiece>& pieces) {
    trc_ctx* const ctx = b.ctx;
    hipStream_t st = b.st;
    const char* const who = "trc_set_triangle_visibility";
    const DScene cur = ctx->ks.sc;
    const uint32_t n_tri = cur.n_triangles, n_tri4 = (n_tri + 3u) & ~3u, n_old = cur.n_nodes + 1u;
    const uint32_t room = (cur.off_tripos - cur.off_nodes) / kNodeDwords + 1u;      // leaves the node region was laid out for (layout_scene)
    DevBuf new_mask, canon, new_ref;
    // the build's temporaries are sized for a full tree; in front of them: stamps, two key / value pairs and a histogram over the triangles, the same
    // over the leaves, the pieces, and what a caller's tree sorts for its canonical records
    b.sc = cur; b.n_interior = room - 1u; b.n = room;
    reserve_temporaries(b, (size_t)n_tri4 * 21u + (size_t)n_old * (ctx->d_bvh_ref ? 17u : 50u) + pieces.size() * sizeof(VisPiece) + (16u << 10));
    b.n_interior = cur.n_nodes; b.n = n_old;
    TimedSection timed(ctx, st), leaf_stage(ctx, st);

    uint32_t *bad = nullptr, *stamp = nullptr, *tkeys[2] = {}, *tvals[2] = {}, *thist = nullptr, *tbase = nullptr;
    uint32_t *lkeys[2] = {}, *lvals[2] = {}, *lhist = nullptr, *lbase = nullptr;
    TRC_TRY(b.tmp.alloc(ctx, &bad, 1, who));
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    if (n_tri) {
        TRC_TRY(new_mask.alloc(ctx, vis_mask_bytes(n_tri), "trc_set_triangle_visibility: mask"));
        for (uint32_t** p : {&tkeys[0], &tkeys[1], &tvals[0], &tvals[1]}) TRC_TRY(b.tmp.alloc(ctx, p, n_tri4, who));
        TRC_TRY(b.tmp.alloc(ctx, &thist, trc_sort_hist_words(n_tri), who)); TRC_TRY(b.tmp.alloc(ctx, &tbase, 256, who));
        if (ctx->d_vis) HIP_TRY(ctx, hipMemcpyAsync(new_mask.p, ctx->d_vis, vis_mask_bytes(n_tri), hipMemcpyDeviceToDevice, st));
        else TRC_TRY(vis_mask_from_tree(ctx, st, new_mask.p, bad));
        if (!pieces.empty()) {
            VisPiece* d_pieces = nullptr;
            TRC_TRY(b.tmp.alloc(ctx, &stamp, n_tri4, who)); TRC_TRY(b.tmp.alloc(ctx, &d_pieces, pieces.size(), who));
            HIP_TRY(ctx, hipMemsetAsync(stamp, 0, sizeof(uint32_t) * n_tri4, st));
            TRC_TRY(trc_copy_to_device(ctx, d_pieces, pieces.data(), pieces.size() * sizeof(VisPiece), st));
            hipLaunchKernelGGL(k_vis_stamp, dim3((uint32_t)pieces.size()), dim3(256), 0, st, d_pieces, n_tri, stamp);
        }
        hipLaunchKernelGGL(k_vis_apply, dim3((n_tri4 / 4u + 255u) / 256u), dim3(256), 0, st, new_mask.as<uint32_t>(), n_tri, reinterpret_cast<const uint4*>(stamp),
                           reinterpret_cast<uint4*>(tkeys[0]), reinterpret_cast<uint4*>(tvals[0]));
        radix_pass(st, tkeys[0], tvals[0], tkeys[1], tvals[1], thist, tbase, n_tri, 0u);
    }
    // the analytic leaves, from the records a rebuild would start from
    const trc_BVH* src = ctx->d_bvh_ref;
    if (!src) { TRC_TRY(canonical_leaf_records(b, canon)); src = canon.as<trc_BVH>(); }
    for (uint32_t** p : {&lkeys[0], &lkeys[1], &lvals[0], &lvals[1]}) TRC_TRY(b.tmp.alloc(ctx, p, n_old, who));
    TRC_TRY(b.tmp.alloc(ctx, &lhist, trc_sort_hist_words(n_old), who)); TRC_TRY(b.tmp.alloc(ctx, &lbase, 256, who));
    hipLaunchKernelGGL(k_vis_leaf_keys, dim3((n_old + 255) / 256), dim3(256), 0, st, src + 1, n_old, lkeys[0], lvals[0]);
    radix_pass(st, lkeys[0], lvals[0], lkeys[1], lvals[1], lhist, lbase, n_old, 0u);
    uint32_t flags = 0, n_visible = 0, n_analytic = 0;
    if (n_tri) TRC_TRY(trc_read_to_host(ctx, st, who, {{&flags, bad, 4}, {&n_visible, tbase + 1, 4}, {&n_analytic, lbase + 1, 4}}));
    else TRC_TRY(trc_read_to_host(ctx, st, who, {{&flags, bad, 4}, {&n_analytic, lbase + 1, 4}}));
    if (flags) return vis_refuse_tree(ctx, who);
    if (n_visible > n_tri || n_analytic > n_old) return trc_fail(ctx, TRC_ERR_HIP, "trc_set_triangle_visibility: partition counts out of range");
    const uint64_t n_new = (uint64_t)n_analytic + n_visible;
    if (n_new < 2) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_set_triangle_visibility: fewer than 2 leaves left");
    if (n_new > room) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_set_triangle_visibility: more leaves than the uploaded tree has room for");
    TRC_TRY(new_ref.alloc(ctx, sizeof(trc_BVH) * (2 * (size_t)room - 1), "trc_set_triangle_visibility: tree records"));
    trc_BVH* const ref = new_ref.as<trc_BVH>();
    HIP_TRY(ctx, hipMemsetAsync(ref, 0, sizeof(trc_BVH), st));
    if (n_analytic) hipLaunchKernelGGL(k_vis_gather_leaves, dim3((4u * n_analytic + 255u) / 256u), dim3(256), 0, st, src + 1, lvals[1], n_old, n_analytic, ref + 1);
    if (n_visible) hipLaunchKernelGGL(k_vis_triangle_leaves, dim3((n_visible + 255u) / 256u), dim3(256), 0, st, ctx->d_verts, ctx->d_idx, n_tri, tvals[1], n_visible,
                                      ref + 1 + n_analytic);
    HIP_TRY(ctx, hipGetLastError());
    leaf_stage.stop();
    b.ref = ref; b.n = (uint32_t)n_new; b.n_interior = b.n - 1u; b.sc.n_nodes = b.n_interior;
    TRC_TRY(rebuild_from_records(b, new_ref, timed));      // (synchronises the stream at its end)
    ctx->vis_leaf_ms = leaf_stage.ms();
    if (n_tri) { (void)hipFree(ctx->d_vis); ctx->d_vis = static_cast<uint8_t*>(new_mask.release()); }
    return TRC_OK;
}
