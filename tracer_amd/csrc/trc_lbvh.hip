// trc_lbvh.hip -- on-device LBVH build + fat-node repack.
//
// The reference builds its BVH on the host (RT_Metal/Metal/BVH.hh:35-269) and lists "LBVHs, Morton Encoding"
// as its own to-do (RT_Metal/README.md:42).  trc_upload_scene_lbvh takes the LEAF records (what BVH::buildNode
// writes, BVH.hh:273-314) and builds the hierarchy on the GPU:
//
//   k_lbvh_bounds     centroid bounds of the leaf boxes            wave min/max -> ordered-uint atomics
//   k_lbvh_keys       30-bit Morton code of every centroid          key = code, value = leaf index
//   k_radix_*         stable LSD radix sort, 4 passes x 8 bits      (ties keep leaf-index order)
//   k_lbvh_hierarchy  T. Karras' binary radix tree (HPG 2012) over the 64-bit keys (code << 32 | index)
//   k_lbvh_refit_pass boxes + subtree heights bottom-up             one launch per level, no atomics / fences
//   k_lbvh_rotate_pass two sweeps of SAH tree rotations (Kensler 2008)  one launch per level, refit in between
//   k_lbvh_emit       fat nodes into the scene blob (dev_scene.hpp) + the tree in the reference's own array
//                     layout [root, leaf 0..n-1, interior 1..n-2] (BVH.hh:246-269) for trc_download_bvh
//
// The host side, upload_device_tree, is these steps over one TreeBuild:
//   intake (arguments, blob layout, host-made prefix: the context is untouched) -> replace_scene (the old scene goes; blob, triangle and
//   leaf records, the build's temporaries: from here a failure releases the new scene too) -> leaf_records -> lbvh_topology | sah_build_topology ->
//   fit_boxes (refit passes; the intake flags are looked at here) -> rotate_sweep + fit_boxes, twice (Morton trees only) -> renumber_and_emit -> adopt
//
// trc_rebuild_tree runs the same steps from what the device already holds (rebuild_tree below): the leaf records are slots 1..n of the
// reference-layout tree as the last upload or refit left them -- for a caller's tree (trc_upload_scene), which has none, k_canonical_leaves
// writes them from the fat nodes' leaf slots -- and k_lbvh_emit overwrites the node region of the blob and the records in place.
// trc_tree_cost (k_tree_cost, k_tree_cost_sum) is a surface-area measure of the fat nodes as they stand.
// trc_set_triangle_visibility (trc_visibility.hpp) writes a NEW leaf list -- the analytic leaves of those records, then one per visible triangle --
// and runs the same steps over it with n = n' (rebuild_from_records: the tail it shares with trc_rebuild_tree).
//
// All of it is integer / min-max work on a few bytes per leaf: HBM-bound streaming passes, no MFMA.  The CPU
// statement of the same build is oracle/oracle_lbvh.cpp; tests compare all 2n-1 records bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <memory>
#include <new>

#include "dev_trileaf.hpp"
#include "trc_ctx.hpp"
#include "trc_scene_prep.hpp"

namespace {

constexpr int kSortBlock = 256;
constexpr int kSortItems = 16;                         // keys per thread per tile
constexpr int kSortTile = kSortBlock * kSortItems;     // 4096 keys per workgroup

struct DLeaf {            // 32 B: what the build needs of a 64-B leaf record
    float mn[3]; uint32_t tag;      // tag = pType << 29 | pIndex
    float mx[3]; uint32_t _pad;
};

__device__ __forceinline__ uint32_t ordered_of(float f) {      // monotone float -> uint map
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ void leaf_centroid(const DLeaf& l, float c[3]) {
    c[0] = (l.mn[0] + l.mx[0]) * 0.5f; c[1] = (l.mn[1] + l.mx[1]) * 0.5f; c[2] = (l.mn[2] + l.mx[2]) * 0.5f;
}

// leaf records as uploaded (reference layout, ref_leaves = slot 1 of the output array) -> compact DLeaf; checks
// what trc_upload_scene checks on the host (primitive type / index range) and clears the link fields
struct LeafLimits { uint32_t n[4]; };      // spheres, squares, cubes, triangles
// clear_links == 0 (trc_rebuild_tree): the records are those of the tree in use, which a refused rebuild leaves as it found them; the
// leaves' child links are 0 since their upload and k_lbvh_emit writes every leaf's parent
__global__ void __launch_bounds__(256) k_lbvh_prepare(trc_BVH* ref_leaves, uint32_t n, LeafLimits lim, DLeaf* out, uint32_t* bad, uint32_t clear_links) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    trc_BVH& r = ref_leaves[i];
    const int32_t t = r.pType;
    const uint32_t pi = r.pIndex;
    if (t == TRC_PRIM_BVH) atomicOr(bad, 1u);
    else if (t < 0 || t > TRC_PRIM_TRIANGLE || pi >= lim.n[t]) atomicOr(bad, 2u);
    else if (pi > kTagIndexMask) atomicOr(bad, 4u);
    DLeaf d;
    d.mn[0] = r.bBOX.mini.x; d.mn[1] = r.bBOX.mini.y; d.mn[2] = r.bBOX.mini.z;
    d.mx[0] = r.bBOX.maxi.x; d.mx[1] = r.bBOX.maxi.y; d.mx[2] = r.bBOX.maxi.z;
    d.tag = ((uint32_t)t << kTagIndexBits) | (pi & kTagIndexMask); d._pad = 0;
    out[i] = d;
    if (clear_links) { r.parent = 0; r.left = 0; r.right = 0; }
}

// bounds[0..2] = min, bounds[3..5] = max of the centroids, as ordered uints (init: 0xFFFFFFFF / 0).
// Grid-stride loop, wavefront shuffle reduction, LDS across the 4 wavefronts, 6 atomics per workgroup.
__global__ void __launch_bounds__(256) k_lbvh_bounds(const DLeaf* leaves, uint32_t n, uint32_t* bounds) {
    __shared__ uint32_t part[4][6];
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        float c[3];
        leaf_centroid(leaves[i], c);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (c[a] == c[a]) {                                            // NaN centroids do not take part
                const uint32_t o = ordered_of(c[a]);
                lo[a] = min(lo[a], o); hi[a] = max(hi[a], o);
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off, 64));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off, 64));
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t a = threadIdx.x;
        atomicMin(&bounds[a], min(min(part[0][a], part[1][a]), min(part[2][a], part[3][a])));
        atomicMax(&bounds[3 + a], max(max(part[0][3 + a], part[1][3 + a]), max(part[2][3 + a], part[3][3 + a])));
    }
}

__device__ __forceinline__ uint32_t expand_bits10(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t quantise(float c, float lo, float ext) {
    if (!(ext > 0.0f)) return 0;
    float v = ((c - lo) / ext) * 1024.0f;
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 1023.0f) v = 1023.0f;
    return (uint32_t)v;
}

__global__ void __launch_bounds__(256) k_lbvh_keys(const DLeaf* leaves, uint32_t n, const uint32_t* bounds,
                                                  uint32_t* keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float lo[3], ext[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = float_of(bounds[a]); ext[a] = float_of(bounds[3 + a]) - lo[a]; }
    leaf_centroid(leaves[i], c);
    keys[i] = (expand_bits10(quantise(c[0], lo[0], ext[0])) << 2) | (expand_bits10(quantise(c[1], lo[1], ext[1])) << 1) |
              expand_bits10(quantise(c[2], lo[2], ext[2]));
    vals[i] = i;
}

// ---- stable LSD radix sort, one 8-bit digit per pass.  hist is digit-major: hist[digit * n_blocks + block].
__global__ void __launch_bounds__(kSortBlock) k_radix_hist(const uint32_t* keys, uint32_t n, uint32_t shift, uint32_t* hist, uint32_t n_blocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int r = 0; r < kSortItems; ++r) {
        const uint32_t i = base + r * kSortBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// hist[digit][block] -> exclusive scan along the row of each digit (one workgroup per digit) + row totals;
// k_radix_digit_base then scans the 256 totals.  Output slot of a key = digit_base[d] + hist[d][block] + rank.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= (uint32_t)off) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t block_exclusive_scan256(uint32_t v, uint32_t* wave_tot /* [4] LDS */, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wave_tot[w];
    total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    return before + inc - v;
}
__global__ void __launch_bounds__(256) k_radix_row_scan(uint32_t* hist, uint32_t n_blocks, uint32_t* row_total) {
    __shared__ uint32_t wave_tot[4];
    uint32_t* row = hist + (size_t)blockIdx.x * n_blocks;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < n_blocks; b += 256) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < n_blocks ? row[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan256(v, wave_tot, total);
        if (i < n_blocks) row[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) row_total[blockIdx.x] = carry;
}
__global__ void __launch_bounds__(256) k_radix_digit_base(uint32_t* row_total) {
    __shared__ uint32_t wave_tot[4];
    uint32_t total;
    row_total[threadIdx.x] = block_exclusive_scan256(row_total[threadIdx.x], wave_tot, total);
}

__global__ void __launch_bounds__(kSortBlock) k_radix_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                                             uint32_t* vals_out, uint32_t n, uint32_t shift, const uint32_t* hist,
                                                             const uint32_t* digit_base, uint32_t n_blocks) {
    __shared__ uint32_t run[256];            // next output slot of each digit for this tile
    __shared__ uint32_t wave_cnt[4][256];    // keys of each digit per wavefront in the current round
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    run[threadIdx.x] = digit_base[threadIdx.x] + hist[threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wave_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int r = 0; r < kSortItems; ++r) {
        const uint32_t i = base + r * kSortBlock + threadIdx.x;
        const bool valid = i < n;
        const uint32_t key = valid ? keys_in[i] : 0u, val = valid ? vals_in[i] : 0u;
        const uint32_t digit = (key >> shift) & 255u;
        // lanes of this wavefront that hold the same digit (and are valid)
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wave_cnt[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t off = run[digit] + rank;
            for (uint32_t w = 0; w < wave; ++w) off += wave_cnt[w][digit];
            keys_out[off] = key;
            vals_out[off] = val;
        }
        __syncthreads();
        {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s += wave_cnt[w][threadIdx.x]; wave_cnt[w][threadIdx.x] = 0; }
            run[threadIdx.x] += s;
        }
        __syncthreads();
    }
}

// ---- Karras 2012.  Child encoding: bit 31 = leaf, low bits = sorted position (leaf) or interior index.
constexpr uint32_t kChildLeaf = 0x80000000u;

struct DTopo {
    uint32_t* child_l; uint32_t* child_r;    // [n-1]
    uint32_t* parent_interior;               // [n-1] parent interior index of interior i (root: 0)
    uint32_t* parent_leaf;                   // [n]   parent interior index of sorted leaf position p (kept for tools)
    uint32_t* axis;                          // [n-1]
};

__device__ __forceinline__ int lbvh_delta(const uint32_t* keys, const uint32_t* vals, uint64_t ki, int64_t j, uint32_t n) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const uint64_t kj = ((uint64_t)keys[j] << 32) | vals[j];
    const uint64_t x = ki ^ kj;
    return x ? __clzll((long long)x) : 64;
}

__global__ void __launch_bounds__(256) k_lbvh_hierarchy(const uint32_t* keys, const uint32_t* vals, uint32_t n, DTopo tp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 >= (int64_t)n) return;
    const uint64_t ki = ((uint64_t)keys[i] << 32) | vals[i];
    auto delta = [&](int64_t j) { return lbvh_delta(keys, vals, ki, j, n); };
    const int d = (delta(i + 1) - delta(i - 1)) < 0 ? -1 : 1;
    const int dmin = delta(i - d);
    int64_t lmax = 2;
    while (delta(i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(j);
    int64_t s = 0;
    for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (delta(i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const bool leaf_l = first == gamma, leaf_r = last == gamma + 1;
    tp.child_l[i] = (uint32_t)gamma | (leaf_l ? kChildLeaf : 0u);
    tp.child_r[i] = (uint32_t)(gamma + 1) | (leaf_r ? kChildLeaf : 0u);
    if (leaf_l) tp.parent_leaf[gamma] = (uint32_t)i; else tp.parent_interior[gamma] = (uint32_t)i;
    if (leaf_r) tp.parent_leaf[gamma + 1] = (uint32_t)i; else tp.parent_interior[gamma + 1] = (uint32_t)i;
    const int mbit = dnode - 2;
    tp.axis[i] = (mbit >= 0 && mbit < 30) ? (uint32_t)(mbit % 3) : 0u;
    if (i == 0) tp.parent_interior[0] = 0;
}

// boxes[i] = 6 floats (min xyz, max xyz) of interior i; height[i] = depth of the deepest leaf below i.
// Bottom-up in PASSES, one kernel launch each: a node is fitted in pass p when both children are leaves or were
// fitted in a pass < p (done[i] = pass of fitting, 0 = not yet).  Launch boundaries are the only synchronisation:
// the usual single-kernel climb with one atomic counter per node needs two device-scope fences per level, and on
// the 8-XCD part each fence writes back / invalidates an L2 (measured 6.6 ms for 1 M leaves vs 0.4 ms like this).
// Which of two EQUAL bounds a merged box keeps matters when they are -0 and +0 (the record is compared bit for bit): the
// oracle of the LBVH build merges with std::min / std::max (the FIRST operand on a tie), the reference's SAH build and its
// restatements with fminf / fmaxf, which on the host compile to minss / maxss (the SECOND operand on a tie).  v_min_f32 would
// pick -0 whatever its position.
template <bool SECOND_ON_TIE> __device__ __forceinline__ float tie_min(float a, float b) { return SECOND_ON_TIE ? (a < b ? a : b) : (b < a ? b : a); }
template <bool SECOND_ON_TIE> __device__ __forceinline__ float tie_max(float a, float b) { return SECOND_ON_TIE ? (a > b ? a : b) : (a < b ? b : a); }
template <bool SAH>
__global__ void __launch_bounds__(256) k_lbvh_refit_pass(const DLeaf* leaves, const uint32_t* vals, uint32_t n, DTopo tp,
                                                        float* boxes, uint32_t* height, uint32_t* done, uint32_t pass) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i + 1 >= n || done[i] != 0u) return;
    const uint32_t ch[2] = {tp.child_l[i], tp.child_r[i]};
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (!(ch[k] & kChildLeaf)) { const uint32_t d = done[ch[k]]; if (d == 0u || d >= pass) return; }
    float mn[3], mx[3];
    uint32_t h = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float cmn[3], cmx[3];
        uint32_t hc;
        if (ch[k] & kChildLeaf) {
            const DLeaf& lf = leaves[vals[ch[k] & ~kChildLeaf]];
            cmn[0] = lf.mn[0]; cmn[1] = lf.mn[1]; cmn[2] = lf.mn[2]; cmx[0] = lf.mx[0]; cmx[1] = lf.mx[1]; cmx[2] = lf.mx[2];
            hc = 1;
        } else {
            const float* b = boxes + (size_t)ch[k] * 6;
            cmn[0] = b[0]; cmn[1] = b[1]; cmn[2] = b[2]; cmx[0] = b[3]; cmx[1] = b[4]; cmx[2] = b[5];
            hc = height[ch[k]] + 1;
        }
        if (k == 0) { for (int a = 0; a < 3; ++a) { mn[a] = cmn[a]; mx[a] = cmx[a]; } h = hc; }
        else { for (int a = 0; a < 3; ++a) { mn[a] = tie_min<SAH>(mn[a], cmn[a]); mx[a] = tie_max<SAH>(mx[a], cmx[a]); } h = max(h, hc); }
    }
    float* b = boxes + (size_t)i * 6;
    b[0] = mn[0]; b[1] = mn[1]; b[2] = mn[2]; b[3] = mx[0]; b[4] = mx[1]; b[5] = mx[2];
    height[i] = h;
    done[i] = pass;
}

// ---- tree rotations (A. Kensler, "Tree Rotations for Improving Bounding Volume Hierarchies", RT 2008)
// One bottom-up sweep: every interior node, after all nodes below it, may swap one of its children with a grandchild
// on the other side when that shrinks the surface area of the child that is rebuilt (greedy: best of the <= 4 swaps,
// candidates in a fixed order, strict improvement).  Nodes of equal height have disjoint subtrees, so a sweep is one
// launch per height of the refit that precedes it (sched[i] = height of i then); a rotation changes heights, so
// the tree is refitted before the next sweep.  A Morton-order tree gains most near its top, where the split planes
// ignore the geometry: on the 1 M-triangle scene two sweeps take the box steps per ray from 10.6 to 9.4 (the
// reference's SAH builder: 10.3) and the frame from 20.2 to 19.4 ms, for 1.1 ms of build time.
constexpr int kRotationSweeps = 2;
__device__ __forceinline__ void lbvh_child_box(const DLeaf* leaves, const uint32_t* vals, const float* boxes, uint32_t c, float b[6]) {
    if (c & kChildLeaf) {
        const DLeaf& lf = leaves[vals[c & ~kChildLeaf]];
        b[0] = lf.mn[0]; b[1] = lf.mn[1]; b[2] = lf.mn[2]; b[3] = lf.mx[0]; b[4] = lf.mx[1]; b[5] = lf.mx[2];
    } else {
        const float* q = boxes + (size_t)c * 6;
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = q[a];
    }
}
__device__ __forceinline__ float lbvh_area(const float b[6]) {
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    return 2.0f * ((dx * dy + dy * dz) + dz * dx);
}
__device__ __forceinline__ float lbvh_merged_area(const float a[6], const float b[6]) {
    float m[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { m[k] = fminf(a[k], b[k]); m[3 + k] = fmaxf(a[3 + k], b[3 + k]); }
    return lbvh_area(m);
}
__device__ __forceinline__ void lbvh_set_parent(DTopo tp, uint32_t c, uint32_t parent) {
    if (c & kChildLeaf) tp.parent_leaf[c & ~kChildLeaf] = parent; else tp.parent_interior[c] = parent;
}
__global__ void __launch_bounds__(256) k_lbvh_rotate_pass(const DLeaf* leaves, const uint32_t* vals, uint32_t n, DTopo tp, float* boxes,
                                                         const uint32_t* sched, uint32_t pass) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i + 1 >= n || sched[i] != pass) return;
    const uint32_t L = tp.child_l[i], R = tp.child_r[i];
    float bl[6], br[6];
    lbvh_child_box(leaves, vals, boxes, L, bl);
    lbvh_child_box(leaves, vals, boxes, R, br);
    float best = 0.0f;
    int which = -1;
    uint32_t g0 = 0, g1 = 0;                       // the two children of the interior child of the best swap
    if (!(R & kChildLeaf)) {
        const uint32_t RL = tp.child_l[R], RR = tp.child_r[R];
        float b0[6], b1[6];
        lbvh_child_box(leaves, vals, boxes, RL, b0);
        lbvh_child_box(leaves, vals, boxes, RR, b1);
        const float old = lbvh_area(br);
        const float a0 = lbvh_merged_area(bl, b1);      // swap 0, L <-> RL: R' = (L, RR)
        const float a1 = lbvh_merged_area(b0, bl);      // swap 1, L <-> RR: R' = (RL, L)
        if (old - a0 > best) { best = old - a0; which = 0; g0 = RL; g1 = RR; }
        if (old - a1 > best) { best = old - a1; which = 1; g0 = RL; g1 = RR; }
    }
    if (!(L & kChildLeaf)) {
        const uint32_t LL = tp.child_l[L], LR = tp.child_r[L];
        float b0[6], b1[6];
        lbvh_child_box(leaves, vals, boxes, LL, b0);
        lbvh_child_box(leaves, vals, boxes, LR, b1);
        const float old = lbvh_area(bl);
        const float a2 = lbvh_merged_area(br, b1);      // swap 2, R <-> LL: L' = (R, LR)
        const float a3 = lbvh_merged_area(b0, br);      // swap 3, R <-> LR: L' = (LL, R)
        if (old - a2 > best) { best = old - a2; which = 2; g0 = LL; g1 = LR; }
        if (old - a3 > best) { best = old - a3; which = 3; g0 = LL; g1 = LR; }
    }
    if (which < 0) return;
    // X = the interior child that is rebuilt, `up` = its child that moves up to i, `keep` = the one that stays,
    // `down` = i's other child, which takes the place of `up` below X
    const bool right_side = which < 2;
    const uint32_t X = right_side ? R : L, down = right_side ? L : R;
    const bool first = (which == 0 || which == 2);      // the grandchild that moves up is X's left child
    const uint32_t up = first ? g0 : g1, keep = first ? g1 : g0;
    if (right_side) tp.child_l[i] = up; else tp.child_r[i] = up;
    lbvh_set_parent(tp, up, i);
    if (first) tp.child_l[X] = down; else tp.child_r[X] = down;
    lbvh_set_parent(tp, down, X);
    float bd[6], bk[6];
    lbvh_child_box(leaves, vals, boxes, down, bd);
    lbvh_child_box(leaves, vals, boxes, keep, bk);
    float* q = boxes + (size_t)X * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) { q[k] = tie_min<false>(bd[k], bk[k]); q[3 + k] = tie_max<false>(bd[3 + k], bk[3 + k]); }      // merged(down, keep)
}

// depth of interior node i (root 0): a walk up the parent links, <= TRC_MAX_BVH_DEPTH steps
__global__ void __launch_bounds__(256) k_lbvh_depth(uint32_t n_interior, const uint32_t* parent_interior, uint32_t* keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_interior) return;
    uint32_t d = 0;
    for (uint32_t j = i; j != 0u && d < 255u; j = parent_interior[j]) ++d;
    keys[i] = d; vals[i] = i;
}
// rank[interior] = its position in the depth-sorted order
__global__ void __launch_bounds__(256) k_lbvh_rank(uint32_t n_interior, const uint32_t* sorted_vals, uint32_t* rank) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n_interior) rank[sorted_vals[p]] = p;
}

// fat node of interior i (dev_scene.hpp) + its record in the reference layout; one thread per interior node.  The fat nodes
// are numbered by DEPTH (rank[]: a stable sort of the interior nodes by their depth, root = 0), not by Karras index: any
// prefix of the array is then a top of the tree, which is what the render kernels stage in LDS (stage_scene, k_render_pwg)
// -- the numbering host-built trees get from their BFS walk (trc_abi.hip::build_blob).
__global__ void __launch_bounds__(256) k_lbvh_emit(const DLeaf* leaves, const uint32_t* vals, uint32_t n, DTopo tp, const float* boxes,
                                                  const uint32_t* rank, uint32_t* blob_nodes, trc_BVH* ref) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i + 1 >= n) return;
    const uint32_t ch[2] = {tp.child_l[i], tp.child_r[i]};
    float cb[2][6];
    uint32_t tag[2], slot[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t c = ch[k] & ~kChildLeaf;
        if (ch[k] & kChildLeaf) {
            const uint32_t leaf = vals[c];
            const DLeaf& lf = leaves[leaf];
            cb[k][0] = lf.mn[0]; cb[k][1] = lf.mn[1]; cb[k][2] = lf.mn[2]; cb[k][3] = lf.mx[0]; cb[k][4] = lf.mx[1]; cb[k][5] = lf.mx[2];
            tag[k] = lf.tag;
            slot[k] = leaf + 1u;
        } else {
            const float* b = boxes + (size_t)c * 6;
#pragma unroll
            for (int a = 0; a < 6; ++a) cb[k][a] = b[a];
            tag[k] = (kTagInterior << kTagIndexBits) | rank[c];
            slot[k] = n + c;                                   // interior c >= 1 here (0 is the root)
        }
    }
    uint32_t* q = blob_nodes + (size_t)rank[i] * kNodeDwords;
    q[0] = __float_as_uint(cb[0][0]); q[1] = __float_as_uint(cb[0][1]); q[2] = __float_as_uint(cb[0][2]); q[3] = __float_as_uint(cb[0][3]);
    q[4] = __float_as_uint(cb[0][4]); q[5] = __float_as_uint(cb[0][5]); q[6] = __float_as_uint(cb[1][0]); q[7] = __float_as_uint(cb[1][1]);
    q[8] = __float_as_uint(cb[1][2]); q[9] = __float_as_uint(cb[1][3]); q[10] = __float_as_uint(cb[1][4]); q[11] = __float_as_uint(cb[1][5]);
    q[12] = 0; q[13] = 0; q[14] = tag[0]; q[15] = tag[1];

    const uint32_t self = i == 0 ? 0u : n + i;
    trc_BVH nd;
    memset(&nd, 0, sizeof nd);                                 // padding bytes of the POD are part of the compared record
    const uint32_t pi = tp.parent_interior[i];
    nd.parent = i == 0 ? 0u : (pi == 0 ? 0u : n + pi);
    nd.left = slot[0]; nd.right = slot[1];
    nd.axis = tp.axis[i];
    nd.pType = TRC_PRIM_BVH; nd.pIndex = 0; nd._pad[0] = 0; nd._pad[1] = 0;
    const float* b = boxes + (size_t)i * 6;
    nd.bBOX.mini.x = b[0]; nd.bBOX.mini.y = b[1]; nd.bBOX.mini.z = b[2];
    nd.bBOX.maxi.x = b[3]; nd.bBOX.maxi.y = b[4]; nd.bBOX.maxi.z = b[5];
    ref[self] = nd;
    if (ch[0] & kChildLeaf) ref[slot[0]].parent = self;      // leaf records were uploaded with parent 0;
    if (ch[1] & kChildLeaf) ref[slot[1]].parent = self;      // interior children write their own record
}

// ---- trc_rebuild_tree on a caller's tree (trc_upload_scene): no reference-layout array exists, so the leaf records are written from the
// fat nodes in the canonical order of include/tracer_abi.h -- by pType, then by pIndex.  k_canonical_keys gives child slot s of fat node k
// (value 2k + s) the key first[pType] + pIndex (first[]: prefix sums of the scene's primitive counts) when it holds a leaf and ~0 when it
// holds an interior node; the tree builds' radix sort puts the n leaves in front, in canonical order; k_canonical_leaves writes the leaf at
// sorted position p into record 1 + p (the box from the slot's six floats, padding lanes 0, parent and links 0).  Bad bit 1: a tag that
// names no primitive of the scene, or fewer than n leaves; bit 2: two leaves name the same primitive
struct LeafFirst { uint32_t first[4], n[4]; };
constexpr uint32_t kNoLeafKey = 0xFFFFFFFFu;
__global__ void __launch_bounds__(256) k_canonical_keys(const uint4* __restrict__ nodes, uint32_t n_nodes, LeafFirst lf, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, uint32_t* __restrict__ bad) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    const uint4 q3 = nodes[4 * (size_t)k + 3];
    const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t type = tag[s] >> kTagIndexBits, index = tag[s] & kTagIndexMask;
        uint32_t key = kNoLeafKey;
        if (type != kTagInterior) {
            if (type <= (uint32_t)TRC_PRIM_TRIANGLE && index < lf.n[type]) key = lf.first[type] + index; else atomicOr(bad, 1u);
        }
        keys[2u * k + s] = key; vals[2u * k + s] = 2u * k + s;
    }
}
__global__ void __launch_bounds__(256) k_canonical_leaves(const uint4* __restrict__ nodes, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          LeafFirst lf, uint32_t n_leaves, trc_BVH* __restrict__ ref, uint32_t* __restrict__ bad) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_leaves) return;
    const uint32_t key = keys[p], slot = vals[p];
    if (key == kNoLeafKey) { atomicOr(bad, 1u); return; }
    if (p > 0 && keys[p - 1] == key) atomicOr(bad, 2u);
    const uint32_t type = key >= lf.first[3] ? 3u : key >= lf.first[2] ? 2u : key >= lf.first[1] ? 1u : 0u;
    const uint4* nd = nodes + 4 * (size_t)(slot >> 1);
    const uint4 q0 = nd[0], q1 = nd[1], q2 = nd[2];
    const bool right = (slot & 1u) != 0u;
    uint4* r = reinterpret_cast<uint4*>(&ref[1u + p]);          // a 64-byte record: links + axis | pType, pIndex, padding | mini | maxi
    r[0] = make_uint4(0u, 0u, 0u, 0u);
    r[1] = make_uint4(type, key - lf.first[type], 0u, 0u);
    r[2] = right ? make_uint4(q1.z, q1.w, q2.x, 0u) : make_uint4(q0.x, q0.y, q0.z, 0u);
    r[3] = right ? make_uint4(q2.y, q2.z, q2.w, 0u) : make_uint4(q0.w, q1.x, q1.y, 0u);
}

// ---- trc_tree_cost: half areas of the child slots of every fat node, summed in binary64.  One thread per fat node (grid-stride), the
// node read as k_refit_level reads it (4 x 16 bytes); a wavefront shuffle reduction, the four wavefronts through LDS, ONE partial per
// workgroup; k_tree_cost_sum adds the partials in one workgroup.  No float64 atomics: they execute at the memory side one after the other
// on one address, and the two-launch form gives the same bits for the same grid.  64 B per node, nothing to reuse: bandwidth-trivial.
// d = max - min in binary32, a d that is not > 0 counts as 0; the three products of two binary32 values each are exact in binary64
// (24 + 24 significand bits), so neither contraction nor the fast-math build changes a bit of a slot's value
struct CostPartial { double interior, leaf; uint32_t n_interior, n_leaves; };
__device__ __forceinline__ double half_area(float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    float dx = mxx - mnx, dy = mxy - mny, dz = mxz - mnz;
    if (!(dx > 0.0f)) dx = 0.0f;
    if (!(dy > 0.0f)) dy = 0.0f;
    if (!(dz > 0.0f)) dz = 0.0f;
    return ((double)dx * (double)dy + (double)dy * (double)dz) + (double)dz * (double)dx;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ void cost_block_reduce(double si, double sl, uint32_t ci, uint32_t cl, CostPartial* out) {
    __shared__ double part_d[4][2];
    __shared__ uint32_t part_u[4][2];
    si = wave_sum_f64(si); sl = wave_sum_f64(sl); ci = wave_sum(ci); cl = wave_sum(cl);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { part_d[wave][0] = si; part_d[wave][1] = sl; part_u[wave][0] = ci; part_u[wave][1] = cl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        CostPartial p;
        p.interior = ((part_d[0][0] + part_d[1][0]) + part_d[2][0]) + part_d[3][0];
        p.leaf = ((part_d[0][1] + part_d[1][1]) + part_d[2][1]) + part_d[3][1];
        p.n_interior = part_u[0][0] + part_u[1][0] + part_u[2][0] + part_u[3][0];
        p.n_leaves = part_u[0][1] + part_u[1][1] + part_u[2][1] + part_u[3][1];
        *out = p;
    }
}
__global__ void __launch_bounds__(256) k_tree_cost(const uint4* __restrict__ nodes, uint32_t n_nodes, CostPartial* __restrict__ partial) {
    double si = 0.0, sl = 0.0;
    uint32_t ci = 0, cl = 0;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n_nodes; k += gridDim.x * 256u) {
        const uint4* nd = nodes + 4 * (size_t)k;
        const uint4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        const double h[2] = {half_area(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)),
                             half_area(__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z), __uint_as_float(q2.w))};
        const uint32_t tag[2] = {q3.z, q3.w};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if ((tag[s] >> kTagIndexBits) == kTagInterior) { si += h[s]; ++ci; } else { sl += h[s]; ++cl; }
        }
    }
    cost_block_reduce(si, sl, ci, cl, &partial[blockIdx.x]);
}
__global__ void __launch_bounds__(256) k_tree_cost_sum(const CostPartial* __restrict__ partial, uint32_t n_partial, CostPartial* __restrict__ out) {
    double si = 0.0, sl = 0.0;
    uint32_t ci = 0, cl = 0;
    for (uint32_t i = threadIdx.x; i < n_partial; i += 256u) { const CostPartial p = partial[i]; si += p.interior; sl += p.leaf; ci += p.n_interior; cl += p.n_leaves; }
    cost_block_reduce(si, sl, ci, cl, out);
}
constexpr uint32_t kCostMaxWorkgroups = 2048;      // 8 per CU of 256: every partial is one 24-byte store, the second kernel reads 48 KB at most

// ---- host side.  One 8-bit digit of the sort: n pairs from (keys_in, vals_in) into (keys_out, vals_out); hist: trc_sort_hist_words(n) words
void radix_pass(hipStream_t st, const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t* hist,
                uint32_t* digit_base, uint32_t n, uint32_t shift) {
    const uint32_t n_blocks = (n + kSortTile - 1) / kSortTile;
    hipLaunchKernelGGL(k_radix_hist, dim3(n_blocks), dim3(kSortBlock), 0, st, keys_in, n, shift, hist, n_blocks);
    hipLaunchKernelGGL(k_radix_row_scan, dim3(256), dim3(256), 0, st, hist, n_blocks, digit_base);
    hipLaunchKernelGGL(k_radix_digit_base, dim3(1), dim3(256), 0, st, digit_base);
    hipLaunchKernelGGL(k_radix_scatter, dim3(n_blocks), dim3(kSortBlock), 0, st, keys_in, vals_in, keys_out, vals_out, n, shift, hist, digit_base, n_blocks);
}
// ... and the sort on the `bits` low key bits, from buffer 0 of the two ping-pong arrays; returns the buffer that holds the result
int radix_sort(hipStream_t st, uint32_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* digit_base, uint32_t n, uint32_t bits) {
    int cur = 0;
    for (uint32_t shift = 0; shift < bits; shift += 8, cur ^= 1)
        radix_pass(st, keys[cur], vals[cur], keys[cur ^ 1], vals[cur ^ 1], hist, digit_base, n, shift);
    return cur;
}

// What the steps of a device tree build share.  The device arrays are temporaries (tmp); blob and reference-layout tree are the context's
struct TreeBuild {
    trc_ctx* ctx; hipStream_t st; const trc_scene* s;      // s == nullptr: trc_rebuild_tree -- n, n_interior and sc come from the context's scene (ctx->ks.sc)
    bool sah, triangle_leaves;      // sah: the reference's binned-SAH topology, else Morton order + rotations.  triangle_leaves: bvhList holds
                                    // the analytic primitives' leaves only; one leaf per triangle follows them, written on the device
    bool sah3;                      // with sah: the three-axis, 32-bin split of TRC_TREE_SAH3 in place of the reference's
    uint32_t n = 0, n_interior = 0; DScene sc{}; uint64_t blob_words = 0;
    std::unique_ptr<uint32_t[]> prefix; DevBufs tmp;      // prefix: host side of the blob, analytic primitives + materials
    DLeaf* leaves = nullptr; float* boxes = nullptr; DTopo tp{};
    uint32_t *keys[2] = {}, *vals[2] = {}, *hist = nullptr, *digit_base = nullptr;      // sort ping-pong; vals[cur][position] = leaf index
    uint32_t* bounds = nullptr;               // 6 ordered centroid bounds + word 6 = the leaf-intake flags
    uint32_t *height = nullptr, *arrived = nullptr;      // per interior node: subtree height; pass of fitting (later: its depth rank)
    int cur = 0; uint32_t first_chunk = 40, tree_height = 0;      // sorted buffer; refit passes before the first look at the root; pass that fitted it
    trc_BVH* ref = nullptr;                   // the reference-layout array the steps read the leaf records from and emit into (ctx->d_bvh_ref unless a rebuild makes a new one)
    dim3 g_leaf() const { return dim3((n + 255) / 256); }
    dim3 g_int() const { return dim3((n_interior + 255) / 256); }
};

#include "trc_sah_build.hpp"

// The fat nodes are written by k_lbvh_emit, the triangle records by k_repack_triangles from the caller's arrays: neither is staged on the host
trc_status intake(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx; const trc_scene* const s = b.s;
    if (!s) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "device tree: no scene");
    const uint64_t n_given = s->bvhList ? s->n_bvh : 0u, n_all = n_given + (b.triangle_leaves ? s->n_index / 3 : 0u);
    if ((!s->bvhList && !b.triangle_leaves) || n_all < 2) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "lbvh: need >= 2 leaf records");
    if (n_all > (1u << 28)) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "lbvh: more than 2^28 leaves");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRC_TRY(validate_primitives(ctx, s));
    b.n = (uint32_t)n_all; b.n_interior = b.n - 1;
    TRC_TRY(layout_scene(ctx, s, b.n_interior, b.sc, b.blob_words));
    b.prefix.reset(new (std::nothrow) uint32_t[(size_t)b.sc.off_nodes]());      // zeroed
    if (!b.prefix) return trc_fail(ctx, TRC_ERR_OOM, "lbvh: host staging buffer");
    fill_primitives(s, b.sc, b.prefix.get());
    return TRC_OK;
}

// Room for the build's temporaries in one allocation (DevBufs::reserve): per leaf 32 + 24 B of leaves and boxes, 11 words of sort and
// topology arrays and 2 of the depth sort (109 B with the histograms), for the SAH build 68 B of records in tree order, side array and
// moves and ~20 B of level tables and finish list (198 B in all), under TRC_TREE_SAH3 another 42 B of bin rows (2 688 B for each of the
// n / 64 rows a level can have) and 6 B more of task histograms (246 B in all); `extra`: what a rebuild of a caller's tree sorts before
// that.  An estimate: what it leaves out gets a buffer of its own
void reserve_temporaries(TreeBuild& b, size_t extra = 0) { b.tmp.reserve((size_t)b.n * (b.sah ? (b.sah3 ? 246u : 198u) : 109u) + extra + (64u << 10)); }

// the build's temporary arrays, and the centroid bounds / intake flags at their identities
trc_status work_arrays(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx;
    const uint32_t n = b.n, ni = b.n_interior;
    const char* const what = "tree build: work arrays";
    TRC_TRY(b.tmp.alloc(ctx, &b.leaves, n, what)); TRC_TRY(b.tmp.alloc(ctx, &b.boxes, (size_t)ni * 6, what));
    const struct { uint32_t** p; size_t count; } words[] = {
        {&b.keys[0], n}, {&b.vals[0], n}, {&b.keys[1], n}, {&b.vals[1], n}, {&b.hist, trc_sort_hist_words(n)}, {&b.digit_base, 256}, {&b.bounds, 8},
        {&b.height, ni}, {&b.arrived, ni}, {&b.tp.child_l, ni}, {&b.tp.child_r, ni}, {&b.tp.parent_interior, ni}, {&b.tp.parent_leaf, n}, {&b.tp.axis, ni}};
    for (const auto& w : words) TRC_TRY(b.tmp.alloc(ctx, w.p, w.count, what));
    const uint32_t bounds_init[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u};
    return trc_copy_to_device(ctx, b.bounds, bounds_init, sizeof bounds_init, b.st);
}

// the caller's leaf records go straight to slots 1..n of the reference-layout array (BVH.hh:246-269), the triangles' behind them
trc_status replace_scene(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx;
    const uint64_t n_given = b.s->bvhList ? b.s->n_bvh : 0u;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    trc_scene_changed(ctx, kSceneReplaced);      // another scene: the old one goes, with everything derived from it
    ctx->blob_bytes = (size_t)b.blob_words * 4;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_blob, ctx->blob_bytes));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_bvh_ref, sizeof(trc_BVH) * (2 * (size_t)b.n - 1)));
    TRC_TRY(trc_copy_to_device(ctx, ctx->d_blob, b.prefix.get(), (size_t)b.sc.off_nodes * 4, b.st));
    TRC_TRY(trc_repack_triangles(ctx, b.s, b.sc, ctx->d_blob, b.triangle_leaves ? ctx->d_bvh_ref + 1 + n_given : nullptr));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_bvh_ref, 0, sizeof(trc_BVH), b.st));
    if (n_given) TRC_TRY(trc_copy_to_device(ctx, ctx->d_bvh_ref + 1, b.s->bvhList, sizeof(trc_BVH) * n_given, b.st));
    b.ref = ctx->d_bvh_ref;
    reserve_temporaries(b);
    return work_arrays(b);
}


// the uploaded leaf records (slots 1..n of the reference-layout array) -> compact leaves; what is wrong with them -> the intake flags
void leaf_records(TreeBuild& b) {
    LeafLimits lim;
    lim.n[0] = b.sc.n_spheres; lim.n[1] = b.sc.n_squares; lim.n[2] = b.sc.n_cubes; lim.n[3] = b.sc.n_triangles;
    hipLaunchKernelGGL(k_lbvh_prepare, b.g_leaf(), dim3(256), 0, b.st, b.ref + 1, b.n, lim, b.leaves, b.bounds + 6, b.s ? 1u : 0u);
}

// Morton order and T. Karras' radix tree over it: the sibling of sah_build_topology
void lbvh_topology(TreeBuild& b) {
    hipLaunchKernelGGL(k_lbvh_bounds, dim3(std::min<uint32_t>((b.n + 255) / 256, 1024u)), dim3(256), 0, b.st, b.leaves, b.n, b.bounds);
    hipLaunchKernelGGL(k_lbvh_keys, b.g_leaf(), dim3(256), 0, b.st, b.leaves, b.n, b.bounds, b.keys[0], b.vals[0]);
    b.cur = radix_sort(b.st, b.keys, b.vals, b.hist, b.digit_base, b.n, 32);
    hipLaunchKernelGGL(k_lbvh_hierarchy, b.g_int(), dim3(256), 0, b.st, b.keys[b.cur], b.vals[b.cur], b.n, b.tp);
}

// boxes and heights bottom-up, a tree of height h in h passes; the root is looked at after first_chunk passes, then every 8, the intake flags with it
trc_status fit_boxes(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx;
    uint32_t pass = 0, bad_leaves = 0;
    const uint32_t pass_limit = TRC_MAX_BVH_DEPTH + 1;
    const auto pass_kernel = b.sah ? k_lbvh_refit_pass<true> : k_lbvh_refit_pass<false>;
    b.tree_height = 0;
    HIP_TRY(ctx, hipMemsetAsync(b.arrived, 0, sizeof(uint32_t) * b.n_interior, b.st));
    for (uint32_t chunk = b.first_chunk; pass < pass_limit && !b.tree_height; chunk = 8) {
        for (uint32_t k = 0; k < chunk && pass < pass_limit; ++k)
            hipLaunchKernelGGL(pass_kernel, b.g_int(), dim3(256), 0, b.st, b.leaves, b.vals[b.cur], b.n, b.tp, b.boxes, b.height, b.arrived, ++pass);
        TRC_TRY(trc_read_to_host(ctx, b.st, "tree build: refit", {{&b.tree_height, b.arrived, 4}, {&bad_leaves, b.bounds + 6, 4}}));
        TRC_TRY(intake_status(ctx, bad_leaves));      // k_lbvh_prepare, k_sah_init
    }
    if (!b.tree_height) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "lbvh: tree deeper than TRC_MAX_BVH_DEPTH");
    return TRC_OK;
}

// one sweep of rotations.  arrived[i] = pass in which i was fitted = its height; nodes of height 1 have two leaf children: nothing to rotate
void rotate_sweep(TreeBuild& b) {
    for (uint32_t pass = 2; pass <= b.tree_height; ++pass)
        hipLaunchKernelGGL(k_lbvh_rotate_pass, b.g_int(), dim3(256), 0, b.st, b.leaves, b.vals[b.cur], b.n, b.tp, b.boxes, b.arrived, pass);
}

// fat-node numbering: the interior nodes sorted by depth (one radix pass; the root alone has depth 0), then the fat nodes and the reference-layout tree
trc_status renumber_and_emit(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx;
    uint32_t *depth = b.keys[b.cur ^ 1], *node = b.vals[b.cur ^ 1], *sorted_depth = nullptr, *sorted_node = nullptr;
    for (uint32_t** p : {&sorted_depth, &sorted_node}) TRC_TRY(b.tmp.alloc(ctx, p, b.n_interior, "tree build: depth sort"));
    uint32_t* const rank = b.arrived;              // reuses the arrival array (the heights in b.height are read back by adopt)
    hipLaunchKernelGGL(k_lbvh_depth, b.g_int(), dim3(256), 0, b.st, b.n_interior, b.tp.parent_interior, depth, node);
    radix_pass(b.st, depth, node, sorted_depth, sorted_node, b.hist, b.digit_base, b.n_interior, 0u);
    hipLaunchKernelGGL(k_lbvh_rank, b.g_int(), dim3(256), 0, b.st, b.n_interior, sorted_node, rank);
    hipLaunchKernelGGL(k_lbvh_emit, b.g_int(), dim3(256), 0, b.st, b.leaves, b.vals[b.cur], b.n, b.tp, b.boxes, rank, ctx->d_blob + b.sc.off_nodes, b.ref);
    HIP_TRY(ctx, hipGetLastError());
    return TRC_OK;
}

// the tree's height and root box come back, and the scene becomes the context's
trc_status adopt(TreeBuild& b, const TimedSection& timed) {
    trc_ctx* const ctx = b.ctx;
    uint32_t height = 0; KScene ks{};
    TRC_TRY(trc_read_to_host(ctx, b.st, "tree build: root", {{&height, b.height, 4}, {ks.root_box, b.boxes, sizeof ks.root_box}}));
    if (height > TRC_MAX_BVH_DEPTH) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "lbvh: tree deeper than TRC_MAX_BVH_DEPTH");
    plan_lds(b.sc, height, true);       // the fat nodes are numbered by depth: any prefix may be staged
    ks.sc = b.sc;
    ctx->n_bvh_ref = 2 * b.n - 1;
    ctx->lbvh_height = height;
    ctx->lbvh_build_ms = timed.ms();
    trc_adopt_scene(ctx, ks, b.s);
    return TRC_OK;
}

// everything after the old scene has gone; a failure here leaves upload_device_tree a half-built scene to release
trc_status build_tree(TreeBuild& b) {
    TRC_TRY(replace_scene(b));
    TimedSection timed(b.ctx, b.st);
    leaf_records(b);
    if (b.sah) TRC_TRY(sah_build_topology(b)); else lbvh_topology(b);
    TRC_TRY(fit_boxes(b));
    for (int sweep = 0; !b.sah && sweep < kRotationSweeps; ++sweep) { rotate_sweep(b); TRC_TRY(fit_boxes(b)); }
    TRC_TRY(renumber_and_emit(b));
    timed.stop();
    return adopt(b, timed);
}

// trc_rebuild_tree on a caller's tree: a new reference-layout array with the leaf records in canonical order (k_canonical_leaves); the
// context keeps its own (none) until the rebuild has emitted into this one.  The tree builds' sort arrays are not yet in use
trc_status canonical_leaf_records(TreeBuild& b, DevBuf& new_ref) {
    trc_ctx* const ctx = b.ctx;
    const DScene& sc = b.sc;
    LeafFirst lf;
    const uint32_t counts[4] = {sc.n_spheres, sc.n_squares, sc.n_cubes, sc.n_triangles};
    uint32_t total = 0;
    for (int t = 0; t < 4; ++t) { lf.first[t] = total; lf.n[t] = counts[t]; total += counts[t]; }      // (each below 2^29: no wrap)
    TRC_TRY(new_ref.alloc(ctx, sizeof(trc_BVH) * (2 * (size_t)b.n - 1), "trc_rebuild_tree: tree records"));
    const uint32_t n_slots = 2u * b.n_interior;
    const char* const what = "trc_rebuild_tree: leaf intake";
    uint32_t *keys[2] = {}, *vals[2] = {}, *hist = nullptr, *digit_base = nullptr, *bad = nullptr, flags = 0;
    for (uint32_t** p : {&keys[0], &keys[1], &vals[0], &vals[1]}) TRC_TRY(b.tmp.alloc(ctx, p, n_slots, what));
    TRC_TRY(b.tmp.alloc(ctx, &hist, trc_sort_hist_words(n_slots), what)); TRC_TRY(b.tmp.alloc(ctx, &digit_base, 256, what)); TRC_TRY(b.tmp.alloc(ctx, &bad, 1, what));
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, sizeof(uint32_t), b.st));
    HIP_TRY(ctx, hipMemsetAsync(new_ref.p, 0, sizeof(trc_BVH), b.st));
    const uint4* const nodes = reinterpret_cast<const uint4*>(ctx->d_blob + sc.off_nodes);
    hipLaunchKernelGGL(k_canonical_keys, b.g_int(), dim3(256), 0, b.st, nodes, sc.n_nodes, lf, keys[0], vals[0], bad);
    const int cur = radix_sort(b.st, keys, vals, hist, digit_base, n_slots, 32);
    hipLaunchKernelGGL(k_canonical_leaves, b.g_leaf(), dim3(256), 0, b.st, nodes, keys[cur], vals[cur], lf, b.n, new_ref.as<trc_BVH>(), bad);
    TRC_TRY(trc_read_to_host(ctx, b.st, "trc_rebuild_tree: leaf intake", {{&flags, bad, 4}}));
    if (flags) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_rebuild_tree: two leaves of the tree name the same primitive");
    b.ref = new_ref.as<trc_BVH>();
    return TRC_OK;
}

trc_status rebuild_from_records(TreeBuild& b, DevBuf& new_ref, TimedSection& timed);

// The second way into the steps: everything from what the device holds.  Whatever can refuse comes before renumber_and_emit, which is the first
// to write into the tree in use; from there on only a HIP error can end the call
trc_status rebuild_tree(TreeBuild& b) {
    trc_ctx* const ctx = b.ctx;
    b.sc = ctx->ks.sc; b.n_interior = b.sc.n_nodes; b.n = b.n_interior + 1;
    DevBuf new_ref;
    b.ref = ctx->d_bvh_ref;
    reserve_temporaries(b, b.ref ? 0u : (size_t)b.n * 33u);      // a caller's tree: two key / value pairs over its 2 (n - 1) child slots
    TimedSection timed(ctx, b.st);
    if (!b.ref) TRC_TRY(canonical_leaf_records(b, new_ref));
    return rebuild_from_records(b, new_ref, timed);
}

// ... and the steps from the leaf records in slots 1..b.n of b.ref on, for trc_rebuild_tree and trc_set_triangle_visibility (trc_visibility.hpp)
// alike; b.sc.n_nodes == b.n - 1.  new_ref, where it holds an array, is b.ref and takes the place of the context's when the tree is in place
trc_status rebuild_from_records(TreeBuild& b, DevBuf& new_ref, TimedSection& timed) {
    trc_ctx* const ctx = b.ctx;
    TRC_TRY(work_arrays(b));
    leaf_records(b);
    if (b.sah) TRC_TRY(sah_build_topology(b)); else lbvh_topology(b);
    TRC_TRY(fit_boxes(b));
    for (int sweep = 0; !b.sah && sweep < kRotationSweeps; ++sweep) { rotate_sweep(b); TRC_TRY(fit_boxes(b)); }
    uint32_t height = 0; float root_box[6];
    TRC_TRY(trc_read_to_host(ctx, b.st, "tree rebuild: root", {{&height, b.height, 4}, {root_box, b.boxes, sizeof root_box}}));
    if (height > TRC_MAX_BVH_DEPTH) return trc_fail(ctx, TRC_ERR_BVH_INVALID, "lbvh: tree deeper than TRC_MAX_BVH_DEPTH");
    trc_sppm_order_after_camera(ctx);             // a camera pass running ahead on its own stream still walks the old nodes
    TRC_TRY(renumber_and_emit(b));
    timed.stop();
    // the new tree is on its way: the layout stays (the node region keeps its room), the LDS plan follows the new height, the root box is the new root's
    plan_lds(b.sc, height, true);
    ctx->ks.sc = b.sc;
    std::memcpy(ctx->ks.root_box, root_box, sizeof root_box);
    ctx->lds_scene = b.sc.n_lds_nodes == b.sc.n_nodes;
    ctx->lds_prefix_ok = true;
    if (new_ref.p) {      // (a caller's tree had none; trc_set_triangle_visibility replaces the one it read the analytic leaves from)
        HIP_TRY(ctx, hipStreamSynchronize(b.st));
        (void)hipFree(ctx->d_bvh_ref);
        ctx->d_bvh_ref = static_cast<trc_BVH*>(new_ref.release());
    }
    ctx->n_bvh_ref = 2 * b.n - 1;
    ctx->lbvh_height = height;
    trc_scene_changed(ctx, kSceneTreeRebuilt);
    if (ctx->cost_valid) { ctx->plan_streak = 0; ctx->cost_fresh_next = true; }      // as after trc_update_vertices: one pass on the last launch's raw durations
    HIP_TRY(ctx, hipStreamSynchronize(b.st));       // the temporaries go when this returns; the build's device time is known
    ctx->lbvh_build_ms = timed.ms();
    return TRC_OK;
}

#include "trc_visibility.hpp"

}  // namespace

void trc_sort_pairs24(hipStream_t st, uint32_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* digit_base, uint32_t n, int* result) {
    *result = radix_sort(st, keys, vals, hist, digit_base, n, 24);
}
void trc_sort_pairs(hipStream_t st, uint32_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* digit_base, uint32_t n, uint32_t bits, int* result) {
    *result = radix_sort(st, keys, vals, hist, digit_base, n, bits);
}
uint32_t trc_sort_hist_words(uint32_t n) { return 256u * ((n + kSortTile - 1) / kSortTile); }

// the steps are the list at the top of this file; what the device finds wrong with the leaf records (fit_boxes) is found when the old scene has gone
static trc_status upload_device_tree(trc_ctx* ctx, const trc_scene* s, bool sah, bool triangle_leaves, bool sah3 = false) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    TreeBuild b{ctx, ctx->stream, s, sah, triangle_leaves, sah3};
    TRC_TRY(intake(b));
    const trc_status status = build_tree(b);
    if (status != TRC_OK) trc_release_scene(ctx);
    return status;
}

extern "C" {

trc_status trc_upload_scene_lbvh(trc_ctx* ctx, const trc_scene* s) { return upload_device_tree(ctx, s, false, false); }
trc_status trc_upload_scene_sah(trc_ctx* ctx, const trc_scene* s) { return upload_device_tree(ctx, s, true, false); }
trc_status trc_upload_scene_device(trc_ctx* ctx, const trc_scene* s, uint32_t flags) {
    if (flags & ~(uint32_t)(TRC_TREE_SAH | TRC_TREE_TRIANGLE_LEAVES | TRC_TREE_SAH3)) return ctx ? trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_scene_device: unknown flag") : TRC_ERR_INVALID_ARG;
    if ((flags & TRC_TREE_SAH3) && !(flags & TRC_TREE_SAH)) return ctx ? trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_scene_device: TRC_TREE_SAH3 modifies TRC_TREE_SAH") : TRC_ERR_INVALID_ARG;
    return upload_device_tree(ctx, s, (flags & TRC_TREE_SAH) != 0, (flags & TRC_TREE_TRIANGLE_LEAVES) != 0, (flags & TRC_TREE_SAH3) != 0);
}

trc_status trc_rebuild_tree(trc_ctx* ctx, uint32_t flags) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)(TRC_TREE_SAH | TRC_TREE_SAH3)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_rebuild_tree: flags other than TRC_TREE_SAH, TRC_TREE_SAH3");
    if ((flags & TRC_TREE_SAH3) && !(flags & TRC_TREE_SAH)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_rebuild_tree: TRC_TREE_SAH3 modifies TRC_TREE_SAH");
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_rebuild_tree: no scene");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TreeBuild b{ctx, ctx->stream, nullptr, (flags & TRC_TREE_SAH) != 0, false, (flags & TRC_TREE_SAH3) != 0};
    return rebuild_tree(b);
}

trc_status trc_set_triangle_visibility(trc_ctx* ctx, const trc_triangle_range* ranges, uint32_t n_ranges, uint32_t tree_flags) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    const char* const who = "trc_set_triangle_visibility: ";
    if (tree_flags & ~(uint32_t)(TRC_TREE_SAH | TRC_TREE_SAH3)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "flags other than TRC_TREE_SAH, TRC_TREE_SAH3");
    if ((tree_flags & TRC_TREE_SAH3) && !(tree_flags & TRC_TREE_SAH)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "TRC_TREE_SAH3 modifies TRC_TREE_SAH");
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, std::string(who) + "no scene");
    if (n_ranges && !ranges) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "ranges == NULL with n_ranges > 0");
    if (n_ranges > 0x7FFFFFFEu) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "more than 2^31 - 2 ranges");
    const uint32_t n_tri = ctx->ks.sc.n_triangles;
    std::vector<VisPiece> pieces;      // a range in workgroup-sized pieces, each with its range's stamp: (number + 1) << 1 | visible
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const trc_triangle_range& g = ranges[r];
        if (g.visible > 1u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "visible is neither 0 nor 1");
        if (g.first > n_tri || g.count > n_tri - g.first) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(who) + "first + count > n_index / 3");
        for (uint32_t off = 0; off < g.count; off += kVisPiece) pieces.push_back(VisPiece{g.first + off, std::min(kVisPiece, g.count - off), ((r + 1u) << 1) | g.visible});
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TreeBuild b{ctx, ctx->stream, nullptr, (tree_flags & TRC_TREE_SAH) != 0, false, (tree_flags & TRC_TREE_SAH3) != 0};
    return set_visibility(b, pieces);
}

trc_status trc_download_triangle_visibility(trc_ctx* ctx, uint8_t* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_download_triangle_visibility: no scene");
    const uint32_t n_tri = ctx->ks.sc.n_triangles;
    if (n_tri == 0) return TRC_OK;
    if (!out) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_triangle_visibility: out == NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_vis) TRC_TRY(vis_make_explicit(ctx, "trc_download_triangle_visibility"));
    return trc_copy_to_host(ctx, out, ctx->d_vis, n_tri, ctx->stream);      // synchronous
}

trc_status trc_debug_visibility_ms(trc_ctx* ctx, float* leaf_list_ms) {
    if (!ctx || !leaf_list_ms) return TRC_ERR_INVALID_ARG;
    *leaf_list_ms = ctx->vis_leaf_ms;
    return TRC_OK;
}

trc_status trc_tree_cost(trc_ctx* ctx, trc_tree_cost_t* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!out) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_tree_cost: out == NULL");
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_tree_cost: no scene");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const DScene& sc = ctx->ks.sc;
    const uint32_t n_wg = std::min<uint32_t>((sc.n_nodes + 255) / 256, kCostMaxWorkgroups);
    DevBuf partial;
    TRC_TRY(partial.alloc(ctx, sizeof(CostPartial) * ((size_t)n_wg + 1), "trc_tree_cost: partial sums"));
    CostPartial* const d_partial = partial.as<CostPartial>();
    hipLaunchKernelGGL(k_tree_cost, dim3(n_wg), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4*>(ctx->d_blob + sc.off_nodes), sc.n_nodes, d_partial);
    hipLaunchKernelGGL(k_tree_cost_sum, dim3(1), dim3(256), 0, ctx->stream, d_partial, n_wg, d_partial + n_wg);
    CostPartial sum{};
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "trc_tree_cost", {{&sum, d_partial + n_wg, sizeof sum}}));
    const float* r = ctx->ks.root_box;
    float d[3];
    for (int a = 0; a < 3; ++a) { d[a] = r[3 + a] - r[a]; if (!(d[a] > 0.0f)) d[a] = 0.0f; }
    out->root_half_area = ((double)d[0] * (double)d[1] + (double)d[1] * (double)d[2]) + (double)d[2] * (double)d[0];
    out->interior_half_area = sum.interior; out->leaf_half_area = sum.leaf;
    out->n_interior = sum.n_interior; out->n_leaves = sum.n_leaves;
    return TRC_OK;
}

trc_status trc_download_bvh(trc_ctx* ctx, trc_BVH* out, uint32_t capacity, uint32_t* n_nodes) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_bvh_ref || ctx->n_bvh_ref == 0) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_download_bvh: no device-built tree (trc_upload_scene_lbvh)");
    if (n_nodes) *n_nodes = ctx->n_bvh_ref;
    if (!out) return TRC_OK;
    if (capacity < ctx->n_bvh_ref) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_bvh: capacity too small");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_copy_to_host(ctx, out, ctx->d_bvh_ref, sizeof(trc_BVH) * ctx->n_bvh_ref, ctx->stream);      // synchronous
}

trc_status trc_lbvh_info(trc_ctx* ctx, uint32_t* n_nodes, uint32_t* height, float* device_build_ms) {
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (ctx->n_bvh_ref == 0) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_lbvh_info: no device-built tree");
    if (n_nodes) *n_nodes = ctx->n_bvh_ref;
    if (height) *height = ctx->lbvh_height;
    if (device_build_ms) *device_build_ms = ctx->lbvh_build_ms;
    return TRC_OK;
}

}  // extern "C"
