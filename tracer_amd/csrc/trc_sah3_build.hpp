// trc_sah3_build.hpp -- the kernels of TRC_TREE_SAH3 (included by trc_sah_build.hpp after the kernels of TRC_TREE_SAH, which stay as they
// are).  The definition is in include/tracer_abi.h: every axis of positive centroid extent, 32 bins, cost = n0 A(B0) + n1 A(B1), first
// minimum in (axis, i) order.  The level loop, the tables, k_sah_init / k_sah_scatter / k_sah_apply / k_sah_vals are the SAH build's; a
// level here is
//     k_sah3_bins    per task: ONE pass over its records fills the bins of all three axes (8 LDS copies of a 672-word row), one set of
//                    atomics per task into the node's row of the level's bin table; the task's 96 counts are kept for the scatter
//     k_sah3_price   one WAVEFRONT per node: per axis, lanes 0..31 hold the prefix unions of the bins and lanes 32..63 the suffix unions
//                    (two 32-lane scans side by side), lane i < 31 prices split i; a wave-wide first minimum
//     k_sah3_split   one lane per node: topology and the children's rows, as k_sah_split's second half
// and subtrees of <= 64 leaves are finished by k_sah3_finish, which prices the 93 candidates straight from the records in LDS.
// A bin is 7 words: the count, the three box minima as INVERTED ordered uints and the three maxima as ordered uints -- every word grows
// under atomicAdd / atomicMax and its identity is 0, so a level's table is reset by one memset.  min / max and counts are exact in any
// order; only the cost has an order, and it is computed in one place per kernel.

constexpr uint32_t kBin3Copies = 8, kBin3Stride = kRow3 + 1u;      // odd stride: the copies start in different banks; 8 x 673 words = 21.5 KB

__device__ __forceinline__ float sah3_cost(uint32_t n0, const float mn0[3], const float mx0[3], uint32_t n1, const float mn1[3], const float mx1[3]) {
    return (float)n0 * sah_area(mn0, mx0) + (float)n1 * sah_area(mn1, mx1);
}

__global__ void __launch_bounds__(256) k_sah3_bins(const DLeaf* elems, const SNode* nodes, const uint32_t* task_node, uint32_t* bins3, uint32_t* task_hist) {
    __shared__ uint32_t s_bin[kBin3Copies * kBin3Stride];
    const uint32_t t = blockIdx.x, node = task_node[t];
    const SNode& N = nodes[node];
    const uint32_t p0 = N.first + (t - N.task0) * kChunk, p1 = min(N.last, p0 + kChunk);
    float lo[3], extent[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = float_of(N.cb[a]); extent[a] = float_of(N.cb[3 + a]) - lo[a]; }
    for (uint32_t i = threadIdx.x; i < kBin3Copies * kBin3Stride; i += 256u) s_bin[i] = 0u;
    __syncthreads();
    uint32_t* mine = s_bin + (threadIdx.x & (kBin3Copies - 1u)) * kBin3Stride;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256u) {
        const DLeaf d = elems[p];
        uint32_t key[6];
#pragma unroll
        for (int a = 0; a < 3; ++a) { key[a] = ~ordered_of(d.mn[a]); key[3 + a] = ordered_of(d.mx[a]); }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(extent[a] > 0.0f)) continue;                             // a skipped axis: its bins stay empty
            uint32_t* w = mine + ((uint32_t)a * kBins3 + sah3_bin(sah_centroid1(d.mn[a], d.mx[a]), lo[a], extent[a])) * 7u;
            atomicAdd(&w[0], 1u);
#pragma unroll
            for (int k = 0; k < 6; ++k) atomicMax(&w[1 + k], key[k]);
        }
    }
    __syncthreads();
    uint32_t* row = bins3 + (size_t)node * kRow3;
    for (uint32_t w = threadIdx.x; w < kRow3; w += 256u) {
        const bool is_count = (w % 7u) == 0u;
        uint32_t v = 0u;
        for (uint32_t c = 0; c < kBin3Copies; ++c) {
            const uint32_t x = s_bin[c * kBin3Stride + w];
            v = is_count ? v + x : max(v, x);
        }
        if (is_count) task_hist[(size_t)t * (3u * kBins3) + w / 7u] = v;
        if (v) { if (is_count) atomicAdd(&row[w], v); else atomicMax(&row[w], v); }
    }
}

// One wavefront per node of the level.  Lane l: half h = l >> 5, j = l & 31; half 0 holds bin j and scans towards higher lanes (prefix:
// bins 0..j), half 1 holds bin 31 - j and does the same (suffix: bins 31 - j..31).  Split i has its left side in lane i and its right side
// (bins i + 1..31) in lane 32 + (30 - i).
__global__ void __launch_bounds__(256) k_sah3_price(SNode* nodes, uint32_t n_rows, const uint32_t* bins3, uint32_t* row_axis) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                             // a whole wavefront; no barrier below
    SNode& N = nodes[row];
    const uint32_t j = lane & 31u, bin = lane < 32u ? j : 31u - j;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    float best = 0.0f; uint32_t best_key = kNone, best_below = 0u;        // key = axis * 31 + i: the order of the definition
    for (uint32_t a = 0; a < 3u; ++a) {
        const float lo = float_of(N.cb[a]), extent = float_of(N.cb[3u + a]) - lo;
        if (!(extent > 0.0f)) continue;                                    // uniform: the row is the wavefront's
        const uint32_t* w = bins3 + (size_t)row * kRow3 + (a * kBins3 + bin) * 7u;
        uint32_t cnt = w[0];
        float mn[3], mx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = cnt ? float_of(~w[1 + k]) : FLT_MAX; mx[k] = cnt ? float_of(w[4 + k]) : -FLT_MAX; }
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const uint32_t tc = (uint32_t)__shfl_up((int)cnt, off, 32);
            float tmn[3], tmx[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { tmn[k] = __shfl_up(mn[k], off, 32); tmx[k] = __shfl_up(mx[k], off, 32); }
            if (j >= (uint32_t)off) {
                cnt += tc;
#pragma unroll
                for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], tmn[k]); mx[k] = fmaxf(mx[k], tmx[k]); }
            }
        }
        const int src = lane < 31u ? (int)(62u - lane) : (int)lane;
        const uint32_t rc = (uint32_t)__shfl((int)cnt, src, 64);
        float rmn[3], rmx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { rmn[k] = __shfl(mn[k], src, 64); rmx[k] = __shfl(mx[k], src, 64); }
        if (lane < 31u && cnt && rc) {                                     // an empty side: the candidate is skipped
            const float cost = sah3_cost(cnt, mn, mx, rc, rmn, rmx);
            if (best_key == kNone || cost < best) { best = cost; best_key = a * 31u + lane; best_below = cnt; }
        }
    }
    // first minimum over the lanes: the lower cost, then the lower key (costs are never NaN: the boxes are finite and no count is 0)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oc = __shfl_xor(best, off, 64);
        const uint32_t ok = (uint32_t)__shfl_xor((int)best_key, off, 64), ob = (uint32_t)__shfl_xor((int)best_below, off, 64);
        if (ok != kNone && (best_key == kNone || oc < best || (oc == best && ok < best_key))) { best = oc; best_key = ok; best_below = ob; }
    }
    if (lane == 0u) {
        const uint32_t first = N.first, last = N.last;
        const bool fallback = best_key == kNone;                           // no axis of positive extent: identical centroids
        N.split = fallback ? 0u : best_key % 31u;
        N.n_below = fallback ? 0u : best_below;
        N.mid = fallback ? first + (last - first) / 2u : first + best_below;      // both sides of a priced split are non-empty
        N.fallback = fallback ? 1u : 0u;
        row_axis[row] = fallback ? 2u : best_key / 31u;
    }
}

// One lane per node: the node's topology record, rows / tasks / finish entries of its children with one atomic per wavefront and
// counter -- k_sah_split without the pricing, which k_sah3_price has done
__global__ void __launch_bounds__(64) k_sah3_split(SNode* nodes, uint32_t n_rows, const uint32_t* row_axis, SNode* next_nodes, uint32_t* next_counts /* [2]: nodes, tasks */,
                                                  SFinish* finish, uint32_t* counters, DTopo tp, uint32_t n, uint32_t level) {
    const uint32_t lane = threadIdx.x, row = blockIdx.x * 64u + lane;
    const bool has = row < n_rows;
    uint32_t c_first[2] = {0, 0}, c_last[2] = {0, 0}, c_q[2] = {0, 0}, c_tasks[2] = {0, 0};
    uint32_t need_rows = 0, need_tasks = 0, need_finish = 0;
    bool c_row[2] = {false, false}, c_fin[2] = {false, false};
    if (has) {
        const SNode& N = nodes[row];
        const uint32_t first = N.first, last = N.last, qbase = N.qbase, mid = N.mid, span = last - first;
        const uint32_t self = sah_id_of(qbase + span - 2u, n);
        uint32_t link[2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint32_t cf = side ? mid : first, cl = side ? last : mid, cs = cl - cf;
            const uint32_t cq = side ? qbase + (mid - first) - 1u : qbase;
            c_first[side] = cf; c_last[side] = cl; c_q[side] = cq;
            if (cs == 1u) { link[side] = kChildLeaf | cf; tp.parent_leaf[cf] = self; atomicMax(&counters[2], level + 1u); continue; }
            const uint32_t ci = sah_id_of(cq + cs - 2u, n);
            link[side] = ci; tp.parent_interior[ci] = self;
            if (cs <= kFinishSpan) { c_fin[side] = true; ++need_finish; }
            else { c_row[side] = true; c_tasks[side] = (cs + kChunk - 1) / kChunk; ++need_rows; need_tasks += c_tasks[side]; }
        }
        tp.child_l[self] = link[0]; tp.child_r[self] = link[1]; tp.axis[self] = row_axis[row];
        if (self == 0u) tp.parent_interior[0] = 0u;
    }
    const uint32_t inc_rows = wave_inclusive_scan(need_rows, lane), inc_tasks = wave_inclusive_scan(need_tasks, lane),
                   inc_fin = wave_inclusive_scan(need_finish, lane);
    uint32_t base_rows = 0, base_tasks = 0, base_fin = 0;
    if (lane == 63u) {
        if (inc_rows) { base_rows = atomicAdd(&next_counts[0], inc_rows); base_tasks = atomicAdd(&next_counts[1], inc_tasks); }
        if (inc_fin) base_fin = atomicAdd(&counters[0], inc_fin);
    }
    uint32_t my_row = (uint32_t)__shfl((int)base_rows, 63, 64) + inc_rows - need_rows;
    uint32_t my_task = (uint32_t)__shfl((int)base_tasks, 63, 64) + inc_tasks - need_tasks;
    uint32_t my_fin = (uint32_t)__shfl((int)base_fin, 63, 64) + inc_fin - need_finish;
    uint32_t child_row[2] = {kNoNode, kNoNode}, child_t0[2] = {0, 0};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        if (c_fin[side]) { SFinish f; f.first = c_first[side]; f.last = c_last[side]; f.qbase = c_q[side]; f.depth = level + 1u; finish[my_fin++] = f; }
        if (c_row[side]) {
            child_row[side] = my_row++; child_t0[side] = my_task; my_task += c_tasks[side];
            SNode& c = next_nodes[child_row[side]];        // header and identity centroid bounds (k_sah_scatter accumulates them)
            c.first = c_first[side]; c.last = c_last[side]; c.qbase = c_q[side]; c.task0 = child_t0[side];
#pragma unroll
            for (int a = 0; a < 6; ++a) c.cb[a] = a < 3 ? 0xFFFFFFFFu : 0u;
        }
    }
    if (has) { SNode& N = nodes[row]; N.child[0] = child_row[0]; N.child[1] = child_row[1]; N.child_t0[0] = child_t0[0]; N.child_t0[1] = child_t0[1]; }
}

// One wavefront per subtree of <= 64 leaves, lane p = position p of its range, every level of the subtree one trip: k_sah_finish with the
// split of TRC_TREE_SAH3.  No bins: the lane at offset o of a node of s positions prices candidates o, o + s, ... of the 93 straight from
// the node's s records in LDS (their bins on the three axes packed into a word per position); counts and unions are what bins would give.
__global__ void __launch_bounds__(64) k_sah3_finish(const DLeaf* elems, const SFinish* finish, uint32_t* vals, uint32_t* counters, DTopo tp, uint32_t n) {
    constexpr uint32_t kNone = 0xFFFFFFFFu, kCandidates = 3u * (kBins3 - 1u);
    __shared__ float s_c[3][64], s_mn[3][64], s_mx[3][64];      // by record (the lane that loaded it)
    __shared__ uint32_t s_ord[64], s_x[64];                      // by position: the record there; exchange
    __shared__ uint32_t s_pk[64], s_key[64];                     // by position: its bins, 8 bits per axis; the best candidate of the lane there
    __shared__ float s_cost[64];
    const uint32_t lane = threadIdx.x;
    const SFinish f = finish[blockIdx.x];
    const uint32_t F = f.first, S = min(f.last - f.first, 64u);
    uint32_t leaf = 0;
    if (lane < S) {
        const DLeaf d = elems[F + lane];
        leaf = d._pad;
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_mn[a][lane] = d.mn[a]; s_mx[a][lane] = d.mx[a]; s_c[a][lane] = sah_centroid1(d.mn[a], d.mx[a]); }
    }
    s_ord[lane] = lane;
    uint32_t nf = 0, nl = S, nq = f.qbase, depth = f.depth;
    __syncthreads();
    for (;; ++depth) {
        const uint32_t span = nl - nf;
        const bool active = lane < S && span >= 2u;
        if (__ballot(active) == 0ull) break;
        // centroid bounds of the node: a scan that stops at the node's first position, then the last position's value
        const uint32_t me = s_ord[lane < S ? lane : 0u];
        float c[3], lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { c[a] = s_c[a][me]; lo[a] = c[a]; hi[a] = c[a]; }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const bool take = lane >= nf + (uint32_t)off;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float tl = __shfl_up(lo[a], off, 64), th = __shfl_up(hi[a], off, 64);
                if (take) { lo[a] = fminf(lo[a], tl); hi[a] = fmaxf(hi[a], th); }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = __shfl(lo[a], (int)((nl - 1u) & 63u), 64); hi[a] = __shfl(hi[a], (int)((nl - 1u) & 63u), 64); }
        uint32_t mid = nf + 1u;
        bool below = false, moved = false;
        uint32_t rank = 0;
        const uint32_t axis2 = sah_widest(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);      // of a node of two leaves, BVH.hh:59-77
        {
            const float my_key = axis2 == 0 ? c[0] : (axis2 == 1 ? c[1] : c[2]);
            const float ka = __shfl(my_key, (int)(nf & 63u), 64), kb = __shfl(my_key, (int)((nf + 1u) & 63u), 64);
            if (active && span == 2u && !(ka < kb)) { moved = true; rank = 0; below = lane != nf; }      // the two change places
        }
        const bool wide = active && span > 2u;
        // bins of this position's record on the axes that are considered
        bool use[3]; uint32_t bk[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float extent = hi[a] - lo[a];
            use[a] = extent > 0.0f;
            bk[a] = (wide && use[a]) ? sah3_bin(c[a], lo[a], extent) : 0u;
        }
        s_pk[lane] = bk[0] | bk[1] << 8 | bk[2] << 16;
        __syncthreads();
        float best = 0.0f; uint32_t best_key = kNone;
        for (uint32_t cand = lane - nf; wide && cand < kCandidates; cand += span) {
            const uint32_t a = cand / 31u, i = cand % 31u;
            if (!(a == 0 ? use[0] : (a == 1 ? use[1] : use[2]))) continue;
            float mn0[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx0[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            float mn1[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx1[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            uint32_t n0 = 0, n1 = 0;
            for (uint32_t q = nf; q < nl; ++q) {
                const uint32_t r = s_ord[q] & 63u;
                if (((s_pk[q] >> (8u * a)) & 255u) <= i) {
                    ++n0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { mn0[k] = fminf(mn0[k], s_mn[k][r]); mx0[k] = fmaxf(mx0[k], s_mx[k][r]); }
                } else {
                    ++n1;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { mn1[k] = fminf(mn1[k], s_mn[k][r]); mx1[k] = fmaxf(mx1[k], s_mx[k][r]); }
                }
            }
            if (!n0 || !n1) continue;                                              // an empty side: skipped
            const float cost = sah3_cost(n0, mn0, mx0, n1, mn1, mx1);
            if (best_key == kNone || cost < best) { best = cost; best_key = cand; }
        }
        s_cost[lane] = best; s_key[lane] = best_key;
        __syncthreads();
        // first minimum over the node's lanes: the lower cost, then the lower candidate
        best_key = kNone;
        for (uint32_t q = nf; wide && q < nl && q - nf < kCandidates; ++q) {
            const uint32_t k = s_key[q];
            const float cq = s_cost[q];
            if (k != kNone && (best_key == kNone || cq < best || (cq == best && k < best_key))) { best = cq; best_key = k; }
        }
        const bool degenerate = best_key == kNone;                                 // no axis of positive extent: identical centroids
        const uint32_t axis = degenerate ? 2u : best_key / 31u, split = degenerate ? 0u : best_key % 31u;
        if (wide && !degenerate) below = (axis == 0 ? bk[0] : (axis == 1 ? bk[1] : bk[2])) <= split;
        const unsigned long long node_mask = (span >= 64u ? ~0ull : ((1ull << span) - 1ull)) << nf;
        const unsigned long long bm = __ballot(wide && !degenerate && below) & node_mask;
        if (wide) {
            const uint32_t n_below = (uint32_t)__popcll(bm);
            mid = nf + n_below;
            const bool fallback = degenerate || mid <= nf || mid >= nl;
            if (fallback) {
                if (!degenerate && lane == nf) atomicOr(&counters[1], 16u);        // a priced split has two non-empty sides: cannot happen
                mid = nf + span / 2u;
            } else {
                const unsigned long long lt = (1ull << lane) - 1ull;
                if (lane < mid && !below) { moved = true; rank = (uint32_t)__popcll(~bm & node_mask & lt); }
                else if (lane >= mid && below) { moved = true; rank = (uint32_t)__popcll(bm & ~lt & ~(1ull << lane)); }
            }
        }
        // the k-th misplaced record from the left changes places with the k-th from the right (BVH.hh:154-168)
        const bool from_right = moved && below;
        if (moved && !from_right) s_x[(nf + rank) & 63u] = me;
        if (from_right) s_x[(nl - 1u - rank) & 63u] = me;
        __syncthreads();
        if (moved) s_ord[lane] = from_right ? s_x[(nf + rank) & 63u] : s_x[(nl - 1u - rank) & 63u];
        __syncthreads();
        if (active && lane == nf) {
            const uint32_t self = sah_id_of(nq + span - 2u, n);
            const uint32_t sl = mid - nf, sr = nl - mid, rq = nq + sl - 1u;
            uint32_t l, r;
            if (sl == 1u) { l = kChildLeaf | (F + nf); tp.parent_leaf[F + nf] = self; }
            else { l = sah_id_of(nq + sl - 2u, n); tp.parent_interior[l] = self; }
            if (sr == 1u) { r = kChildLeaf | (F + mid); tp.parent_leaf[F + mid] = self; }
            else { r = sah_id_of(rq + sr - 2u, n); tp.parent_interior[r] = self; }
            tp.child_l[self] = l; tp.child_r[self] = r; tp.axis[self] = span == 2u ? axis2 : axis;
            if (self == 0u) tp.parent_interior[0] = 0u;
        }
        if (active) {
            if (lane < mid) nl = mid; else { nq = nq + (mid - nf) - 1u; nf = mid; }
        }
    }
    if (lane == 0u) atomicMax(&counters[2], depth);      // every trip put its nodes' children one level further down
    // leaf indices in their final order
    __shared__ uint32_t s_leaf[64];
    s_leaf[lane] = leaf;
    __syncthreads();
    if (lane < S) vals[F + lane] = s_leaf[s_ord[lane] & 63u];
}
