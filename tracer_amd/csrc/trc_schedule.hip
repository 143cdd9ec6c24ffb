// trc_schedule.hip -- the launch schedule of the render pass: the pixel-block list of a rank's share (trc_ensure_tiles), the
// adaptive launch order and the cost-adaptive block size with their kernels (schedule_blocks), and what is known about the
// blocks' costs (drop_stale_costs, trc_debug_block_costs).  Pixels depend on none of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "trc_launch.hpp"

// sort keys of the adaptive launch order: descending cost (shader clocks / 64, clamped to 24 bits), ties in list order.
// Lists that may be split (stride kCostSlots): the last launch may have run an 8x8 block as four quarters (split[i] != 0),
// and a quarter as four sixteenths (qsplit[4 i + q]).  A block's cost as ONE block is then what it measured when it last ran
// whole (whole[i], kept by k_build_launch), or -- a first launch made of quarters only -- an estimate from its slowest part
// on the high side.
constexpr float kQuarterCost = 0.85f;        // a quarter's duration relative to its 8x8 block's: what the plan assumes for
                                             // a block it has not split yet (measured: 0.8-0.9 for the blocks that matter)
constexpr float kQuarterEstimate = 0.65f;
constexpr float kSixteenthTier = 0.8f;       // quarters within this factor of the launch's longest part go on to 2x2 blocks
// the slowest part of block i that the last launch ran (quarters, the sixteenths of the quarters that were split again, their pixels)
__device__ __forceinline__ uint32_t slowest_part(const uint32_t* cost, const uint32_t* qsplit, uint32_t i) {
    const uint32_t* c = cost + (size_t)i * kCostSlots;
    uint32_t m = 0u;
    for_each_part(qsplit, i, [&](uint32_t slot) { m = max(m, c[slot]); });
    return m;
}
// What a block's duration says about the block.  A SIMD issues from its oldest wavefronts first (tools/probe/age_probe.hip:
// of five wavefronts on a SIMD the first two run as fast as a lone one, the fifth takes 1.8x as long), so the duration a
// wavefront measures is its own work only if it started among the first of its SIMD; started later, the same block lasts up
// to twice as long.  Sorting by the raw durations therefore feeds back on itself: a heavy block that ran first looks light,
// starts late in the next launch, looks heavy again.  The order and the plan work on the SHORTEST duration seen lately
// instead (it grows by 1/64 per launch until a measurement undercuts it, so a scene that changes is followed): config 2
// 20.9 -> 20.4 ms, its shares of 2 / 4 / 8 ranks 12.3 -> 11.1, 8.5 -> 7.3, 5.95 -> 5.6 ms (knob no_cost_filter switches it off).
// One thread per block filters the slots its last launch wrote (the block, its quarters or their sixteenths).
__device__ __forceinline__ void filter_block_costs(const uint32_t* cost, const uint32_t* split, const uint32_t* qsplit, uint32_t stride, uint32_t i,
                                                   uint32_t* filt, uint32_t* whole, const bool fresh) {
    // fresh: what the filter holds are the durations of a cold HEAD (8 samples, row-major, trc_render) -- good enough to order
    // and plan the launch that followed, but no "shortest duration seen lately" of a settled launch: that launch's replace them
    auto slot = [&](uint32_t k) {
        const size_t at = (size_t)i * stride + k;
        const uint32_t f = filt[at], c = cost[at];
        filt[at] = (f && !fresh) ? min(f + (f >> 6) + 1u, c) : c;
    };
    if (stride != kCostSlots || !split[i]) { slot(0u); return; }
    for_each_part(qsplit, i, slot);
    // What the block cost when it last ran WHOLE ranks it for as long as it runs in parts (a value measured under the same
    // conditions as its unsplit neighbours': re-estimating it from the parts every launch made the plan settle elsewhere,
    // config 3 329 -> 344-366 ms).  It only follows the parts DOWN when they say the block is no longer what it was (a camera
    // or a scene that moved on): a quarter lasts 0.8-0.9 of its block, so parts below half of `whole` are another picture's.
    const uint32_t w = whole[i];
    if (w) whole[i] = max(1u, min(w, (uint32_t)((float)slowest_part(filt, qsplit, i) * 2.0f)));
}
// One thread per block: (1) filter the slots its last launch wrote (the block, its quarters or their sixteenths) into `filt`
// (skipped with the knob no_cost_filter: filt == cost then), (2) the block's sort key: its cost as ONE block, descending.
__global__ void __launch_bounds__(256) k_order_keys(const uint32_t* raw, uint32_t* cost, const uint32_t* split, uint32_t* whole, const uint32_t* qsplit,
                                                    uint32_t stride, uint32_t n, uint32_t* keys, uint32_t* vals, const bool filtered, const bool fresh) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (filtered) filter_block_costs(raw, split, qsplit, stride, i, cost, whole, fresh);
    uint32_t c = cost[(size_t)i * stride];
    if (stride == kCostSlots && split[i])
        c = whole[i] ? whole[i] : (uint32_t)((float)slowest_part(cost, qsplit, i) * (1.0f / kQuarterEstimate));
    keys[i] = 0xFFFFFFu - min(c, 0xFFFFFFu);
    vals[i] = i;
}

// Cost-adaptive block size.  A block's samples are a sequential chain, so a launch cannot end before its slowest
// wavefront; a rank that owns about as many 8x8 blocks as the GPU has wavefront slots (a strong-scaled share of a frame)
// lasts exactly that long, while most slots sit idle.  An 8x8 block run as four 4x4 quarters on 16 lanes each ends earlier
// (a quarter waits for 16 pixels' branches, not 64) but occupies four slots and issues ~3x the instructions -- so only
// the blocks that would otherwise decide the launch are split.  Input: the blocks in descending order of their cost as
// whole blocks (keys[r] = 0xFFFFFF - cost, vals[r] = block).  Model of a launch that splits the K most expensive blocks:
//     makespan(K) = max( cost[K], longest part, (sum + (4 * kQuarterCost - 1) * prefix(K)) / slots )
// -- the longest block left whole; the longest part: the slowest quarter / sixteenth MEASURED in the previous launch, and
// kQuarterCost x the most expensive block that launch ran whole if K reaches it; the work over the wavefront slots.  One
// workgroup picks the smallest K <= k_max that minimises it: a launch with many more blocks than slots gets K = 0 from
// the third term, an eighth of a 1080p frame splits the few blocks above the longest part.
// Second level: where wavefront slots are still idle after that (entries < slots), the quarters within kSixteenthTier of the
// launch's longest part -- the ones the launch now ends on -- run as four 2x2 sixteenths on 4 lanes each in the next launch;
// plan[3] = the threshold a quarter's duration must reach, plan[4] = how many do, plan[1] = the entries of the launch.
// per RANK r of the sorted order (block i = vals[r]), gathered by one thread each so that the one-workgroup planner below reads
// dense arrays: part[r] = the slowest part the last launch ran of it (0: it ran whole), rawv[r] = its measured duration when
// it ran whole (else -1), quart[4 r + q] = quarter q's cost when the block ran in parts and that quarter ran as ONE (else 0;
// 0xFFFFFFFF: it already ran as sixteenths)
__global__ void __launch_bounds__(256) k_plan_gather(const uint32_t* vals, const uint32_t* split, const uint32_t* cost, const uint32_t* qsplit,
                                                     const uint32_t* raw, uint32_t n, uint32_t* part, float* rawv, uint32_t* quart, uint32_t* sixt) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t i = vals[r];
    const bool sp = split[i] != 0u;
    part[r] = sp ? slowest_part(cost, qsplit, i) : 0u;
    rawv[r] = sp ? -1.0f : (float)raw[(size_t)i * kCostSlots];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t m = sp ? qsplit[4u * i + q] : 0u;
        quart[4u * r + q] = !sp ? 0u : ((m & 1u) ? 0xFFFFFFFFu : cost[(size_t)i * kCostSlots + q]);
        // third level: sixteenth s of a quarter that ran as sixteenths -- its cost as ONE sixteenth (0xFFFFFFFF: it already ran as
        // pixels; 0: its quarter ran whole, nothing is known about it)
        for (uint32_t s4 = 0; s4 < 4u; ++s4)
            sixt[16u * r + 4u * q + s4] = !(m & 1u) ? 0u : (((m >> (kPixelBit + s4)) & 1u) ? 0xFFFFFFFFu : cost[(size_t)i * kCostSlots + 4u + 4u * q + s4]);
    }
}
// exclusive prefix sum over the 1024 threads of the workgroup (wave shuffles, then the 16 wave totals); returns the total
__device__ __forceinline__ double block_scan_1024(double v, double* s_wave /* [16] */, double& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const double o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc += o; }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    double base = 0.0, tot = 0.0;
#pragma unroll
    for (uint32_t w = 0; w < 16u; ++w) { const double x = s_wave[w]; if (w < wave) base += x; tot += x; }
    __syncthreads();
    total = tot;
    return base + inc - v;
}
__global__ void __launch_bounds__(1024) k_plan_split(const uint32_t* keys, const uint32_t* part, const float* rawv, const uint32_t* quart, const uint32_t* sixt,
                                                     uint32_t n, uint32_t k_max, const uint32_t slots, const uint32_t max_entries, uint32_t* plan, uint32_t* launch) {
    __shared__ double s_wave[16];
    __shared__ float s_best[1024];
    __shared__ uint32_t s_k[1024], s_q[1024], s_first[1024];
    __shared__ float s_raw[1024], s_est[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
    double local = 0.0;
    float raw_sum = 0.0f, est_sum = 0.0f;          // blocks the last launch ran whole: measured durations / filtered costs
    uint32_t q_max = 0u, first_whole = 0xFFFFFFFFu;
    for (uint32_t r = lo; r < hi; ++r) {
        const float c = (float)(0xFFFFFFu - keys[r]);
        local += (double)c;
        const uint32_t pr = part[r];
        if (pr) q_max = max(q_max, pr);
        else {
            if (first_whole == 0xFFFFFFFFu) first_whole = r;
            raw_sum += rawv[r]; est_sum += c;
        }
    }
    double total = 0.0;
    double prefix = block_scan_1024(local, s_wave, total);          // cost of the blocks before rank `lo`
    s_q[t] = q_max; s_first[t] = first_whole; s_raw[t] = raw_sum; s_est[t] = est_sum;
    __syncthreads();
    for (uint32_t off = 512u; off > 0u; off >>= 1) {
        if (t < off) { s_q[t] = max(s_q[t], s_q[t + off]); s_first[t] = min(s_first[t], s_first[t + off]); s_raw[t] += s_raw[t + off]; s_est[t] += s_est[t + off]; }
        __syncthreads();
    }
    // the costs are what a block takes when it starts first on its SIMD; a wavefront slot is held for the measured
    // duration: the work term scales by the ratio of the two over the blocks that ran whole
    const double held = s_est[0] > 0.0f ? (double)fminf(fmaxf(s_raw[0] / s_est[0], 1.0f), 4.0f) : 1.0;      // slot time per unit of cost
    const float part_seen = (float)s_q[0];
    const uint32_t r_whole = s_first[0];            // most expensive block the previous launch ran whole
    __syncthreads();
    if (t == 0) plan[2] = (uint32_t)min(held * total / (double)slots, 4294967295.0);   // diagnostic: work / slots of the unsplit launch
    const float quarter_new = r_whole < n ? kQuarterCost * (float)(0xFFFFFFu - keys[r_whole]) : 0.0f;
    const double extra = 4.0 * (double)kQuarterCost - 1.0;
    float best = 3.0e38f;
    uint32_t best_k = 0;
    auto candidate = [&](uint32_t k, float whole) {       // split ranks 0 .. k-1
        const float pt = k == 0u ? 0.0f : (k > r_whole ? fmaxf(part_seen, quarter_new) : part_seen);
        const float work = (float)(held * (total + extra * prefix) / (double)slots);
        const float m = fmaxf(fmaxf(whole, pt), work);
        if (m < best) { best = m; best_k = k; }
    };
    // fewer blocks than wavefront slots: the parts must not push the launch into a second round of wavefronts
    if (n < slots) k_max = min(k_max, (slots - n) / 3u);
    for (uint32_t k = lo; k < hi && k <= k_max; ++k) {
        candidate(k, (float)(0xFFFFFFu - keys[k]));
        prefix += (double)(0xFFFFFFu - keys[k]);
    }
    if (hi == n && lo < hi && n <= k_max) candidate(n, 0.0f);          // ... and "every block as quarters"
    s_best[t] = best; s_k[t] = best_k;
    __syncthreads();
    for (uint32_t off = 512u; off > 0u; off >>= 1) {
        if (t < off) {
            const float a = s_best[t], b = s_best[t + off];
            if (b < a || (b == a && s_k[t + off] < s_k[t])) { s_best[t] = b; s_k[t] = s_k[t + off]; }
        }
        __syncthreads();
    }
    // the plan feeds back on itself (parts that end earlier lower the bar for the next launch's split): K moves by at most
    // half of its previous value (+ 16) per launch, so the launch time settles instead of swinging
    const uint32_t k_prev = plan[6];               // 0xFFFFFFFF: the previous launch was not planned from measurements
    const uint32_t K = k_prev == 0xFFFFFFFFu ? s_k[0] : min(max(s_k[0], k_prev - k_prev / 2u), k_prev + k_prev / 2u + 16u);
    __syncthreads();
    // second level: the quarters of blocks that were quarters last launch too and lasted at least `tier`, as long as every
    // entry of the launch still gets a wavefront slot of its own
    // ... or, with more entries than slots, as long as the launch is bound by its longest part and not by its work
    const uint32_t entries1 = n + 3u * K;
    const float work_bound = (float)(held * total / (double)slots);    // the unsplit launch's work over the slots
    const bool tail_bound = entries1 < slots || work_bound < 0.7f * part_seen;
    const uint32_t tier = tail_bound && part_seen > 0.0f ? max(1u, (uint32_t)(kSixteenthTier * part_seen)) : 0xFFFFFFFFu;
    uint32_t have = 0u, want = 0u;                  // quarters that already run as sixteenths / that would join them
    for (uint32_t j = t; j < 4u * K; j += 1024u) {
        const uint32_t cq = quart[j];
        if (cq == 0u) continue;                                        // becomes quarters now: their durations are not known yet
        if (cq == 0xFFFFFFFFu) have++;
        else if (cq >= tier) want++;
    }
    s_k[t] = have; s_q[t] = want;
    __syncthreads();
    for (uint32_t off = 512u; off > 0u; off >>= 1) { if (t < off) { s_k[t] += s_k[t + off]; s_q[t] += s_q[t + off]; } __syncthreads(); }
    const uint32_t room = min(max_entries, max(slots, entries1 + slots / 8u)) - entries1;      // entries the sixteenths may add
    uint32_t K2 = s_k[0] + s_q[0], use_tier = tier, keep = 1u;
    if (12u * K2 > room) { K2 = s_k[0]; use_tier = 0xFFFFFFFFu; }                 // no new ones
    if (12u * K2 > room) { K2 = 0u; keep = 0u; }                                  // not even the old ones: back to quarters
    __syncthreads();
    // third level (round 6): the sixteenths of quarters that were sixteenths last launch too and lasted at least `tier` run as four
    // single pixels -- one lane, the floor of a pixel's sample chain -- under the same condition (the launch ends on its longest
    // part while wavefront slots are idle) and out of what room the second level left
    uint32_t have3 = 0u, want3 = 0u;
    if (keep) for (uint32_t j = t; j < 16u * K; j += 1024u) {
        const uint32_t cs = sixt[j];
        if (cs == 0u) continue;
        if (cs == 0xFFFFFFFFu) have3++;
        else if (cs >= tier) want3++;
    }
    s_k[t] = have3; s_q[t] = want3;
    __syncthreads();
    for (uint32_t off = 512u; off > 0u; off >>= 1) { if (t < off) { s_k[t] += s_k[t + off]; s_q[t] += s_q[t + off]; } __syncthreads(); }
    const uint32_t room3 = room - 12u * K2;
    uint32_t K3 = s_k[0] + s_q[0], tier3 = tier, keep3 = 1u;
    if (3u * K3 > room3) { K3 = s_k[0]; tier3 = 0xFFFFFFFFu; }
    if (3u * K3 > room3) { K3 = 0u; keep3 = 0u; }
    if (t == 0) {
        plan[0] = K; plan[3] = use_tier; plan[4] = K2; plan[7] = keep;
        plan[5] = 0u;                                                  // k_build_launch's cursor into the part region
        plan[6] = K;
        plan[8] = tier3; plan[9] = K3; plan[10] = keep3;
        plan[1] = entries1 + 12u * K2 + 3u * K3;
    }
    // the part region is sized for more parts than k_build_launch may make: entries it does not claim name no pixels
    for (uint32_t j = t; j < 4u * K + 12u * K2 + 3u * K3; j += 1024u) launch[j] = kLaunchIndexMask;
}
// the launch list of a plan: first the parts of ranks 0 .. K-1 (the longest blocks: quarters, or sixteenths of the quarters
// the second level picked), then the other blocks whole, longest first.  The parts take their places with an atomic cursor
// (any order will do among them: they all start in the first round of wavefronts); a part region sized for more sixteenths
// than were made is padded with entries that name no pixels.
__global__ void __launch_bounds__(256) k_build_launch(const uint32_t* keys, const uint32_t* vals, uint32_t* cost, uint32_t n, uint32_t* plan,
                                                      uint32_t* launch, uint32_t* split, uint32_t* whole, uint32_t* qsplit, uint32_t* qwhole, uint32_t* swhole, const bool filtered) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t K = plan[0], tier = plan[3], keep = plan[7], tier3 = plan[8], keep3 = plan[10], i = vals[r];
    const uint32_t region = 4u * K + 12u * plan[4] + 3u * plan[9];
    if (r < K) {
        const bool was_split = split[i] != 0u;
        uint32_t codes[64], n_parts = 0u;          // per quarter: 1 entry, or per sixteenth 1 or 4
        uint32_t* c = cost + (size_t)i * kCostSlots;
        for (uint32_t q = 0; q < 4u; ++q) {
            bool again = false;
            const uint32_t m = was_split ? qsplit[4u * i + q] : 0u;
            const bool was = (m & 1u) != 0u;
            if (was_split) {
                const uint32_t cq = was ? qwhole[4u * i + q] : c[q];
                again = was ? keep != 0u : cq >= tier;
                if (again && !was) {
                    qwhole[4u * i + q] = max(1u, cq);
                    if (filtered) for (uint32_t s4 = 0; s4 < 4u; ++s4) c[4u + 4u * q + s4] = 0u;   // nothing known yet
                } else if (!again && was && filtered) c[q] = qwhole[4u * i + q];    // back to one quarter: what it took as one
            }
            uint32_t mnew = again ? 1u : 0u;
            if (!again) { codes[n_parts++] = 1u + q; qsplit[4u * i + q] = 0u; continue; }
            for (uint32_t s4 = 0; s4 < 4u; ++s4) {
                // a sixteenth goes on to pixels only once it has been MEASURED as a sixteenth (its quarter ran as sixteenths before)
                const uint32_t at16 = 16u * i + 4u * q + s4;
                const bool was3 = was && ((m >> (kPixelBit + s4)) & 1u);
                bool again3 = false;
                if (was) {
                    const uint32_t cs = was3 ? swhole[at16] : c[4u + 4u * q + s4];
                    again3 = was3 ? keep3 != 0u : cs >= tier3;
                    if (again3 && !was3) {
                        swhole[at16] = max(1u, cs);
                        if (filtered) for (uint32_t p4 = 0; p4 < 4u; ++p4) c[20u + 16u * q + 4u * s4 + p4] = 0u;
                    } else if (!again3 && was3 && filtered) c[4u + 4u * q + s4] = swhole[at16];     // back to one sixteenth
                }
                if (again3) { mnew |= 1u << (kPixelBit + s4); for (uint32_t p4 = 0; p4 < 4u; ++p4) codes[n_parts++] = 21u + 16u * q + 4u * s4 + p4; }
                else codes[n_parts++] = 5u + 4u * q + s4;
            }
            qsplit[4u * i + q] = mnew;
        }
        const uint32_t at = atomicAdd(&plan[5], n_parts);
        for (uint32_t j = 0; j < n_parts; ++j) if (at + j < region) launch[at + j] = i | (codes[j] << kLaunchCodeShift);
        if (!was_split) {
            whole[i] = max(1u, 0xFFFFFFu - keys[r]);     // what it cost as one block, for as long as it runs in parts
            if (filtered) for (uint32_t k = 0; k < 4u; ++k) c[k] = 0u;               // the quarters: nothing known yet
        }
        split[i] = 1u;
    } else {
        launch[region + (r - K)] = i;
        if (filtered && split[i]) cost[(size_t)i * kCostSlots] = whole[i];                                       // back to one block: slot 0 was its first quarter's
        split[i] = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) qsplit[4u * i + q] = 0u;
    }
}
// every block as four quarters (a first launch of few blocks: nothing is known about their costs yet)
__global__ void __launch_bounds__(256) k_build_launch_all_quarters(uint32_t n, uint32_t* plan, uint32_t* launch, uint32_t* split, uint32_t* whole, uint32_t* qsplit) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) { plan[0] = n; plan[1] = 4u * n; plan[2] = 0u; plan[3] = 0xFFFFFFFFu; plan[4] = 0u; plan[5] = 4u * n; plan[6] = 0xFFFFFFFFu; plan[7] = 1u;
                  plan[8] = 0xFFFFFFFFu; plan[9] = 0u; plan[10] = 1u; }
    if (i >= n) return;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) { launch[4u * i + j] = i | ((j + 1u) << kLaunchCodeShift); qsplit[4u * i + j] = 0u; }
    split[i] = 1u;
    whole[i] = 0u;            // never measured as one block: k_order_keys estimates it from the slowest quarter
}

// A tile mask that only clears tiles (trc_set_tile_mask, trc_render_adaptive): the new block list is the old one without the blocks of the
// cleared tiles, in the same order, so what is known about the surviving blocks moves from old list index i to new index j = the kept
// blocks before i.  One workgroup: thread t owns old indices [t * per, (t + 1) * per).  (1) every block's cost as ONE block -- k_order_keys'
// `c`, taken from the raw durations and from the filtered costs alike -- into `tmp` (2 n words: the sort's key buffers, idle between launches),
// and the kept flags counted; (2) the exclusive prefix sum of the counts; (3) slot 0 of the new index takes the cost, the split state of the
// whole list is zeroed (every block whole: the other slots are written before they are read again, k_build_launch).  Reads of step 1 and
// writes of step 3 are a barrier apart, so the arrays are compacted in place.
__global__ void __launch_bounds__(1024) k_compact_costs(const uint32_t* tiles, const uint8_t* mask, uint32_t tiles_x, uint32_t blk_shift, uint32_t n,
                                                        uint32_t stride, uint32_t* raw, uint32_t* est, uint32_t* split, uint32_t* whole, uint32_t* qsplit,
                                                        uint32_t* tmp_raw, uint32_t* tmp_est) {
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
    auto kept = [&](uint32_t i) {
        const uint32_t b = tiles[i], tx = ((b & 0xFFFFu) << blk_shift) / TRC_TILE, ty = ((b >> 16) << blk_shift) / TRC_TILE;
        return mask[(size_t)ty * tiles_x + tx] != 0;
    };
    auto as_one = [&](const uint32_t* cost, uint32_t i) {
        uint32_t c = cost[(size_t)i * stride];
        if (stride == kCostSlots && split[i])
            c = whole[i] ? whole[i] : (uint32_t)((float)slowest_part(cost, qsplit, i) * (1.0f / kQuarterEstimate));
        return c;
    };
    uint32_t count = 0u;
    for (uint32_t i = lo; i < hi; ++i) {
        tmp_raw[i] = as_one(raw, i); tmp_est[i] = as_one(est, i);
        if (kept(i)) count++;
    }
    // exclusive prefix sum of `count` over the workgroup
    const uint32_t lane = t & 63u, wave = t >> 6;
    uint32_t inc = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc += o; }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();                       // ... and every read of step 1 is done
    uint32_t j = inc - count;
    for (uint32_t w = 0; w < wave; ++w) j += s_wave[w];
    for (uint32_t i = lo; i < hi; ++i) {
        if (!kept(i)) continue;
        raw[(size_t)j * stride] = tmp_raw[i]; est[(size_t)j * stride] = tmp_est[i];
        ++j;
    }
    if (stride == kCostSlots)
        for (uint32_t i = lo; i < hi; ++i) {
            split[i] = 0u; whole[i] = 0u;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) qsplit[4u * i + q] = 0u;
        }
}

namespace {

constexpr bool kAutoSmallBlocks = true;       // decided by measurement (tools/small_blocks_bench.py, tile_balance.py); DESIGN.md section 5

// tiles owned by `rank` of `nranks`, in row-major order.  Workgroups are dealt to the 8 XCDs round-robin
// (blockIdx % 8), so neighbouring tiles -- similar cost: the same object fills them -- land on different XCDs and
// every XCD receives the same mix.  Measured: handing each XCD a contiguous band of the image instead (the
// "L2-friendly" order) costs 22 % on the Cornell scene and 44 % on the 1 M-triangle scene, because the XCD whose
// band holds the glass / mesh pixels finishes long after the others; 8x8-tile blocks per XCD sit in between.
// `mask` (trc_set_tile_mask; null: every tile): one byte per tile of the frame, row-major; of the owned blocks those of tiles with a non-zero
// byte stay, in the order they have in the unmasked list
std::vector<uint32_t> make_tiles(uint32_t W, uint32_t H, uint32_t nranks, uint32_t rank, uint32_t view_height, uint32_t blk_shift, const uint8_t* mask) {
    // ownership is decided per TRC_TILE x TRC_TILE tile; the launch unit is the pixel block of one wavefront:
    // 8x8 (blk_shift 3) or, for launches with too few blocks to fill the GPU, 4x4 on 16 lanes (blk_shift 2)
    const uint32_t e = 1u << blk_shift;
    const uint32_t bw = (W + e - 1) / e, bh = (H + e - 1) / e;
    const uint32_t tiles_x = (W + TRC_TILE - 1) / TRC_TILE;
    std::vector<uint32_t> mine;
    for (uint32_t by = 0; by < bh; ++by)
        for (uint32_t bx = 0; bx < bw; ++bx)
            if ((bx * e / TRC_TILE + by * e / TRC_TILE) % nranks == rank && (!mask || mask[(size_t)(by * e / TRC_TILE) * tiles_x + bx * e / TRC_TILE]))
                mine.push_back(bx | (by << 16));
    if (view_height != 0 && view_height < H) {
        // stacked views: walk the rows of ALL views together (row within the view first), so the launch ends on the
        // last rows of every view like a single-view launch does.  View after view, the expensive blocks of the final
        // view would start a few ms before the end of the list and run on alone (measured 28-31 ms instead of 25).
        std::stable_sort(mine.begin(), mine.end(), [&](uint32_t a, uint32_t b) {
            const uint32_t ra = ((a >> 16) * e) % view_height / e, rb = ((b >> 16) * e) % view_height / e;
            return ra < rb;
        });
    }
    return mine;
}

}  // namespace

// the block list and everything sized by it, freed and nulled; the cache key goes with them (trc_ensure_tiles, trc_release_frame).
// d_last_order / d_stale_order point into d_order_vals: whoever calls this rebuilds the list (trc_ensure_tiles forgets them) before a launch
void trc_release_tiles(trc_ctx* ctx) {
    ctx->tiles_nranks = 0;
    (void)hipFree(ctx->d_tiles); ctx->d_tiles = nullptr;
    (void)hipFree(ctx->d_block_cost); ctx->d_block_cost = nullptr;
    for (int k = 0; k < 2; ++k) { (void)hipFree(ctx->d_order_keys[k]); (void)hipFree(ctx->d_order_vals[k]); ctx->d_order_keys[k] = ctx->d_order_vals[k] = nullptr; }
    (void)hipFree(ctx->d_order_hist); ctx->d_order_hist = nullptr;
    (void)hipFree(ctx->d_split); ctx->d_split = nullptr;
    (void)hipFree(ctx->d_whole); ctx->d_whole = nullptr;
    (void)hipFree(ctx->d_cost_est); ctx->d_cost_est = nullptr;
    (void)hipFree(ctx->d_qsplit); ctx->d_qsplit = nullptr;
    (void)hipFree(ctx->d_qwhole); ctx->d_qwhole = nullptr;
    (void)hipFree(ctx->d_swhole); ctx->d_swhole = nullptr;
    (void)hipFree(ctx->d_launch); ctx->d_launch = nullptr;
    (void)hipFree(ctx->d_plan_gather); ctx->d_plan_gather = nullptr;
    (void)hipFree(ctx->d_cost_scratch); ctx->d_cost_scratch = nullptr;
}

trc_status trc_ensure_tiles(trc_ctx* ctx, uint32_t nranks, uint32_t rank, uint32_t view_height, uint32_t blk_shift, bool masked) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const uint64_t mask_gen = masked ? ad.mask_gen : 0u;
    if (ctx->d_tiles && ctx->d_block_cost && ctx->tiles_nranks == nranks && ctx->tiles_rank == rank &&
        ctx->tiles_view_height == view_height && ctx->tiles_blk_shift == blk_shift && ctx->tiles_mask_gen == mask_gen) return TRC_OK;
    const uint8_t* mask = mask_gen ? ad.tile_mask.data() : nullptr;
    std::vector<uint32_t> tiles = make_tiles(ctx->width, ctx->height, nranks, rank, view_height, blk_shift, mask);
    if (tiles.size() > (size_t)kLaunchIndexMask) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "frame too large: more pixel blocks than a launch-list entry can name");
    // The list of a mask that only cleared tiles of the list before it (shrinks_from: trc_adopt_tile_mask compared the two masks): the
    // allocations stay, they are large enough, and so do the costs of the surviving blocks (k_compact_costs), so the next launch is ordered by
    // them as one pass -- not a cold head + rest, which a driver that clears tiles every round would pay every round.  Costs per strip
    // (cost_strip > 1) name no block; knob mask_forgets_costs: every mask change starts a new list as below.
    if (ctx->d_tiles && ctx->d_block_cost && ctx->tiles_nranks == nranks && ctx->tiles_rank == rank && ctx->tiles_view_height == view_height &&
        ctx->tiles_blk_shift == blk_shift && mask && ad.shrinks_from == ctx->tiles_mask_gen && !ctx->knobs.mask_forgets_costs && ad.d_mask && ad.mask_on_device) {
        const bool carry = ctx->cost_valid && ctx->cost_strip == 1 && ctx->n_tiles != 0 && !tiles.empty();
        if (carry) {
            hipLaunchKernelGGL(k_compact_costs, dim3(1), dim3(1024), 0, ctx->stream, ctx->d_tiles, ad.d_mask, trc_tiles_x(ctx), blk_shift, ctx->n_tiles,
                               ctx->cost_quarters ? kCostSlots : 1u, ctx->d_block_cost, ctx->d_cost_est, ctx->d_split, ctx->d_whole, ctx->d_qsplit,
                               ctx->d_order_keys[0], ctx->d_order_keys[1]);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_plan, 0, kPlanWords * sizeof(uint32_t), ctx->stream));
            ctx->split_live = false;
        } else trc_forget_costs(ctx);
        ctx->plan_streak = 0; ctx->d_last_order = nullptr; ctx->d_stale_order = nullptr;
        ctx->tiles_nranks = 0;               // (the key is whole again once the list is in place)
        TRC_TRY(trc_copy_to_device(ctx, ctx->d_tiles, tiles.data(), tiles.size() * 4, ctx->stream));      // behind the kernel, which reads the old list
        ctx->n_tiles = (uint32_t)tiles.size();
        ctx->tiles_nranks = nranks; ctx->tiles_mask_gen = mask_gen;
        return TRC_OK;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the cache key (tiles_nranks ...) is written LAST: a failed allocation below leaves the list invalid, so the next
    // call rebuilds it instead of launching with a null block_cost / order buffer
    trc_release_tiles(ctx);
    ctx->plan_streak = 0;
    trc_forget_costs(ctx); ctx->cost_quarters = false; ctx->launch_cap = 0;
    ctx->n_tiles = (uint32_t)tiles.size();
    if (ctx->n_tiles) {
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_tiles, tiles.size() * 4));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_block_cost, tiles.size() * 4 * kCostSlots));      // per block: whole / quarters / sixteenths
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_split, tiles.size() * 4));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_whole, tiles.size() * 4));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cost_est, tiles.size() * 4 * kCostSlots));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_qsplit, tiles.size() * 16));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_qwhole, tiles.size() * 16));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_swhole, tiles.size() * 64));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_launch, tiles.size() * 4 * kCostSlots));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_plan_gather, tiles.size() * 4 * 22));     // k_plan_gather: part, raw, 4 quarters, 16 sixteenths per rank
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cost_scratch, tiles.size() * 4 * kCostSlots));   // where instrumented launches leave their durations      // k_plan_gather: part, raw, 4 quarters per rank
        if (!ctx->d_plan) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_plan, kPlanWords * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_plan, 0, kPlanWords * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_split, 0, tiles.size() * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_qsplit, 0, tiles.size() * 16, ctx->stream));
        ctx->launch_cap = (uint32_t)tiles.size() * kCostSlots;
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_order_keys[k], tiles.size() * 4));
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_order_vals[k], tiles.size() * 4));
        }
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_order_hist, (trc_sort_hist_words(ctx->n_tiles) + 256) * 4));
        TRC_TRY(trc_copy_to_device(ctx, ctx->d_tiles, tiles.data(), tiles.size() * 4, ctx->stream));
    }
    ctx->tiles_nranks = nranks; ctx->tiles_rank = rank; ctx->tiles_view_height = view_height; ctx->tiles_blk_shift = blk_shift; ctx->tiles_mask_gen = mask_gen;
    return TRC_OK;
}

// Durations recorded for another strip length, block size or integrator say nothing about this launch's list
void drop_stale_costs(trc_ctx* ctx, const trc_params* p, const RenderLaunch& r) {
    if (r.stats) return;
    if (ctx->cost_strip != r.kp.strip || ctx->cost_quarters != r.quarters_ok) {
        trc_forget_costs(ctx); ctx->cost_strip = r.kp.strip; ctx->cost_quarters = r.quarters_ok;
    }
    if (ctx->cost_integrator != p->integrator || ctx->cost_light != r.light || ctx->cost_rays != r.rays || ctx->cost_params != r.params) {
        trc_forget_costs(ctx); ctx->cost_integrator = p->integrator; ctx->cost_light = r.light; ctx->cost_rays = r.rays; ctx->cost_params = r.params;
    }
}

// Block schedule.  (1) Order: most expensive blocks of the previous launch first (longest-processing-time order; cost = the
// wavefront's measured duration): a block's samples are a sequential chain, so whatever starts last decides how long
// the GPU drains.  Measured: config 2 25.2 -> 22.3 ms (ray counts as the key: 23.7), the 1 M-triangle scene 18.7 ->
// 16.8 ms.  (2) Cost-adaptive block size (k_plan_split): the blocks that would decide the launch run as four 4x4
// quarters.  Pixels depend on neither.
constexpr uint32_t kPlanSettled = 8, kPlanReuse = 3;   // a settled list re-plans every fourth launch
trc_status schedule_blocks(trc_ctx* ctx, const trc_params* p, RenderLaunch& r) {
    KRender& kp = r.kp;
    const bool stats = r.stats;
    const uint32_t wave_slots = r.wave_slots;
    const bool may_split = r.quarters_ok && !stats && p->spp >= 8 && !ctx->knobs.no_split &&
                           !(p->flags & (TRC_FLAG_LARGE_BLOCKS | TRC_FLAG_FIXED_ORDER));
    if (!stats) { ctx->last_cost_div = kp.cost_div; ctx->last_wave_slots = wave_slots; }
    if (stats) {} else if (!ctx->cost_valid || (p->flags & TRC_FLAG_FIXED_ORDER) || kp.strip > 1) ctx->plan_streak = 0;      // nothing settled to reuse
    r.grid_cap = ctx->n_tiles;
    r.planned = false;
    if (stats) {
        // row-major, every block whole, nothing recorded
    } else if (ctx->cost_valid && !(p->flags & TRC_FLAG_FIXED_ORDER) && kp.strip > 1 && ctx->d_last_order && ctx->order_age < 4) {
        kp.order = ctx->d_last_order;              // short launches: the order of a few launches ago is as good, and 13 tiny
        ctx->order_age++;                          // sort launches per 0.7 ms render are not
    } else if (ctx->cost_valid && !(p->flags & TRC_FLAG_FIXED_ORDER)) {
        const uint32_t n = (ctx->n_tiles + kp.strip - 1) / kp.strip;
        // the costs the order and the plan work on: the shortest durations seen lately (filter_block_costs), or the last launch's
        const bool filtered = !ctx->knobs.no_cost_filter;
        uint32_t* costs = filtered ? ctx->d_cost_est : ctx->d_block_cost;
        // A list whose plan has settled (kPlanSettled planned launches in a row) keeps its order and plan for kPlanReuse
        // launches: the filtered costs of a progressive render barely move from one launch to the next, and the dozen small
        // kernels below are 0.1 ms in front of every launch (schedule_ms in trc_stats) -- 2 % of an eighth of a frame.  The
        // launch that is reused ran with the same list, so the durations it leaves land in the same slots.
        const bool reuse = ctx->plan_streak >= kPlanSettled && ctx->plan_reused < kPlanReuse && ctx->plan_n == n && ctx->plan_split_mode == may_split &&
                           ctx->plan_wave_slots == wave_slots && !ctx->knobs.no_plan_reuse;
        if (reuse) {
            ctx->plan_reused++;
            if (may_split) { kp.order = ctx->d_launch; kp.n_launch = ctx->d_plan + 1; r.grid_cap = ctx->plan_grid_cap; r.planned = true; }
            else kp.order = ctx->d_last_order;
        } else {
        hipEvent_t s0 = trc_get_event(ctx), s1 = trc_get_event(ctx);
        if (s0) (void)hipEventRecord(s0, ctx->stream);
        hipLaunchKernelGGL(k_order_keys, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_block_cost, costs, ctx->d_split, ctx->d_whole, ctx->d_qsplit,
                           kp.cost_stride, n, ctx->d_order_keys[0], ctx->d_order_vals[0], filtered, ctx->cost_head_age == 2 || ctx->cost_fresh_next);
        ctx->cost_fresh_next = false;
        int res = 0;
        trc_sort_pairs24(ctx->stream, ctx->d_order_keys, ctx->d_order_vals, ctx->d_order_hist, ctx->d_order_hist + trc_sort_hist_words(n), n, &res);
        kp.order = ctx->d_order_vals[res];
        ctx->d_last_order = kp.order;
        ctx->order_age = 0;
        if (may_split) {
            // the grid is sized before the plan is known: half the slots' worth of split blocks is more than any plan has
            // taken (a launch with fewer blocks than slots is capped to the slots anyway), + an eighth for sixteenths
            const uint32_t k_max = std::min(n, wave_slots / 2u);
            const uint32_t max_entries = std::min(ctx->launch_cap, std::max(n + 3u * k_max, wave_slots) + wave_slots / 8u);
            uint32_t* g_part = ctx->d_plan_gather;
            float* g_raw = reinterpret_cast<float*>(ctx->d_plan_gather + n);
            uint32_t* g_quart = ctx->d_plan_gather + 2 * (size_t)n;
            uint32_t* g_sixt = ctx->d_plan_gather + 6 * (size_t)n;
            hipLaunchKernelGGL(k_plan_gather, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_order_vals[res], ctx->d_split, costs, ctx->d_qsplit,
                               ctx->d_block_cost, n, g_part, g_raw, g_quart, g_sixt);
            hipLaunchKernelGGL(k_plan_split, dim3(1), dim3(1024), 0, ctx->stream, ctx->d_order_keys[res], g_part, g_raw, g_quart, g_sixt, n, k_max, wave_slots,
                               max_entries, ctx->d_plan, ctx->d_launch);
            hipLaunchKernelGGL(k_build_launch, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_order_keys[res], ctx->d_order_vals[res], costs, n,
                               ctx->d_plan, ctx->d_launch, ctx->d_split, ctx->d_whole, ctx->d_qsplit, ctx->d_qwhole, ctx->d_swhole, filtered);
            kp.order = ctx->d_launch;
            kp.n_launch = ctx->d_plan + 1;
            r.grid_cap = max_entries;
            r.planned = true;
        }
        if (s0 && s1 && hipEventRecord(s1, ctx->stream) == hipSuccess) ctx->pending_sched.emplace_back(s0, s1);
        else { if (s0) ctx->event_pool.push_back(s0); if (s1) ctx->event_pool.push_back(s1); }
        ctx->plan_streak = (ctx->plan_n == n && ctx->plan_split_mode == may_split && ctx->plan_wave_slots == wave_slots) ? ctx->plan_streak + 1 : 1;
        ctx->plan_reused = 0; ctx->plan_n = n; ctx->plan_split_mode = may_split; ctx->plan_wave_slots = wave_slots; ctx->plan_grid_cap = r.grid_cap;
        }
    } else if (may_split && !ctx->cost_valid && kAutoSmallBlocks && r.fits && r.blocks8 <= (uint64_t)ctx->cu_count * 16u &&
               p->integrator == TRC_INTEGRATOR_PATH && ctx->lds_scene) {
        // nothing is known about the blocks yet and there are no more of them than wavefront slots (a small frame, or an
        // eighth of a 1080p frame): every block as quarters -- measured on whole small frames at 64 spp (920 / 2 040 / 3 600
        // blocks: 8.5 / 8.3 / 8.9 -> 7.0 / 7.2 / 7.4 ms); from the second launch on the plan decides block by block
        hipLaunchKernelGGL(k_build_launch_all_quarters, dim3((ctx->n_tiles + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_tiles, ctx->d_plan, ctx->d_launch, ctx->d_split, ctx->d_whole, ctx->d_qsplit);
        kp.order = ctx->d_launch;
        kp.n_launch = ctx->d_plan + 1;
        r.grid_cap = 4u * ctx->n_tiles;
        r.planned = true;
    }
    if (!stats && !ctx->cost_valid && !r.planned && !kp.order && ctx->d_stale_order && kp.strip == 1 && !(p->flags & TRC_FLAG_FIXED_ORDER))
        kp.order = ctx->d_stale_order;              // a cold pass after a camera move: the previous view's order beats row-major
    if (!stats) ctx->d_stale_order = nullptr;       // (the buffer belongs to the next sort)
    if (!stats && !r.planned && ctx->split_live) {                        // this launch runs every block whole
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_split, 0, (size_t)ctx->n_tiles * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_qsplit, 0, (size_t)ctx->n_tiles * 16, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_cost_est, 0, (size_t)ctx->n_tiles * 4 * kCostSlots, ctx->stream));   // slot 0 held first quarters
    }
    if (!stats) ctx->split_live = r.planned;
    if (!stats && !ctx->cost_valid) HIP_TRY(ctx, hipMemsetAsync(ctx->d_cost_est, 0, (size_t)ctx->n_tiles * 4 * kCostSlots, ctx->stream));
    if (!stats) {
        ctx->cost_head_age = (ctx->cost_valid && ctx->cost_head_age == 1) ? 2 : 0;     // head -> the launch on its costs -> settled
        ctx->cost_valid = true;
    }
    return TRC_OK;
}

extern "C" {
// developer diagnostic: the pixel blocks of the last trc_render (x | y << 16 in units of the block edge) and the duration
// each one's wavefront measured per sample (shader clocks / (4 spp), the adaptive order's sort key)
trc_status trc_debug_block_costs(trc_ctx* ctx, uint32_t* tiles, uint32_t* costs, uint32_t capacity, uint32_t* n_blocks, uint32_t* blk_shift) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_blocks) *n_blocks = ctx->n_tiles;
    if (blk_shift) *blk_shift = ctx->tiles_blk_shift;
    const uint32_t n = std::min(capacity, ctx->n_tiles);
    if (n == 0 || !ctx->d_tiles) return TRC_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (tiles) TRC_TRY(trc_copy_to_host(ctx, tiles, ctx->d_tiles, (size_t)n * 4, ctx->stream));
    if (costs) {
        const uint32_t stride = ctx->cost_quarters ? kCostSlots : 1u;
        std::vector<uint32_t> c((size_t)n * stride), sp(n, 0u), qs((size_t)n * 4u, 0u);
        TRC_TRY(trc_copy_to_host(ctx, c.data(), ctx->d_block_cost, c.size() * 4, ctx->stream));
        if (stride != 1u) {
            TRC_TRY(trc_copy_to_host(ctx, sp.data(), ctx->d_split, (size_t)n * 4, ctx->stream));
            TRC_TRY(trc_copy_to_host(ctx, qs.data(), ctx->d_qsplit, (size_t)n * 16, ctx->stream));
        }
        for (uint32_t i = 0; i < n; ++i) {        // a block that ran in parts: its slowest part, bit 31 set (bit 30: some of them 2x2)
            const uint32_t* q = &c[(size_t)i * stride];
            if (!sp[i]) { costs[i] = q[0]; continue; }
            uint32_t m = 0u, deep = 0u;      // bit 30: some of its quarters ran as 2x2 sixteenths; bit 29: some of those as single pixels
            for_each_part(qs.data(), i, [&](uint32_t slot) { m = std::max(m, q[slot]); if (slot >= 4u) deep |= 0x40000000u; if (slot >= 20u) deep |= 0x20000000u; });
            costs[i] = std::min(m, 0xFFFFFFu) | 0x80000000u | deep;
        }
    }
    return TRC_OK;
}

}  // extern "C"
