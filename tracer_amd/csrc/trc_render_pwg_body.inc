// trc_render_pwg_body.inc -- the body of k_render_pwg / _tex / _env / _mesh, included as the body of each kernel (trc_render_kernels.hpp)
// rather than called from a helper: every kernel keeps its code and its name, and the twins share the source.  (The strip body was tried as
// a function in round 12 and changed its kernels' code -- trc_render_strip_body.inc; this one stays a file with it.)
// Expects in scope: kp, INTEGRATOR, SOBOL, TEX, LIGHT and tables (that light's sampling tables, null for Light::None).
    const DScene& sc = kp.ks.sc;
    {
        const uint4* src = reinterpret_cast<const uint4*>(sc.blob);
        uint4* dst = reinterpret_cast<uint4*>(trc_smem);
        const uint32_t n16 = sc.lds_dwords >> 2;
        for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    constexpr bool kHybridStack = hybrid_stack(INTEGRATOR);
    constexpr uint32_t kRows = pwg_park_rows(INTEGRATOR);       // a wavefront's LDS: stack_lds stack rows, then the park rows (render_block)
    constexpr bool kPark = kRows != 0u;
    uint32_t* stack = trc_smem + sc.lds_dwords + wave * (sc.stack_lds + kRows) * kBlock + lane;
    uint32_t* park = stack + sc.stack_lds * kBlock;
    uint32_t* ovf = kHybridStack ? kp.stack_ovf + ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * sc.stack_ovf_rows * kBlock + lane : nullptr;
    // primary replay (render_block): MEMO rows per wavefront in global memory, this lane's column
    constexpr int kMemo = (!SOBOL && LIGHT == Light::None) ? (int)pwg_memo_rows(INTEGRATOR) : 0;
    uint32_t* memo = kMemo ? kp.memo + ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * kMemo * kBlock + lane : nullptr;
    uint32_t n_paths = 0;
    TravCounters cnt;
    counters_zero(cnt);
    const uint32_t n_entries = kp.n_launch ? *kp.n_launch : kp.n_tiles;
    uint32_t r_rays, r_shaded;
    if constexpr (kPark) {
        park[kParkRays * kBlock] = 0u; park[kParkShaded * kBlock] = 0u;
        LdsCount n_rays{park + kParkRays * kBlock}, n_shaded{park + kParkShaded * kBlock};
        for (;;) {
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(kp.queue, 1u);
            slot = __builtin_amdgcn_readfirstlane(slot);
            if (slot >= n_entries) break;
            render_block<false, false, INTEGRATOR, SOBOL, kHybridStack, (int)kRows, TEX, LIGHT, kMemo>(kp, sc, trc_smem, stack, nullptr, ovf, park, slot, lane, n_rays, n_shaded, n_paths, cnt, tables, memo);
        }
        r_rays = wave_sum(park[kParkRays * kBlock]); r_shaded = wave_sum(park[kParkShaded * kBlock]);
    } else {
        uint32_t n_rays = 0, n_shaded = 0;
        for (;;) {
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(kp.queue, 1u);
            slot = __builtin_amdgcn_readfirstlane(slot);
            if (slot >= n_entries) break;
            render_block<false, false, INTEGRATOR, SOBOL, kHybridStack, 0, TEX, LIGHT, kMemo>(kp, sc, trc_smem, stack, nullptr, ovf, nullptr, slot, lane, n_rays, n_shaded, n_paths, cnt, tables, memo);
        }
        r_rays = wave_sum(n_rays); r_shaded = wave_sum(n_shaded);
    }
    const uint32_t r_paths = wave_sum(n_paths);
    if (lane == 0) {
        unsigned long long* const stats = stat_row(kp.stats, blockIdx.x * (blockDim.x >> 6) + wave);
        atomicAdd(&stats[kStatPaths], (unsigned long long)r_paths);
        atomicAdd(&stats[kStatRays], (unsigned long long)r_rays);
        atomicAdd(&stats[kStatShaded], (unsigned long long)r_shaded);
    }
