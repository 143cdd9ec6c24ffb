// trc_render_lds.hip -- tracePath on scenes whose whole tree is staged in LDS (the Cornell scenes: BASELINE config 2 -- the bench's
// kernel), instantiated with the guard-free reciprocal / square root of dev_vec.hpp (TRC_FAST_UNARY, bit-identical:
// tests/test_gpu_unary.py).  traceMIS / traceVolume on such scenes: trc_render_lds_mis.hip -- two translation units since round 5
// because this one is compiled with -mllvm -amdgpu-use-amdgpu-trackers (Makefile: EXTRA_trc_render_lds; config 2 16.64 -> 16.50 ms,
// traceMIS on the same scene would lose 1.6 %: profiles/r05/ab_flags*.txt).  Definitions: trc_render_kernels.hpp; launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twins reading per-triangle materials: trc_render_*_tm.hip
#endif
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#ifndef TRC_MICROFACET_STREAM
#define TRC_MICROFACET_STREAM 1      // dev_bsdf.hpp: the Metal lobe through the Beckmann lobes' stream (profiles/r22)
#endif
#ifndef TRC_SAMPLE11_ONCE
#define TRC_SAMPLE11_ONCE 7          // dev_bsdf.hpp: Beckmann's sample11 evaluates each exp, log and erf_inv once (profiles/r31)
#endif
#include "trc_render_kernels.hpp"

TRC_RENDER_NS_BEGIN
// tracePath on an LDS-resident tree at one more wavefront per SIMD, for launch lists many times the wavefront slots (trc_render_config.hpp)
__global__ void __launch_bounds__(kBlock, TRC_PATH_WAVES_DENSE) k_render_dense(const KRender kp) {
    // + per-pixel state parked in LDS rows, the camera ray's hit memoised (render_block)
    render_workgroup<true, false, TRC_INTEGRATOR_PATH, false, TRC_PARK_DENSE, false, Light::None, TRC_REPLAY_DENSE, TRC_REPLAY_DENSE_GLOBAL != 0>(kp);
}

// the kernel table (trc_render_config.hpp); k_render_dense has no texture twin (a textured scene takes k_render_tex instead)
const RenderKernels render_lds_path = render_kernels<true, TRC_INTEGRATOR_PATH>();
const RenderKernel render_dense = render_kernel(&k_render_dense, TRC_PATH_WAVES_DENSE);
TRC_RENDER_NS_END
