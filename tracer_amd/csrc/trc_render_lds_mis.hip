// trc_render_lds_mis.hip -- traceMIS and traceVolume on scenes whose whole tree is staged in LDS (default compiler options; tracePath's
// kernels of the same scenes are in trc_render_lds.hip).  Definitions: trc_render_kernels.hpp; launched from trc_render_pass.hip.
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
// the kernel tables (trc_render_config.hpp)
const RenderKernels render_lds_mis = render_kernels<true, TRC_INTEGRATOR_MIS>();
const RenderKernels render_lds_volume = render_kernels<true, TRC_INTEGRATOR_VOLUME>();
TRC_RENDER_NS_END
