// trc_render_lds_mis.hip -- traceMIS and traceVolume on scenes whose whole tree is staged in LDS (default compiler options; tracePath's
// kernels of the same scenes are in trc_render_lds.hip).  Definitions: trc_render_kernels.hpp; launched from trc_abi.hip.
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#include "trc_render_kernels.hpp"

// the kernel tables (trc_render_config.hpp)
const RenderKernels render_lds_mis = render_kernels<true, TRC_INTEGRATOR_MIS>();
const RenderKernels render_lds_volume = render_kernels<true, TRC_INTEGRATOR_VOLUME>();
