// trc_render_params.hip -- the kernels of TRC_FLAG_MATERIAL_PARAMS (trc_render_params.hpp: a lobe's parameters are read from the context's
// table) on scenes whose whole tree is staged in LDS, tracePath and traceMIS, without and with image textures, compiled with the source
// options of the units they shadow (trc_render_lds.hip, trc_render_lds_mis.hip).  Trees read from memory: trc_render_params_mem.hip.
// Launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twin reading per-triangle materials: trc_render_params_tm.hip
#endif
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#ifndef TRC_MICROFACET_STREAM
#define TRC_MICROFACET_STREAM 1      // dev_bsdf.hpp (the parametrised lobes are the stream form whatever this says)
#endif
#ifndef TRC_SAMPLE11_ONCE
#define TRC_SAMPLE11_ONCE 7          // dev_bsdf.hpp: Beckmann's sample11 evaluates each exp, log and erf_inv once (profiles/r31)
#endif
#include "trc_render_params.hpp"

TRC_RENDER_NS_BEGIN
// the kernel table (trc_render_config.hpp)
const RenderParamsKernels render_params_lds = render_params_kernels<true>();
TRC_RENDER_NS_END
