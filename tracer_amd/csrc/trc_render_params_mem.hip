// trc_render_params_mem.hip -- the kernels of TRC_FLAG_MATERIAL_PARAMS (trc_render_params.hpp) on trees read from memory (mesh scenes),
// tracePath and traceMIS, without and with image textures, compiled with the source options of the units they shadow
// (trc_render_mem_path.hip, trc_render_mem.hip).  Trees staged in LDS: trc_render_params.hip.  Launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twin reading per-triangle materials: trc_render_params_mem_tm.hip
#endif
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#ifndef TRC_WALK_TRIM
#define TRC_WALK_TRIM 0      // dev_intersect.hpp: trees read from memory keep the reference's forms (trc_render_mem.hip)
#endif
#include "trc_render_params.hpp"

TRC_RENDER_NS_BEGIN
// the kernel table (trc_render_config.hpp)
const RenderParamsKernels render_params_mem = render_params_kernels<false>();
TRC_RENDER_NS_END
