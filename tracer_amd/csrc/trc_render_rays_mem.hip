// trc_render_rays_mem.hip -- the kernels of TRC_FLAG_CAMERA_RAYS (trc_render_rays.hpp) on trees read from memory (mesh scenes),
// tracePath, traceMIS and traceMIS under TRC_FLAG_ENV_LIGHT, without and with image textures, compiled with the source options of the units they shadow
// (trc_render_mem_path.hip, trc_render_mem.hip).  Trees staged in LDS: trc_render_rays.hip.  Launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twin reading per-triangle materials: trc_render_rays_mem_tm.hip
#endif
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#ifndef TRC_WALK_TRIM
#define TRC_WALK_TRIM 0      // dev_intersect.hpp: trees read from memory keep the reference's forms (trc_render_mem.hip)
#endif
#include "trc_render_rays.hpp"

TRC_RENDER_NS_BEGIN
// the kernel table (trc_render_config.hpp)
const RenderRaysKernels render_rays_mem = render_rays_kernels<false>();
TRC_RENDER_NS_END
