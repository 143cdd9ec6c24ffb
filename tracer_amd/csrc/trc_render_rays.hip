// trc_render_rays.hip -- the kernels of TRC_FLAG_CAMERA_RAYS (trc_render_rays.hpp: a sample's camera ray is read from the context's ray
// sets) on scenes whose whole tree is staged in LDS, tracePath, traceMIS and traceMIS under TRC_FLAG_ENV_LIGHT, without and with image textures, compiled with the source
// options of the units they shadow (trc_render_lds.hip, trc_render_lds_mis.hip).  Trees read from memory: trc_render_rays_mem.hip.
// Launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twin reading per-triangle materials: trc_render_rays_tm.hip
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
#include "trc_render_rays.hpp"

TRC_RENDER_NS_BEGIN
// the kernel table (trc_render_config.hpp)
const RenderRaysKernels render_rays_lds = render_rays_kernels<true>();
TRC_RENDER_NS_END
