// trc_render_mem_volume.hip -- traceVolume on trees read from memory (the participating-media scene): one-wavefront workgroups, strips
// and the persistent workgroups.  Its own translation unit because it is compiled with -mllvm -disable-machine-sink like tracePath's
// (Makefile: EXTRA_trc_render_mem_volume; 35.97 -> 35.61 ms per 16-spp launch, profiles/r05/ab_flags_volume.txt), which traceMIS, its
// former neighbour in trc_render_mem.hip, does not want.  Definitions: trc_render_kernels.hpp; launched from trc_render_pass.hip.
#ifndef TRC_TRIANGLE_MATERIALS
#define TRC_TRIANGLE_MATERIALS 0      // triangles keep material 19; the twins reading per-triangle materials: trc_render_*_tm.hip
#endif
#ifndef TRC_FAST_UNARY
#define TRC_FAST_UNARY 1
#endif
#ifndef TRC_WALK_TRIM
#define TRC_WALK_TRIM 0      // dev_intersect.hpp: the short forms cost traceVolume 1.8 % on a tree read from memory and gain nothing here
#endif
#include "trc_render_kernels.hpp"

TRC_RENDER_NS_BEGIN
// the kernel table (trc_render_config.hpp)
const RenderKernels render_mem_volume = render_kernels<false, TRC_INTEGRATOR_VOLUME>();
TRC_RENDER_NS_END
