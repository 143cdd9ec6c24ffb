// trc_render_mem.hip -- the render kernels of trees read from memory (mesh scenes) for traceMIS (BASELINE config 3): one-wavefront
// workgroups, strips and the persistent workgroups.  tracePath's are in trc_render_mem_path.hip and traceVolume's in
// trc_render_mem_volume.hip, translation units of their own since round 5 because the families want different compiler options
// (Makefile: EXTRA_*; this one keeps the defaults: -disable-machine-sink costs traceMIS 1.5 %).  Compiled WITH dev_vec.hpp's guard-free forms since their guards became one or two instructions
// (profiles/r04/guard_cost_ab.txt).  Definitions: trc_render_kernels.hpp; launched from trc_render_pass.hip.
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
const RenderKernels render_mem_mis = render_kernels<false, TRC_INTEGRATOR_MIS>();
TRC_RENDER_NS_END
