// trc_render_mem_path.hip -- tracePath on trees read from memory (BASELINE config 4 and every mesh scene under the default integrator):
// one-wavefront workgroups, strips and the persistent workgroups, at 7 waves per SIMD (trc_render_config.hpp).  Its own translation
// unit because it is compiled with -mllvm -disable-machine-sink (Makefile: EXTRA_trc_render_mem_path): machine sinking moves
// computations into the branches behind the traversal loop and with them their operands' live ranges across it -- without it config 4 runs
// 22.90 -> 22.55 ms per 32-spp launch and the scene beyond the Infinity Cache 18.29 -> 17.16, while traceMIS loses 1.5 % and keeps the
// default (profiles/r05/ab_flags*.txt).  Same instructions' results either way: scheduling.  Definitions: trc_render_kernels.hpp.
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
const RenderKernels render_mem_path = render_kernels<false, TRC_INTEGRATOR_PATH>();
TRC_RENDER_NS_END
