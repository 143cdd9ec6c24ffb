// trc_render_params_mem_tm.hip -- the kernels and table of trc_render_params_mem.hip that read each triangle's material (dev_intersect.hpp:
// TRC_TRIANGLE_MATERIALS), in namespace trimat; trc_render_pass.hip launches them only while per-triangle materials are set.
#define TRC_TRIANGLE_MATERIALS 1
#include "trc_render_params_mem.hip"
