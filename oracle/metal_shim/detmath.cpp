// detmath.cpp -- the elementary functions of metal_stdlib (the stand-in beside this file): include/trc_detmath.h, the ones
// the oracle and the kernels use.  A translation unit of its own because trc_detmath.h needs <math.h>, whose global sqrt / abs /
// isinf / gamma would collide with the names <metal_stdlib> and the reference's Math.hh declare.
#include "trc_detmath.h"

extern "C" {
float refm_sinf(float x) { return dm_sinf(x); }
float refm_cosf(float x) { return dm_cosf(x); }
float refm_expf(float x) { return dm_expf(x); }
float refm_logf(float x) { return dm_logf(x); }
float refm_powf(float x, float y) { return dm_powf(x, y); }
float refm_asinf(float x) { return dm_asinf(x); }
float refm_acosf(float x) { return dm_acosf(x); }
float refm_atan2f(float y, float x) { return dm_atan2f(y, x); }
}
