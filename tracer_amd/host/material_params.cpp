// material_params.cpp -- the host side of TRC_FLAG_MATERIAL_PARAMS (tracer_abi.h: "Material parameters"): the reference's literals per
// material type, as its create*() functions write them (MicrofacetBXDF.h:438-455, 514-530, 576-586) and the unflagged kernels hold them.
#include <cstdint>

#include "tracer_abi.h"

extern "C" void trc_host_default_material_params(int32_t material_type, trc_material_params* out) {
    if (!out) return;
    trc_material_params p{};
    p.alpha_x = 0.01f; p.alpha_y = 0.1f; p.eta = 1.5f;             // Plastic's, and of every type that reads none of them
    if (material_type == TRC_MAT_GLASS) p.alpha_y = 0.01f;
    if (material_type == TRC_MAT_METAL) p.alpha_y = 0.02f;
    p.metal_eta[0] = 0.18f; p.metal_eta[1] = 0.15f; p.metal_eta[2] = 0.81f;
    p.metal_k[0] = p.metal_k[1] = p.metal_k[2] = 1.0f;
    *out = p;
}
