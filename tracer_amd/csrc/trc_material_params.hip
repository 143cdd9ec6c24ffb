// trc_material_params.hip -- the table of TRC_FLAG_MATERIAL_PARAMS (tracer_abi.h): one trc_material_params per material of the scene,
// validated, uploaded, downloaded, dropped with the scene.  The kernels that read it: trc_render_params.hpp (the lobes: dev_bsdf.hpp);
// their choice: trc_render_pass.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "trc_ctx.hpp"

void trc_material_params_release(trc_ctx* ctx) {
    (void)hipFree(ctx->d_mparams); ctx->d_mparams = nullptr; ctx->n_mparams = 0;
    if (ctx->cost_params) trc_forget_costs(ctx);      // the recorded block costs were measured on this table
}

// nullptr: the record is acceptable.  Otherwise the reason.
static const char* params_check(const trc_material_params& m) {
    const float all[] = {m.alpha_x, m.alpha_y, m.eta, m.metal_eta[0], m.metal_eta[1], m.metal_eta[2], m.metal_k[0], m.metal_k[1], m.metal_k[2]};
    for (const float f : all)
        if (!std::isfinite(f)) return "a field is not finite";
    if (!(m.alpha_x > 0.0f) || !(m.alpha_y > 0.0f)) return "alpha_x or alpha_y <= 0";
    if (!(m.eta > 1.0f)) return "eta <= 1";
    for (int k = 0; k < 3; ++k)
        if (!(m.metal_eta[k] > 0.0f) || !(m.metal_k[k] > 0.0f)) return "a component of metal_eta or metal_k <= 0";
    return nullptr;
}

extern "C" {

trc_status trc_upload_material_params(trc_ctx* ctx, const trc_material_params* p, uint32_t n_material) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_upload_material_params before trc_upload_scene");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!p && n_material == 0) {                      // none in force
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        trc_material_params_release(ctx);
        return TRC_OK;
    }
    if (!p || n_material != ctx->ks.sc.n_materials)
        return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_material_params: p == NULL or n_material is not the scene's");
    for (uint32_t i = 0; i < n_material; ++i)
        if (const char* why = params_check(p[i]))
            return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_material_params: material " + std::to_string(i) + ": " + why);
    DevBuf fresh;      // allocated before the old table goes: TRC_ERR_OOM leaves it in force
    TRC_TRY(fresh.alloc(ctx, (size_t)n_material * sizeof(trc_material_params), "material parameters"));
    TRC_TRY(trc_copy_to_device(ctx, fresh.p, p, (size_t)n_material * sizeof(trc_material_params), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // a launch in flight may still read the old one
    trc_material_params_release(ctx);
    ctx->d_mparams = static_cast<trc_material_params*>(fresh.release()); ctx->n_mparams = n_material;
    return TRC_OK;
}

trc_status trc_download_material_params(trc_ctx* ctx, trc_material_params* out, uint32_t n_material) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_mparams) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_material_params: no table in force");
    if (n_material != ctx->n_mparams) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_material_params: n_material is not the table's");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_copy_to_host(ctx, out, ctx->d_mparams, (size_t)n_material * sizeof(trc_material_params), ctx->stream);
}

}  // extern "C"
