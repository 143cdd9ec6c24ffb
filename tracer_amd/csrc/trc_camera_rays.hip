// trc_camera_rays.hip -- the ray sets of TRC_FLAG_CAMERA_RAYS (tracer_abi.h): uploaded by the host, or generated on the device from the
// context's camera (k_make_camera_rays: the arithmetic of include/trc_raygen.h), downloaded, cleared.  The kernels that read them:
// trc_render_rays.hpp; their choice: trc_render_pass.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "trc_ctx.hpp"
#include "trc_raygen.h"

// One thread per ray over W * H * n_sets, set-major then row-major; the record leaves as two 16-byte stores.  offsets: 2 floats per set
// (null: all zero).
__global__ void __launch_bounds__(256) k_make_camera_rays(const trc_raygen_camera cam, uint32_t model, uint32_t W, uint32_t H, uint32_t n_sets,
                                                          const float* __restrict__ offsets, float4* __restrict__ rays) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x, per_set = (uint64_t)W * H;
    if (i >= per_set * n_sets) return;
    const uint32_t k = (uint32_t)(i / per_set), pix = (uint32_t)(i - (uint64_t)k * per_set);
    const uint32_t y = pix / W, x = pix - y * W;
    const float dx = offsets ? offsets[2u * k] : 0.0f, dy = offsets ? offsets[2u * k + 1u] : 0.0f;
    trc_ray r;
    trc_raygen_ray(&cam, model, x, y, W, H, dx, dy, &r);
    rays[2u * i] = make_float4(r.origin[0], r.origin[1], r.origin[2], r.tmax);
    rays[2u * i + 1u] = make_float4(r.direction[0], r.direction[1], r.direction[2], __uint_as_float(r._pad));
}

void trc_camera_rays_release(trc_ctx* ctx) {
    (void)hipFree(ctx->d_cam_rays); ctx->d_cam_rays = nullptr; ctx->n_ray_sets = 0;
    ctx->ray_gen++;                                 // whatever comes next is another generation (trc_denoise under trc_denoise_guide_rays)
    if (ctx->cost_rays) trc_forget_costs(ctx);      // the recorded block costs were measured on these rays
}

// What the three calls that need a frame share: the kept launch first, then the arguments' context and the frame
static trc_status rays_entry(trc_ctx* ctx, const char* who) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, std::string(who) + " before trc_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return TRC_OK;
}
static size_t set_bytes(const trc_ctx* ctx) { return (size_t)ctx->width * ctx->height * sizeof(trc_ray); }
// `fresh` becomes the rays in force: a launch in flight may still read the old ones
static trc_status adopt_rays(trc_ctx* ctx, DevBuf& fresh, uint32_t n_sets) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    trc_camera_rays_release(ctx);
    ctx->d_cam_rays = static_cast<trc_ray*>(fresh.release()); ctx->n_ray_sets = n_sets;
    return TRC_OK;
}

extern "C" {

trc_status trc_upload_camera_rays(trc_ctx* ctx, const trc_ray* rays, uint32_t n_sets) {
    TRC_TRY(rays_entry(ctx, "trc_upload_camera_rays"));
    if (!rays || n_sets == 0 || n_sets > TRC_MAX_RAY_SETS) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_upload_camera_rays: rays == NULL or n_sets outside 1 .. TRC_MAX_RAY_SETS");
    DevBuf fresh;      // allocated before the old rays go: TRC_ERR_OOM leaves them in force
    TRC_TRY(fresh.alloc(ctx, set_bytes(ctx) * n_sets, "camera rays"));
    TRC_TRY(trc_copy_to_device(ctx, fresh.p, rays, set_bytes(ctx) * n_sets, ctx->stream));
    return adopt_rays(ctx, fresh, n_sets);
}

trc_status trc_generate_camera_rays(trc_ctx* ctx, const trc_ray_gen* g) {
    TRC_TRY(rays_entry(ctx, "trc_generate_camera_rays"));
    if (!ctx->has_camera) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_generate_camera_rays before trc_set_camera");
    if (!g || g->n_sets == 0 || g->n_sets > TRC_MAX_RAY_SETS || g->model > TRC_RAYS_EQUIRECT)
        return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_generate_camera_rays: g == NULL, n_sets outside 1 .. TRC_MAX_RAY_SETS or unknown model");
    for (uint32_t i = 0; g->offsets && i < 2u * g->n_sets; ++i)
        if (!(g->offsets[i] >= 0.0f && g->offsets[i] < 1.0f)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_generate_camera_rays: offset outside [0, 1)");
    DevBuf fresh, d_offsets;
    TRC_TRY(fresh.alloc(ctx, set_bytes(ctx) * g->n_sets, "camera rays"));
    if (g->offsets) {
        TRC_TRY(d_offsets.alloc(ctx, 2u * g->n_sets * sizeof(float), "camera-ray offsets"));
        TRC_TRY(trc_copy_to_device(ctx, d_offsets.p, g->offsets, 2u * g->n_sets * sizeof(float), ctx->stream));
    }
    trc_raygen_camera cam;
    for (int k = 0; k < 3; ++k) {
        cam.lookFrom[k] = ctx->cam.lookFrom[k]; cam.horizontal[k] = ctx->cam.horizontal[k];
        cam.vertical[k] = ctx->cam.vertical[k]; cam.cornerLowLeft[k] = ctx->cam.cornerLowLeft[k];
    }
    const uint64_t n = (uint64_t)ctx->width * ctx->height * g->n_sets;
    hipLaunchKernelGGL(k_make_camera_rays, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, ctx->stream, cam, g->model, ctx->width, ctx->height, g->n_sets,
                       d_offsets.as<float>(), fresh.as<float4>());
    HIP_TRY(ctx, hipGetLastError());
    return adopt_rays(ctx, fresh, g->n_sets);      // synchronises: d_offsets may go
}

trc_status trc_download_camera_rays(trc_ctx* ctx, uint32_t set, trc_ray* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_cam_rays) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_download_camera_rays: no camera rays in force");
    if (set >= ctx->n_ray_sets) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_download_camera_rays: set >= n_sets");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_copy_to_host(ctx, out, ctx->d_cam_rays + (size_t)set * ctx->width * ctx->height, set_bytes(ctx), ctx->stream);
}

trc_status trc_clear_camera_rays(trc_ctx* ctx) {
    TRC_TRY(rays_entry(ctx, "trc_clear_camera_rays"));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    trc_camera_rays_release(ctx);
    return TRC_OK;
}

}  // extern "C"
