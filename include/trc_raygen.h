/*
 * trc_raygen.h -- the arithmetic of the camera-ray generator (tracer_abi.h: trc_generate_camera_rays, trc_host_generate_camera_rays),
 * written once for the device kernel (tracer_amd/csrc/trc_camera_rays.hip: k_make_camera_rays) and the host library
 * (tracer_amd/host/camera_rays.cpp).  binary32, one rounding per operation in the order written, no contraction, divisions
 * correctly rounded; sine and cosine are dm_sinf / dm_cosf of trc_detmath.h.  The exact build of the device library and the host
 * library therefore produce the same bits; the fast-math build contracts and takes the hardware's sine and cosine.
 */
#ifndef TRC_RAYGEN_H
#define TRC_RAYGEN_H

#include <float.h>
#include <stdint.h>

#include "tracer_abi.h"
#include "trc_detmath.h"

/* the camera as the generator reads it: four of trc_Camera's vectors */
typedef struct trc_raygen_camera {
    float lookFrom[3], horizontal[3], vertical[3], cornerLowLeft[3];
} trc_raygen_camera;

/* P(s, t) = (cornerLowLeft + horizontal * s) + vertical * t, per component: cast_ray's `sample` (Camera.hh:59-69) */
TRC_HD void trc_raygen_point(const trc_raygen_camera* c, float s, float t, float p[3]) {
    for (int k = 0; k < 3; ++k) p[k] = (c->cornerLowLeft[k] + c->horizontal[k] * s) + c->vertical[k] * t;
}

/* the ray of pixel (x, y) of a W x H frame under sub-pixel offset (dx, dy) */
TRC_HD void trc_raygen_ray(const trc_raygen_camera* c, uint32_t model, uint32_t x, uint32_t y, uint32_t W, uint32_t H, float dx, float dy, trc_ray* out) {
    const float s = ((float)x + dx) / (float)W, t = ((float)y + dy) / (float)H;
    float o[3], d[3];
    if (model == TRC_RAYS_EQUIRECT) {
        const float phi = 6.2831855f * (s - 0.5f), lat = 3.1415927f * (t - 0.5f);
        const float cl = dm_cosf(lat);
        d[0] = cl * dm_cosf(phi); d[1] = dm_sinf(lat); d[2] = cl * dm_sinf(phi);
        for (int k = 0; k < 3; ++k) o[k] = c->lookFrom[k];
    } else {
        float p[3];
        trc_raygen_point(c, s, t, p);
        if (model == TRC_RAYS_ORTHOGRAPHIC) {
            float m[3];
            trc_raygen_point(c, 0.5f, 0.5f, m);
            for (int k = 0; k < 3; ++k) { o[k] = c->lookFrom[k] + (p[k] - m[k]); d[k] = m[k] - c->lookFrom[k]; }
        } else {
            for (int k = 0; k < 3; ++k) { o[k] = c->lookFrom[k]; d[k] = p[k] - c->lookFrom[k]; }
        }
    }
    out->origin[0] = o[0]; out->origin[1] = o[1]; out->origin[2] = o[2]; out->tmax = FLT_MAX;
    out->direction[0] = d[0]; out->direction[1] = d[1]; out->direction[2] = d[2]; out->_pad = 0u;
}

#endif /* TRC_RAYGEN_H */
