// camera_rays.cpp -- the host side of the camera-ray sets (tracer_abi.h: "Camera-ray sets"): the generator's definition, from the one
// statement of its arithmetic that the device kernel compiles too (include/trc_raygen.h), and Halton offsets for anti-aliasing sets.
#include <cmath>
#include <cstdint>

#include "tracer_abi.h"
#include "trc_raygen.h"

namespace {

// the radical inverse of i in base b: the exact fraction num / b^digits, rounded once to binary32 (to nearest, ties to even)
float radical_inverse(uint32_t i, uint32_t b) {
    uint64_t num = 0, den = 1;
    for (; i; i /= b) { num = num * b + i % b; den *= b; }
    if (num == 0) return 0.0f;
    int e = 0;                                              // 2^23 <= num * 2^e / den < 2^24
    while (((unsigned __int128)num << e) / den < (1u << 23)) ++e;
    const unsigned __int128 scaled = (unsigned __int128)num << e;
    uint64_t q = (uint64_t)(scaled / den);
    const unsigned __int128 r = scaled - (unsigned __int128)q * den;
    if (2 * r > den || (2 * r == den && (q & 1u))) ++q;
    const float v = std::ldexp((float)q, -e);
    return v < 1.0f ? v : std::nextafter(1.0f, 0.0f);
}

}  // namespace

extern "C" {

trc_status trc_host_generate_camera_rays(const trc_Camera* camera, uint32_t W, uint32_t H, const trc_ray_gen* g, trc_ray* out) {
    if (!camera || !g || !out || W == 0 || H == 0 || g->n_sets == 0 || g->n_sets > TRC_MAX_RAY_SETS || g->model > TRC_RAYS_EQUIRECT) return TRC_ERR_INVALID_ARG;
    for (uint32_t i = 0; g->offsets && i < 2u * g->n_sets; ++i)
        if (!(g->offsets[i] >= 0.0f && g->offsets[i] < 1.0f)) return TRC_ERR_INVALID_ARG;
    trc_raygen_camera cam;
    const trc_float3* src[4] = {&camera->lookFrom, &camera->horizontal, &camera->vertical, &camera->cornerLowLeft};
    float* dst[4] = {cam.lookFrom, cam.horizontal, cam.vertical, cam.cornerLowLeft};
    for (int i = 0; i < 4; ++i) { dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z; }
    for (uint32_t k = 0; k < g->n_sets; ++k) {
        const float dx = g->offsets ? g->offsets[2u * k] : 0.0f, dy = g->offsets ? g->offsets[2u * k + 1u] : 0.0f;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) trc_raygen_ray(&cam, g->model, x, y, W, H, dx, dy, &out[((size_t)k * H + y) * W + x]);
    }
    return TRC_OK;
}

void trc_host_halton_offsets(uint32_t n, float* out) {
    for (uint32_t k = 0; k < n; ++k) { out[2u * k] = radical_inverse(k + 1u, 2u); out[2u * k + 1u] = radical_inverse(k + 1u, 3u); }
}

}  // extern "C"
