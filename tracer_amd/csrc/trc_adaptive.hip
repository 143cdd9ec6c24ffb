// trc_adaptive.hip -- samples where the picture is still noisy: the tile mask of trc_render's block list (trc_set_tile_mask), the per-tile
// error estimate (trc_tile_snapshot, trc_tile_error: k_tile_error) and the driver that stops the tiles that have settled
// (trc_render_adaptive: k_tile_decide).  include/tracer_abi.h is the definition, operation by operation; tests/adaptive_ref.py restates it.
// No render kernel knows about any of this: a masked launch is an ordinary launch over a shorter block list (trc_schedule.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "trc_ctx.hpp"

// E_t of one tile per 256-lane workgroup, one pixel per lane: lane l holds pixel (16 tx + (l & 15), 16 ty + (l >> 4)), so a wavefront reads
// four tile rows of 256 bytes from each plane with one 16-byte load per lane.  q is summed as integers -- across the wavefront in registers,
// the four wave totals through LDS -- so the result does not depend on the order.  A workgroup whose tile is masked off returns at once
// (the branch is uniform).  snapshot_after: A := I on the way, one 16-byte store per lane.
__global__ void __launch_bounds__(256) k_tile_error(const float4* __restrict__ accum, float4* __restrict__ snap, uint32_t W, uint32_t H, uint32_t tiles_x,
                                                    const uint8_t* __restrict__ mask, float* __restrict__ err, const int snapshot_after) {
    __shared__ unsigned long long s_wave[4];
    const uint32_t t = blockIdx.x;
    if (!mask[t]) return;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t x = tx * TRC_TILE + (threadIdx.x & 15u), y = ty * TRC_TILE + (threadIdx.x >> 4);
    unsigned long long q = 0ull;
    if (x < W && y < H) {
        const size_t at = (size_t)y * W + x;
        const float4 I = accum[at], A = snap[at];
        const float d = (fabsf(I.x - A.x) + fabsf(I.y - A.y)) + fabsf(I.z - A.z);
        const float s = (I.x + I.y) + I.z;
        const float s1 = s > TRC_ADAPTIVE_EPS ? s : TRC_ADAPTIVE_EPS;
        const float e = d / sqrtf(s1);
        const float e1 = e < 65535.0f ? e : 65535.0f;
        q = (unsigned long long)(uint32_t)(e1 * 65536.0f);
        if (snapshot_after) snap[at] = I;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t nx = min((uint32_t)TRC_TILE, W - tx * TRC_TILE), ny = min((uint32_t)TRC_TILE, H - ty * TRC_TILE);
        const unsigned long long sum = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        err[t] = (float)((double)sum / ((double)(nx * ny) * 65536.0));
    }
}

// step 4 of trc_render_adaptive, one thread per tile: n_t = n for every tile that was rendered in this round; a tile whose estimate has
// fallen to the threshold leaves the mask for good.  decide[0]: the tiles that stay, decide[1]: the largest E_t of the frame, as the bits
// of a float that is never negative and never NaN (so unsigned order is the floats' order).  Both zeroed by the host before the launch.
__global__ void __launch_bounds__(256) k_tile_decide(uint8_t* mask, const float* err, uint32_t* samples, uint32_t n_tiles, uint32_t n, float threshold,
                                                     uint32_t* decide) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tiles) return;
    const float e = err[t];
    atomicMax(&decide[1], __float_as_uint(e));
    if (!mask[t]) return;
    samples[t] = n;
    if (e <= threshold) mask[t] = 0;
    else atomicAdd(&decide[0], 1u);
}

// ----------------------------------------------------------------------- the mask
void trc_adaptive_release(trc_ctx* ctx) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    (void)hipFree(ad.d_mask); (void)hipFree(ad.d_snapshot); (void)hipFree(ad.d_error); (void)hipFree(ad.d_samples); (void)hipFree(ad.d_decide);
    ad.d_mask = nullptr; ad.d_snapshot = nullptr; ad.d_error = nullptr; ad.d_samples = nullptr; ad.d_decide = nullptr;
    ad.tile_mask.clear(); ad.mask_gen = 0; ad.shrinks_from = ~0ull; ad.mask_on_device = false; ad.has_samples = false;
}

// the device's copy of the mask in force (all ones without one), made when a kernel first needs it
static trc_status mask_to_device(trc_ctx* ctx) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const uint32_t n = trc_tile_count(ctx);
    if (!ad.d_mask) { HIP_TRY(ctx, hipMalloc((void**)&ad.d_mask, ((size_t)n + 15u) & ~(size_t)15u)); ad.mask_on_device = false; }
    if (ad.mask_on_device) return TRC_OK;
    if (ad.mask_gen) TRC_TRY(trc_copy_to_device(ctx, ad.d_mask, ad.tile_mask.data(), n, ctx->stream));
    else HIP_TRY(ctx, hipMemsetAsync(ad.d_mask, 1, n, ctx->stream));
    ad.mask_on_device = true;
    return TRC_OK;
}

// `mask` (trc_tile_count bytes, null: every tile) becomes the mask in force.  A mask that only clears tiles of the one before it says so
// (shrinks_from): trc_ensure_tiles then keeps the surviving blocks' costs.  The block list itself is rebuilt by the next launch.
trc_status trc_adopt_tile_mask(trc_ctx* ctx, const uint8_t* mask, bool on_device) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const uint32_t n = trc_tile_count(ctx);
    if (!mask) {
        ad.tile_mask.clear(); ad.mask_gen = 0; ad.shrinks_from = ~0ull; ad.mask_on_device = false;
        return TRC_OK;
    }
    bool subset = true;
    if (ad.mask_gen) for (uint32_t t = 0; t < n && subset; ++t) subset = !mask[t] || ad.tile_mask[t];
    // the list that stands may be the one of the mask before, or still that of a mask further back which the one before only shrank
    const uint64_t from = !subset ? ~0ull : ctx->tiles_mask_gen == ad.mask_gen ? ad.mask_gen : ad.shrinks_from == ctx->tiles_mask_gen ? ad.shrinks_from : ~0ull;
    ad.tile_mask.resize(n);
    for (uint32_t t = 0; t < n; ++t) ad.tile_mask[t] = mask[t] ? 1 : 0;
    ad.mask_gen = ++ad.next_gen;
    ad.shrinks_from = from;
    ad.mask_on_device = on_device && ad.d_mask;
    TRC_TRY(mask_to_device(ctx));
    // a mask that shrinks the list that stands: the list follows at once, with the costs of the blocks that stay (trc_debug_block_costs
    // shows them); any other list is made by the launch that needs it
    if (from != ~0ull && ctx->d_tiles && ctx->tiles_nranks)
        return trc_ensure_tiles(ctx, ctx->tiles_nranks, ctx->tiles_rank, ctx->tiles_view_height, ctx->tiles_blk_shift, true);
    return TRC_OK;
}

static trc_status adaptive_entry(trc_ctx* ctx, const char* what) {
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (ctx->grouped()) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, std::string(what) + ": not on a context in a group");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, std::string(what) + " before trc_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return TRC_OK;
}

static trc_status tile_snapshot(trc_ctx* ctx) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const size_t bytes = (size_t)ctx->width * ctx->height * 16;
    if (!ad.d_snapshot && hipMalloc((void**)&ad.d_snapshot, bytes) != hipSuccess) { ad.d_snapshot = nullptr; (void)hipGetLastError(); return trc_fail(ctx, TRC_ERR_OOM, "hipMalloc tile snapshot"); }
    HIP_TRY(ctx, hipMemcpyAsync(ad.d_snapshot, ctx->d_accum, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return TRC_OK;
}

static trc_status ensure_tile_arrays(trc_ctx* ctx) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const uint32_t n = trc_tile_count(ctx);
    if (!ad.d_error) {
        HIP_TRY(ctx, hipMalloc((void**)&ad.d_error, (size_t)n * 4));
        HIP_TRY(ctx, hipMemsetAsync(ad.d_error, 0, (size_t)n * 4, ctx->stream));
    }
    if (!ad.d_samples) {
        HIP_TRY(ctx, hipMalloc((void**)&ad.d_samples, (size_t)n * 4));
        HIP_TRY(ctx, hipMemsetAsync(ad.d_samples, 0, (size_t)n * 4, ctx->stream));
    }
    if (!ad.d_decide) HIP_TRY(ctx, hipMalloc((void**)&ad.d_decide, 2 * sizeof(uint32_t)));
    return mask_to_device(ctx);
}

static trc_status tile_error(trc_ctx* ctx, int snapshot_after) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    if (!ad.d_snapshot) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_tile_error before trc_tile_snapshot");
    TRC_TRY(ensure_tile_arrays(ctx));
    hipLaunchKernelGGL(k_tile_error, dim3(trc_tile_count(ctx)), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(ctx->d_accum),
                       reinterpret_cast<float4*>(ad.d_snapshot), ctx->width, ctx->height, trc_tiles_x(ctx), ad.d_mask, ad.d_error, snapshot_after ? 1 : 0);
    HIP_TRY(ctx, hipGetLastError());
    return TRC_OK;
}

// the driver's loop (tracer_abi.h); the mask is the driver's own from here on, the caller puts the host's back
static trc_status adaptive_loop(trc_ctx* ctx, const trc_params* p, const trc_adaptive_params* a, trc_adaptive_report* rep) {
    trc_ctx::Adaptive& ad = ctx->adaptive;
    const uint32_t n_tiles = trc_tile_count(ctx), tiles_x = trc_tiles_x(ctx);
    TRC_TRY(trc_adopt_tile_mask(ctx, nullptr));
    TRC_TRY(ensure_tile_arrays(ctx));
    HIP_TRY(ctx, hipMemsetAsync(ad.d_samples, 0, (size_t)n_tiles * 4, ctx->stream));
    ad.has_samples = true;
    trc_params q = *p;
    TRC_TRY(trc_render_now(ctx, &q));
    TRC_TRY(tile_snapshot(ctx));
    std::vector<uint8_t> mask(n_tiles, 1), next(n_tiles);
    std::vector<uint32_t> n_t(n_tiles, 0u);
    uint32_t n = p->spp, active = n_tiles, decide[2] = {0u, 0u};
    rep->passes = 1;
    while (n < a->max_spp && active) {
        q.spp = std::min(n, a->max_spp - n); q.frame0 = n;
        TRC_TRY(trc_render_now(ctx, &q));
        n += q.spp;
        rep->passes++;
        TRC_TRY(tile_error(ctx, 1));
        HIP_TRY(ctx, hipMemsetAsync(ad.d_decide, 0, sizeof decide, ctx->stream));
        hipLaunchKernelGGL(k_tile_decide, dim3((n_tiles + 255) / 256), dim3(256), 0, ctx->stream, ad.d_mask, ad.d_error, ad.d_samples, n_tiles, n, a->threshold,
                           ad.d_decide);
        // the new mask and the two words in ONE read-back (a frame of more tiles than the pinned buffer holds: two)
        if ((size_t)n_tiles + 64u <= kXferChunk) TRC_TRY(trc_read_to_host(ctx, ctx->stream, "k_tile_decide", {{next.data(), ad.d_mask, n_tiles}, {decide, ad.d_decide, sizeof decide}}));
        else {
            TRC_TRY(trc_copy_to_host(ctx, next.data(), ad.d_mask, n_tiles, ctx->stream));
            TRC_TRY(trc_read_to_host(ctx, ctx->stream, "k_tile_decide", {{decide, ad.d_decide, sizeof decide}}));
        }
        for (uint32_t t = 0; t < n_tiles; ++t) if (mask[t]) n_t[t] = n;
        mask = next;
        active = decide[0];
        TRC_TRY(trc_adopt_tile_mask(ctx, mask.data(), true));      // (k_tile_decide wrote it) the list of the next pass: the surviving blocks keep their costs (trc_ensure_tiles)
    }
    rep->active_tiles = active;
    std::memcpy(&rep->max_error, &decide[1], 4);
    rep->samples = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
        const uint64_t px = (uint64_t)std::min((uint32_t)TRC_TILE, ctx->width - tx * TRC_TILE) * std::min((uint32_t)TRC_TILE, ctx->height - ty * TRC_TILE);
        rep->samples += px * n_t[t];
    }
    return TRC_OK;
}

extern "C" {

trc_status trc_set_tile_mask(trc_ctx* ctx, const uint8_t* mask, uint32_t n_tiles) {
    TRC_TRY(trc_flush(ctx));          // a kept launch belongs to the mask it was asked under
    TRC_TRY(adaptive_entry(ctx, "trc_set_tile_mask"));
    if (mask && n_tiles != trc_tile_count(ctx)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_set_tile_mask: n_tiles is not ceil(W / 16) * ceil(H / 16)");
    return trc_adopt_tile_mask(ctx, mask);
}

trc_status trc_download_tile_mask(trc_ctx* ctx, uint8_t* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_download_tile_mask before trc_resize");
    const uint32_t n = trc_tile_count(ctx);
    if (ctx->adaptive.mask_gen) std::memcpy(out, ctx->adaptive.tile_mask.data(), n);
    else std::memset(out, 1, n);
    return TRC_OK;
}

trc_status trc_tile_snapshot(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    TRC_TRY(adaptive_entry(ctx, "trc_tile_snapshot"));
    return tile_snapshot(ctx);
}

trc_status trc_tile_error(trc_ctx* ctx, int snapshot_after) {
    TRC_TRY(trc_flush(ctx));
    TRC_TRY(adaptive_entry(ctx, "trc_tile_error"));
    return tile_error(ctx, snapshot_after);
}

trc_status trc_download_tile_error(trc_ctx* ctx, float* e) {
    TRC_TRY(trc_flush(ctx));
    TRC_TRY(adaptive_entry(ctx, "trc_download_tile_error"));
    if (!e) return TRC_ERR_INVALID_ARG;
    TRC_TRY(ensure_tile_arrays(ctx));
    return trc_copy_to_host(ctx, e, ctx->adaptive.d_error, (size_t)trc_tile_count(ctx) * 4, ctx->stream);
}

void trc_adaptive_default_params(trc_adaptive_params* out) {
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->threshold = TRC_ADAPTIVE_DEFAULT_THRESHOLD;
    out->max_spp = 256;
}

trc_status trc_render_adaptive(trc_ctx* ctx, const trc_params* p, const trc_adaptive_params* a, trc_adaptive_report* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !p || !a) return TRC_ERR_INVALID_ARG;
    if (ctx->grouped()) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_render_adaptive: not on a context in a group");
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_render_adaptive before trc_upload_scene");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_render_adaptive before trc_resize");
    if (!ctx->has_camera) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render_adaptive before trc_set_camera");
    if (p->frame0 != 0) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render_adaptive: frame0 must be 0 (the call starts a picture)");
    if (p->spp < 8) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render_adaptive: a first pass of at least 8 samples");
    if (a->max_spp / 2u < p->spp) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render_adaptive: max_spp < 2 * spp");
    if (!(a->threshold > 0.0f) || !std::isfinite(a->threshold)) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_render_adaptive: threshold must be finite and > 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    trc_params probe = *p; probe.spp = 0;
    TRC_TRY(trc_render_now(ctx, &probe));        // what trc_render refuses (integrator, flags, tile_rank ...), before anything changes
    const std::vector<uint8_t> host_mask = ctx->adaptive.tile_mask;
    const bool had_mask = ctx->adaptive.mask_gen != 0;
    trc_adaptive_report rep{};
    const trc_status st = adaptive_loop(ctx, p, a, &rep);
    const std::string err = ctx->error;
    const trc_status back = trc_adopt_tile_mask(ctx, had_mask ? host_mask.data() : nullptr);
    if (st != TRC_OK) { ctx->error = err; return st; }
    TRC_TRY(back);
    if (out) *out = rep;
    return TRC_OK;
}

trc_status trc_download_tile_samples(trc_ctx* ctx, uint32_t* n) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !n) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_accum || !ctx->adaptive.has_samples) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_download_tile_samples before trc_render_adaptive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return trc_copy_to_host(ctx, n, ctx->adaptive.d_samples, (size_t)trc_tile_count(ctx) * 4, ctx->stream);
}

}  // extern "C"
