// trc_hooks.hip -- the arithmetic, texture and profile entry points of include/tracer_test_hooks.h with their kernels:
// compiled with -DTRC_TEST_HOOKS for libtracer_amd_hooks.so (Makefile: HOOK_TU); the product's build holds trc_has_test_hooks alone.
#include <hip/hip_runtime.h>

#include <string>

#include "trc_ctx.hpp"
#include "trc_render_config.hpp"

extern "C" int trc_has_test_hooks(void) {
#ifdef TRC_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

#ifdef TRC_TEST_HOOKS      // libtracer_amd_hooks.so only (include/tracer_test_hooks.h)
// trc_div_by_test: a[i] / b[i] through the guarded shared-divisor path (three numerators a, -a, a * 0.75 on one divisor) and
// through the plain division
__global__ void __launch_bounds__(256) k_div_by_test(const float* a, const float* b, uint32_t n, float* fast, float* plain) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float av = a[i], bv = b[i];
    const GuardedDivBy d = guarded_div_by(bv);
    const F3 q = guarded_div(f3(av, -av, av * 0.75f), d);
    fast[3 * i] = q.x; fast[3 * i + 1] = q.y; fast[3 * i + 2] = q.z;
    plain[3 * i] = av / bv; plain[3 * i + 1] = -av / bv; plain[3 * i + 2] = (av * 0.75f) / bv;
}

// trc_unary_test: rcp_cr / sqrt_cr / rsqrt_cr (dev_vec.hpp) against the compiler's 1.0f / x, sqrtf(x), 1.0f / sqrtf(x) over a
// range of BIT PATTERNS; counts the operands whose results differ (NaN == NaN) and keeps the smallest one
__global__ void __launch_bounds__(256) k_unary_test(uint32_t op, uint32_t first, uint64_t count, unsigned long long* out) {
    unsigned long long bad = 0, first_bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        float a, b;
        if (op == 0u) { a = rcp_cr(x); b = 1.0f / x; }
        else if (op == 1u) { a = sqrt_cr(x); b = sqrtf(x); }
#if TRC_WAVE_GUARDS
        else if (op == 3u) { a = div_const(x, div_by_pi()); b = x / kPi; }
        else if (op == 4u) { a = div_const(x, div_by_sqr001()); b = x / (0.01f * 0.01f); }
        else if (op == 5u) { a = div_const(x, div_by_sqr002()); b = x / (0.02f * 0.02f); }
        else if (op == 6u) { a = div_const(x, div_by_sqr01()); b = x / (0.1f * 0.1f); }
#endif
        else { a = rsqrt_cr(x); b = 1.0f / sqrtf(x); }
        const bool same = __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
        if (!same) { bad++; first_bad = min(first_bad, (unsigned long long)bits); }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first_bad); }
}

// trc_material_s_f_test: material_S_F (dev_bsdf.hpp) in either form, one lane per input, so that the order of the inputs decides
// which materials share a wavefront.  Both forms, and both texts of sample11 (ONCE: TRC_SAMPLE11_ONCE), are instantiated here whatever
// TRC_MICROFACET_STREAM and TRC_SAMPLE11_ONCE say.
template <bool STREAM, int ONCE = 0>
__global__ void __launch_bounds__(256) k_material_s_f_test(const uint32_t* type, const float* color, const float* wo, const float* uu,
                                                           uint32_t n, float pdf_init, float* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    F2 u; u.x = uu[2 * i]; u.y = uu[2 * i + 1];
    F3 wi = f3(0);
    float pdf = pdf_init;
    TravCounters none;
    const F3 f = material_S_F<false, STREAM, ONCE>((int)type[i], f3(color[3 * i], color[3 * i + 1], color[3 * i + 2]),
                                             f3(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]), wi, u, pdf, none);
    float* o = out + 7 * (size_t)i;
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = f.x; o[4] = f.y; o[5] = f.z; o[6] = pdf;
}

// trc_sample11_test: sample11 alone, one lane per input.  STREAM: Microfacet::sample11 with the family per lane, else a branch per family
// (Beckmann::sample11, TrowbridgeReitzD::sample11); ONCE: the text (TRC_SAMPLE11_ONCE); CAP: the bound of the Newton loop
template <bool STREAM, int ONCE, int CAP>
__global__ void __launch_bounds__(256) k_sample11_test(const uint32_t* family, float alpha_y, const float* in, uint32_t n, float* slopes,
                                                       uint32_t* exit_kind) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const bool tr = family[i] != 0u;
    const float cosTheta = in[4 * i], sinTheta = in[4 * i + 1], U1 = in[4 * i + 2], U2 = in[4 * i + 3];
    float sx = 0, sy = 0;
    int kind;
    if constexpr (STREAM) {
        Microfacet d = Microfacet::make_lobe(tr, false);
        d.alpha_y = alpha_y;
        kind = d.template sample11<ONCE, CAP>(cosTheta, sinTheta, U1, U2, sx, sy);
    } else if (tr) {
        TrowbridgeReitzD<Alpha_01_02>::sample11(cosTheta, sinTheta, U1, U2, sx, sy);
        kind = cosTheta > .9999f ? kS11Corner : kS11ClosedForm;
    } else {
        kind = Beckmann::sample11<ONCE, CAP>(cosTheta, sinTheta, U1, U2, sx, sy);
    }
    slopes[2 * i] = sx; slopes[2 * i + 1] = sy;
    exit_kind[i] = (uint32_t)kind;
}
// trc_material_params_test: material_S_F_params / material_F_params (dev_bsdf.hpp), one lane per input: lane i reads entry i of `table`
__global__ void __launch_bounds__(256) k_material_params_test(uint32_t op, const uint32_t* type, const float* color, const float4* table, const float* wo,
                                                              const float* wi_in, const float* uu, uint32_t n, float pdf_init, float* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    F2 u; u.x = uu[2 * i]; u.y = uu[2 * i + 1];
    const F3 c = f3(color[3 * i], color[3 * i + 1], color[3 * i + 2]), o3 = f3(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]);
    if (op != 1u) {                                   // op 2: sample11 evaluating each exp, log and erf_inv once (TRC_SAMPLE11_ONCE 7)
        F3 wi = f3(0);
        float pdf = pdf_init;
        const F3 f = op == 0u ? material_S_F_params<0>((int)type[i], c, table, i, o3, wi, u, pdf)
                              : material_S_F_params<7>((int)type[i], c, table, i, o3, wi, u, pdf);
        float* o = out + 7 * (size_t)i;
        o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = f.x; o[4] = f.y; o[5] = f.z; o[6] = pdf;
    } else {
        float pdf = pdf_init;
        const F3 f = material_F_params((int)type[i], c, table, i, o3, f3(wi_in[3 * i], wi_in[3 * i + 1], wi_in[3 * i + 2]), u, pdf);
        float* o = out + 4 * (size_t)i;
        o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pdf;
    }
}

template <bool STREAM, int ONCE>
static void launch_sample11(uint32_t cap, dim3 grid, hipStream_t st, const uint32_t* family, float alpha_y, const float* in, uint32_t n,
                            float* slopes, uint32_t* kind) {
    if (cap == 2u) hipLaunchKernelGGL((k_sample11_test<STREAM, ONCE, 2>), grid, dim3(256), 0, st, family, alpha_y, in, n, slopes, kind);
    else if (cap == 3u) hipLaunchKernelGGL((k_sample11_test<STREAM, ONCE, 3>), grid, dim3(256), 0, st, family, alpha_y, in, n, slopes, kind);
    else hipLaunchKernelGGL((k_sample11_test<STREAM, ONCE, 10>), grid, dim3(256), 0, st, family, alpha_y, in, n, slopes, kind);
}

extern "C" {
// developer diagnostic: (lanes, wavefronts) that executed each ProfSite of the instrumented kernels
trc_status trc_debug_profile(trc_ctx* ctx, uint64_t* out, uint32_t n_sites) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long h[kStatCount + 3 * kProfCount];
    TRC_TRY(trc_read_stats_sum(ctx, h, kStatCount + 3 * kProfCount));
    for (uint32_t i = 0; i < n_sites && i < (uint32_t)kProfCount; ++i)
        for (int k = 0; k < 3; ++k) out[3 * i + k] = h[kStatCount + 3 * i + k];
    return TRC_OK;
}

// the render kernels' image lookup (dev_integrator.hpp image_sample), one lane per uv pair
__global__ void __launch_bounds__(256) k_texture_sample_test(const float* texels, const uint4* desc, uint32_t n_tex, uint32_t index,
                                                             const float* uv, uint32_t n, float* rgb) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    TexTable tt; tt.texels = texels; tt.desc = desc; tt.n = n_tex;
    F2 p; p.x = uv[2 * i]; p.y = uv[2 * i + 1];
    const F3 c = image_sample(tt, index, p);
    rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
}
trc_status trc_texture_sample_test(trc_ctx* ctx, uint32_t index, const float* uv, size_t n, float* rgb) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || (n && (!uv || !rgb))) return TRC_ERR_INVALID_ARG;
    if (index >= ctx->n_tex) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_texture_sample_test: no such image");
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu / 3u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_texture_sample_test: too many pairs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;           // (freeing it waits for whatever a failed step left in flight)
    TRC_TRY(d.alloc(ctx, n * 5 * sizeof(float), "texture sample test"));
    float *d_uv = d.as<float>(), *d_rgb = d_uv + 2 * n;
    TRC_TRY(trc_copy_to_device(ctx, d_uv, uv, n * 8, ctx->stream));
    hipLaunchKernelGGL(k_texture_sample_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->d_tex_texels, ctx->d_tex_desc, ctx->n_tex, index, d_uv, (uint32_t)n, d_rgb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_texture_sample_test: ") + hipGetErrorString(e));
    return trc_copy_to_host(ctx, rgb, d_rgb, n * 12, ctx->stream);
}

// the kernel choice of the last render launch (trc_render_pass.hip: choose_kernel)
trc_status trc_debug_last_kernel(trc_ctx* ctx, trc_kernel_choice* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    const trc_ctx::LastKernel& k = ctx->last_kernel;
    out->shape = k.shape; out->variant = k.variant; out->lds_resident = k.lds_resident; out->triangle_materials = k.tri_materials;
    out->strip = k.strip; out->launches = k.count;
    return TRC_OK;
}
// ... and whether it was a kernel of TRC_FLAG_CAMERA_RAYS (choose_rays_kernel)
trc_status trc_debug_last_camera_rays(trc_ctx* ctx, uint32_t* used) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !used) return TRC_ERR_INVALID_ARG;
    *used = ctx->last_kernel.camera_rays;
    return TRC_OK;
}
// ... or a kernel of TRC_FLAG_MATERIAL_PARAMS (choose_params_kernel)
trc_status trc_debug_last_material_params(trc_ctx* ctx, uint32_t* used) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !used) return TRC_ERR_INVALID_ARG;
    *used = ctx->last_kernel.material_params;
    return TRC_OK;
}
trc_status trc_material_params_test(trc_ctx* ctx, uint32_t op, const uint32_t* type, const float* color, const trc_material_params* params,
                                    const float* wo, const float* wi, const float* uu, size_t n, float pdf_init, float* out) {
    if (!ctx || op > 2u || (n && (!type || !color || !params || !wo || !uu || !out || (op == 1u && !wi)))) return TRC_ERR_INVALID_ARG;
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu / 12u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_material_params_test: too many inputs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    // float4 table first (16-byte aligned), then colour, wo, wi, uu, out (7), type
    TRC_TRY(d.alloc(ctx, n * (12 + 3 + 3 + 3 + 2 + 7 + 1) * sizeof(float), "material params test"));
    float *d_table = d.as<float>(), *d_color = d_table + 12 * n, *d_wo = d_color + 3 * n, *d_wi = d_wo + 3 * n, *d_uu = d_wi + 3 * n, *d_out = d_uu + 2 * n;
    uint32_t* d_type = reinterpret_cast<uint32_t*>(d_out + 7 * n);
    TRC_TRY(trc_copy_to_device(ctx, d_table, params, n * 48, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_color, color, n * 12, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_wo, wo, n * 12, ctx->stream));
    if (op == 1u) TRC_TRY(trc_copy_to_device(ctx, d_wi, wi, n * 12, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_uu, uu, n * 8, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_type, type, n * 4, ctx->stream));
    hipLaunchKernelGGL(k_material_params_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, d_type, d_color,
                       reinterpret_cast<const float4*>(d_table), d_wo, d_wi, d_uu, (uint32_t)n, pdf_init, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_material_params_test: ") + hipGetErrorString(e));
    return trc_copy_to_host(ctx, out, d_out, n * (op != 1u ? 28 : 16), ctx->stream);
}
// how the kernel of the last render launch sits on a CU (trc_render_pass.hip: resident_workgroups): the runtime's answer, asked again here,
// beside the plain arithmetic of trc_lds_fit.hpp for an allocation block of 1280 bytes (320 dwords) -- the runtime's query counts bytes
trc_status trc_debug_last_residency(trc_ctx* ctx, trc_residency* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !out) return TRC_ERR_INVALID_ARG;
    const trc_ctx::LastFit& f = ctx->last_fit;
    *out = trc_residency{};
    if (!f.fn) return TRC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int now = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&now, f.fn, (int)f.block, f.lds));      // not the planner's copy
    hipFuncAttributes attr{};
    HIP_TRY(ctx, hipFuncGetAttributes(&attr, f.fn));
    out->cu_count = (uint32_t)ctx->cu_count; out->block = f.block; out->waves = f.waves; out->planned_per_cu = f.planned_per_cu;
    out->planned_with = f.per_cu; out->per_cu = now > 0 ? (uint32_t)now : 0u; out->lds_bytes = (uint64_t)f.lds;
    out->lds_static_bytes = (uint32_t)attr.sharedSizeBytes;
    out->per_cu_block1280 = trc_lds_workgroups((uint32_t)(f.lds + attr.sharedSizeBytes), 1280u, 160u * 1024u);
    out->dense_memo_rows = ctx->last_kernel.shape == 3u ? (uint32_t)TRC_REPLAY_DENSE : 0u;
    return TRC_OK;
}

trc_status trc_div_by_test(trc_ctx* ctx, const float* a, const float* b, size_t n, float* fast, float* plain) {
    if (!ctx || (n && (!a || !b || !fast || !plain))) return TRC_ERR_INVALID_ARG;
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu / 3u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_div_by_test: too many pairs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    TRC_TRY(d.alloc(ctx, n * 8 * sizeof(float), "div_by test"));
    float *d_a = d.as<float>(), *d_b = d_a + n, *d_fast = d_a + 2 * n, *d_plain = d_a + 5 * n;
    TRC_TRY(trc_copy_to_device(ctx, d_a, a, n * 4, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_b, b, n * 4, ctx->stream));
    hipLaunchKernelGGL(k_div_by_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_a, d_b, (uint32_t)n, d_fast, d_plain);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_div_by_test: ") + hipGetErrorString(e));
    TRC_TRY(trc_copy_to_host(ctx, fast, d_fast, n * 12, ctx->stream));
    return trc_copy_to_host(ctx, plain, d_plain, n * 12, ctx->stream);
}

trc_status trc_material_s_f_test(trc_ctx* ctx, uint32_t stream, const uint32_t* type, const float* color, const float* wo, const float* uu,
                                 size_t n, float pdf_init, float* out) {
    if (!ctx || stream > 3u || (n && (!type || !color || !wo || !uu || !out))) return TRC_ERR_INVALID_ARG;
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu / 7u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_material_s_f_test: too many inputs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    TRC_TRY(d.alloc(ctx, n * 16 * sizeof(float), "material S_F test"));
    float *d_color = d.as<float>(), *d_wo = d_color + 3 * n, *d_uu = d_color + 6 * n, *d_out = d_color + 8 * n;
    uint32_t* d_type = reinterpret_cast<uint32_t*>(d_color + 15 * n);
    TRC_TRY(trc_copy_to_device(ctx, d_color, color, n * 12, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_wo, wo, n * 12, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_uu, uu, n * 8, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_type, type, n * 4, ctx->stream));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (stream == 3u) hipLaunchKernelGGL((k_material_s_f_test<true, 7>), grid, dim3(256), 0, ctx->stream, d_type, d_color, d_wo, d_uu, (uint32_t)n, pdf_init, d_out);
    else if (stream == 2u) hipLaunchKernelGGL((k_material_s_f_test<false, 7>), grid, dim3(256), 0, ctx->stream, d_type, d_color, d_wo, d_uu, (uint32_t)n, pdf_init, d_out);
    else if (stream) hipLaunchKernelGGL(k_material_s_f_test<true>, grid, dim3(256), 0, ctx->stream, d_type, d_color, d_wo, d_uu, (uint32_t)n, pdf_init, d_out);
    else hipLaunchKernelGGL(k_material_s_f_test<false>, grid, dim3(256), 0, ctx->stream, d_type, d_color, d_wo, d_uu, (uint32_t)n, pdf_init, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_material_s_f_test: ") + hipGetErrorString(e));
    return trc_copy_to_host(ctx, out, d_out, n * 28, ctx->stream);
}

trc_status trc_sample11_test(trc_ctx* ctx, uint32_t form, const uint32_t* family, float alpha_y, uint32_t cap, const float* in, size_t n,
                             float* slopes, uint32_t* exit_kind) {
    if (!ctx || form > 3u || (cap != 10u && cap != 3u && cap != 2u) || (n && (!family || !in || !slopes || !exit_kind))) return TRC_ERR_INVALID_ARG;
    if (n == 0) return TRC_OK;
    if (n > 0x7FFFFFFFu / 8u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_sample11_test: too many inputs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    TRC_TRY(d.alloc(ctx, n * 8 * sizeof(float), "sample11 test"));
    float *d_in = d.as<float>(), *d_slopes = d_in + 4 * n;
    uint32_t *d_family = reinterpret_cast<uint32_t*>(d_in + 6 * n), *d_kind = d_family + n;
    TRC_TRY(trc_copy_to_device(ctx, d_in, in, n * 16, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_family, family, n * 4, ctx->stream));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (form == 3u) launch_sample11<true, 7>(cap, grid, ctx->stream, d_family, alpha_y, d_in, (uint32_t)n, d_slopes, d_kind);
    else if (form == 2u) launch_sample11<false, 7>(cap, grid, ctx->stream, d_family, alpha_y, d_in, (uint32_t)n, d_slopes, d_kind);
    else if (form == 1u) launch_sample11<true, 0>(cap, grid, ctx->stream, d_family, alpha_y, d_in, (uint32_t)n, d_slopes, d_kind);
    else launch_sample11<false, 0>(cap, grid, ctx->stream, d_family, alpha_y, d_in, (uint32_t)n, d_slopes, d_kind);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_sample11_test: ") + hipGetErrorString(e));
    TRC_TRY(trc_copy_to_host(ctx, slopes, d_slopes, n * 8, ctx->stream));
    return trc_copy_to_host(ctx, exit_kind, d_kind, n * 4, ctx->stream);
}

trc_status trc_unary_test(trc_ctx* ctx, uint32_t op, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch, uint32_t* first_mismatch) {
    if (!ctx || !n_mismatch || op > 6u || count > (1ull << 32)) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf buf;
    TRC_TRY(buf.alloc(ctx, 16, "unary test"));
    unsigned long long* const d = buf.as<unsigned long long>();
    unsigned long long h[2] = {0ull, ~0ull};
    TRC_TRY(trc_copy_to_device(ctx, d, h, 16, ctx->stream));
    if (count) hipLaunchKernelGGL(k_unary_test, dim3(ctx->cu_count * 16), dim3(256), 0, ctx->stream, op, first_bits, count, d);
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "trc_unary_test", {{h, d, 16}}));
    *n_mismatch = h[0];
    if (first_mismatch) *first_mismatch = (uint32_t)h[1];
    return TRC_OK;
}

}  // extern "C"
#endif  // TRC_TEST_HOOKS
