/*
 * tracer_test_hooks.h -- entry points that exist ONLY in libtracer_amd_hooks.so (the sources of libtracer_amd.so compiled
 * with -DTRC_TEST_HOOKS).  They hold device-side arithmetic of the render / SPPM kernels up for inspection by tests/ and
 * tools/; a host never needs them and the product libraries do not export them (tests/test_abi.py checks both lists).
 * Everything a host calls -- including the Scene::hit hook trc_trace_rays, SURVEY 8(b) -- is in tracer_abi.h.
 */
#ifndef TRACER_TEST_HOOKS_H
#define TRACER_TEST_HOOKS_H

#include "tracer_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* developer diagnostic (divergence / cycle profile of the instrumented kernels), per site i since the
 * last trc_reset_stats: out[3*i] = lanes, out[3*i+1] = wavefronts that executed the site, out[3*i+2] =
 * shader-clock cycles those wavefronts spent inside it; sites: 0 loop iteration, 1 box step, 2 square,
 * 3 sphere, 4 cube, 5 triangle, 6 shade, 7 cosine lobe, 8 Metal, 9 Beckmann sampling,
 * 10 Beckmann lobe evaluation (Plastic specular + Glass), 11 path end */
trc_status trc_debug_profile(trc_ctx* ctx, uint64_t* out, uint32_t n_sites);
/* test hook like trc_trace_rays: `hash()` of Photon.hh:71-89 for n cell indices (3 floats each) at one hash scale, as
 * the hashing and refine passes evaluate it (the index into the 512 x 512 grid, before the -1 shift) */
trc_status trc_sppm_hash_cells(trc_ctx* ctx, const float* cells /* n*3 */, size_t n, float hash_scale, float* out /* n */);

/* test hook: the guarded shared-divisor division of tracer_amd/csrc/dev_vec.hpp (one refined reciprocal per divisor, the
 * compiler's own two fused corrections per quotient, plain `/` outside [2^-60, 2^60]) against the plain division, for n
 * operand pairs: fast / plain receive 3 quotients per pair (a / b, -a / b, (0.75 a) / b).  They must agree bit for bit. */
trc_status trc_div_by_test(trc_ctx* ctx, const float* a, const float* b, size_t n, float* fast /* 3 n */, float* plain /* 3 n */);
/* test hook: the render kernels' guard-free reciprocal / square root / reciprocal square root (dev_vec.hpp: rcp_cr, sqrt_cr, rsqrt_cr;
 * op 0 / 1 / 2) against the compiler's correctly rounded 1.0f / x, sqrtf(x), 1.0f / sqrtf(x) on the `count` operands whose bit patterns
 * start at `first_bits` (count = 2^32 covers every float): the number of operands whose results differ, and the smallest one.
 * op 3 .. 6: x / c for the divisors known when the kernels are written (pi, 0.01^2, 0.02^2, 0.1^2), computed as the product with
 * RN(1 / c) and one residual correction, against the compiler's x / c */
trc_status trc_unary_test(trc_ctx* ctx, uint32_t op, uint32_t first_bits, uint64_t count, uint64_t* n_mismatch, uint32_t* first_mismatch);

/* test hook of the lobe code: Material::S_F as the render kernels evaluate it (tracer_amd/csrc/dev_bsdf.hpp: material_S_F), one lane per
 * input in the order given, so that the caller decides which materials meet in one wavefront of 64.  For n inputs (material type by
 * ordinal, colour, wo in the shading frame, the two random numbers) out receives 7 floats each: wi, the attenuation and the pdf; wi
 * starts as 0 and the pdf as pdf_init, which an early-out leaves in place.  stream 0: the Metal lobe as a branch of its own; stream 1:
 * through the Beckmann lobes' stream (TRC_MICROFACET_STREAM); stream 2 and 3: those two with Beckmann's sample11 evaluating each exp,
 * log and erf_inv once (TRC_SAMPLE11_ONCE 7).  All four exist here whichever the render kernels were compiled with. */
trc_status trc_material_s_f_test(trc_ctx* ctx, uint32_t stream, const uint32_t* type /* n */, const float* color /* 3 n */,
                                 const float* wo /* 3 n */, const float* uu /* 2 n */, size_t n, float pdf_init, float* out /* 7 n */);

/* test hook of the visible-normal sampling: sample11 of dev_bsdf.hpp alone, one lane per input in the order given (64 consecutive inputs
 * are one wavefront).  form: as `stream` above (0 a branch per family, 1 Microfacet::sample11 with the family per lane, 2 and 3 those with
 * TRC_SAMPLE11_ONCE 7).  family[i]: 0 Beckmann, 1 Trowbridge-Reitz.  alpha_y: the roughness the stream's distribution object is built with
 * (alpha_x is 0.01; sample11 reads the family alone: the roughness reaches it through the stretched direction's cosine and sine).  cap:
 * the bound of Beckmann's Newton loop, 10 as the render kernels run it, or 3 or 2, which make lanes run out of iterations.  in: cosTheta,
 * sinTheta, U1, U2 per input.  slopes: slope_x, slope_y.  exit_kind: 0 the corner cosTheta > .9999, 1 the Newton loop left by its break,
 * 2 the Newton loop ran out, 3 Trowbridge-Reitz's closed form. */
trc_status trc_sample11_test(trc_ctx* ctx, uint32_t form, const uint32_t* family /* n */, float alpha_y, uint32_t cap, const float* in /* 4 n */,
                             size_t n, float* slopes /* 2 n */, uint32_t* exit_kind /* n */);

/* test hook of the SVGF stage (tracer_abi.h, trc_denoise): the state the last trc_denoise left, W*H float4 each (any pointer may
 * be NULL): integrated = the temporal pass's (colour, variance), history = the colour history the next frame reprojects
 * (a-trous iteration 0's (colour, variance), or the integrated colour at 0 iterations), moments = (mu1, mu2, history length, 0).
 * TRC_ERR_NO_FRAME before a trc_denoise. */
trc_status trc_debug_denoise_state(trc_ctx* ctx, float* integrated, float* history, float* moments);

/* test hook of the image textures (tracer_abi.h, trc_upload_textures): the render kernels' lookup of image `index` at n uv
 * pairs (the non-finite rule included), one lane per pair: rgb receives 3 n floats.  TRC_ERR_INVALID_ARG when index is not
 * below the number of uploaded images. */
trc_status trc_texture_sample_test(trc_ctx* ctx, uint32_t index, const float* uv /* 2 n */, size_t n, float* rgb /* 3 n */);

/* test hooks of TRC_FLAG_ENV_LIGHT (tracer_abi.h); both build the current map's sampling tables if they are not built
 * (TRC_ERR_UNSUPPORTED without a map).  trc_debug_env_tables downloads them (any pointer may be NULL): the W*H cell weights, the
 * rows' alias tables (W*H {threshold, alias} pairs, row after row), the marginal's (H pairs), the float64 total weight and the
 * build's GPU time.  trc_env_light_test runs the render kernels' sampler and pdf (tracer_amd/csrc/dev_envlight.hpp), one lane
 * per item: for n draws (six words each: row index, row alias, cell index, cell alias as 32-bit integers, then two float bit
 * patterns for the point inside the cell) dir_pdf receives the direction and pdf (4 floats each); for m directions (3 floats
 * each) pdf receives the density the sampler gives them. */
trc_status trc_debug_env_tables(trc_ctx* ctx, float* weight, uint32_t* rows, uint32_t* marg, double* total, float* build_ms);
trc_status trc_env_light_test(trc_ctx* ctx, const uint32_t* draws /* 6 n */, size_t n, float* dir_pdf /* 4 n */,
                              const float* dirs /* 3 m */, size_t m, float* pdf /* m */);

/* test hooks of TRC_FLAG_MESH_LIGHTS (tracer_abi.h); both build the scene's tables if they are not built (TRC_ERR_NO_SCENE without a
 * scene).  trc_debug_mesh_light_tables downloads them (any pointer may be NULL): the alias table over the lights ({threshold, alias}
 * pairs, n_lights of them), the lights' triangle indices (n_lights), pdfA (one float per triangle of the scene), the float64 total
 * weight and the light count -- call it once for the count, then with arrays of that size.  trc_mesh_light_test runs the render
 * kernels' sampler (tracer_amd/csrc/dev_meshlight.hpp), one lane per item: for n draws (four words each: light index and alias
 * decision as 32-bit integers, then two float bit patterns for the point) and n shading points (3 floats each) tri receives the
 * triangle and out 7 floats: the point on it (before offset_ray), the normal turned to the shading point, and pdfA.
 * TRC_ERR_UNSUPPORTED when the scene has no light triangle. */
trc_status trc_debug_mesh_light_tables(trc_ctx* ctx, uint32_t* alias /* 2 n_lights */, uint32_t* tri /* n_lights */, float* pdfA /* n_triangles */,
                                       double* total, uint32_t* n_lights);
trc_status trc_mesh_light_test(trc_ctx* ctx, const uint32_t* draws /* 4 n */, const float* pos /* 3 n */, size_t n, uint32_t* tri /* n */,
                               float* out /* 7 n */);

/* test hook of the kernel choice (trc_render_pass.hip: choose_kernel): which render kernel the last launch of this context took.
 * shape: 0 = one pixel block per one-wavefront workgroup (k_render), 1 = a strip of blocks per wavefront (k_render_strip), 2 =
 * persistent workgroups (k_render_pwg), 3 = k_render_dense.  variant: 0 plain, 1 statistics, 2 Sobol', 3 image textures, 4
 * TRC_FLAG_ENV_LIGHT, 5 ... with image textures, 6 TRC_FLAG_MESH_LIGHTS, 7 ... with image textures.  lds_resident: the whole tree was
 * staged in LDS (else read from memory).  triangle_materials: the kernels that read each triangle's material ran
 * (trc_upload_triangle_materials).  strip: blocks per wavefront (1 unless shape is 1).  launches: kernel choices made since trc_create
 * (a trc_render call may be several launches; a kept launch of few samples is flushed first).  All zero before the first launch. */
typedef struct trc_kernel_choice {
    uint32_t shape, variant, lds_resident, triangle_materials, strip, launches;
} trc_kernel_choice;
trc_status trc_debug_last_kernel(trc_ctx* ctx, trc_kernel_choice* out);
/* ... and whether that launch ran a kernel of TRC_FLAG_CAMERA_RAYS (tracer_abi.h): *used = 1, else 0.  Such a launch reports shape 0 and
 * variant 0 or 3 above; its kernels have tables of their own, which trc_kernel_choice does not describe. */
trc_status trc_debug_last_camera_rays(trc_ctx* ctx, uint32_t* used);
/* ... or a kernel of TRC_FLAG_MATERIAL_PARAMS (tracer_abi.h): *used = 1, else 0.  Such a launch reports shape 0 and variant 0 or 3 too. */
trc_status trc_debug_last_material_params(trc_ctx* ctx, uint32_t* used);

/* test hook of TRC_FLAG_MATERIAL_PARAMS: the render kernels' parametrised lobes (tracer_amd/csrc/dev_bsdf.hpp), one lane per input in
 * the order given, 256 lanes per workgroup, so that the order of the inputs decides which materials share a wavefront.  Input i has
 * material type type[i], colour color[3 i ..], parameters params[i], wo[3 i ..] and uu[2 i ..].  op 0: Material::S_F with bxPDF preset
 * to pdf_init; out receives 7 floats per input: wi, f, pdf (wi is not read).  op 1: Material::F and its pdf for the pair (wo, wi[3 i ..]);
 * out receives 4 floats per input: f, pdf.  op 2: op 0 with sample11 evaluating each exp, log and erf_inv once (TRC_SAMPLE11_ONCE 7, the text
 * of the units of LDS-resident trees; op 0 runs the reference's).  The parameters are not validated. */
trc_status trc_material_params_test(trc_ctx* ctx, uint32_t op, const uint32_t* type, const float* color /* 3 n */,
                                    const trc_material_params* params /* n */, const float* wo /* 3 n */, const float* wi /* 3 n, op 1 */,
                                    const float* uu /* 2 n */, size_t n, float pdf_init, float* out /* 7 n or 4 n */);

/* test hook of the LDS plans (trc_render_pass.hip: resident_workgroups): how the kernel of the last render launch sits on a CU.
 * cu_count: CUs of the device; block: threads per workgroup; waves: wavefronts per SIMD of the kernel's launch bounds; lds_bytes: dynamic
 * LDS per workgroup; planned_per_cu: workgroups per CU the launch's plan is for (4 x waves, or the persistent workgroups' count);
 * planned_with: the runtime's answer the planner used; per_cu: hipOccupancyMaxActiveBlocksPerMultiprocessor for (kernel, block,
 * lds_bytes), asked again by this call.  The runtime's query counts bytes; beside it, plain arithmetic: lds_static_bytes: the kernel's own
 * LDS; per_cu_block1280: workgroups of lds_bytes + lds_static_bytes that 160 KB hold if LDS is granted in blocks of 1280 bytes.
 * dense_memo_rows: primary-replay rows in that LDS when k_render_dense ran (else 0).  All zero before the first launch. */
typedef struct trc_residency {
    uint32_t cu_count, block, waves, planned_per_cu, planned_with, per_cu;
    uint64_t lds_bytes;
    uint32_t lds_static_bytes, per_cu_block1280, dense_memo_rows, reserved;
} trc_residency;
trc_status trc_debug_last_residency(trc_ctx* ctx, trc_residency* out);

#ifdef __cplusplus
}
#endif
#endif /* TRACER_TEST_HOOKS_H */
