// trc_meshlight.hip -- the sampling tables of the mesh's emissive triangles as lights (TRC_FLAG_MESH_LIGHTS, tracer_abi.h; sampled by
// dev_meshlight.hpp in the k_render*_mesh kernels).  Built once per scene and triangle-material array, at the first flagged render after
// trc_upload_scene* / trc_upload_triangle_materials:
//   k_mesh_weights   one thread per triangle: its weight as a light, luminance(albedo) * area in float64, 0 when it is none or
//                    when trc_set_triangle_visibility hides it (the mask, where the scene has one)
//                    (dev_meshlight.hpp: mesh_light_weight; the material is dword 15 of the attribute record, 19 after a scene upload)
//   k_mesh_compact   one workgroup: the lights' triangle indices and weights, in triangle order (each thread counts, then writes, one
//                    contiguous chunk of the triangles; a scan over the counts in between)
//   k_mesh_alias     one lane: the float64 total, summed by ascending light index, and the alias table over the lights (trc_alias.hpp:
//                    Vose's method in its stated order).  One lane, as the environment map's marginal: a table of a million lights
//                    takes it on the order of a second, once per scene
//   k_mesh_pdf       one thread per triangle: pdfA = weight / (total * area), float64 rounded once to binary32; 0 for a triangle that
//                    is no light
// Nothing here depends on the order in which threads run, so the tables are a function of the scene alone; tests/meshlight_ref restates them.
#include "trc_alias.hpp"
#include "trc_ctx.hpp"

#include <cfloat>

namespace {

struct MeshScene { const uint32_t* blob; uint32_t off_tripos, off_triattr, off_materials, n_materials, n_tri; const uint8_t* vis; };      // vis: trc_set_triangle_visibility's mask (null: none)

__device__ double tri_weight(const MeshScene& ms, uint32_t t, float& area) {
    F3 v0, v1, v2;
    mesh_tri_load(ms.blob + ms.off_tripos, t, v0, v1, v2);
    area = mesh_tri_area(v0, v1, v2);
    if (ms.vis && !ms.vis[t]) return 0.0;      // a hidden triangle is no light
    const uint32_t m = ms.blob[ms.off_triattr + (size_t)t * kTriAttrDwords + 15u];
    if (m >= ms.n_materials) return 0.0;
    const uint32_t* mat = ms.blob + ms.off_materials + (size_t)m * kMaterialDwords;
    const float y = rgb_to_y(f3(__uint_as_float(mat[2]), __uint_as_float(mat[3]), __uint_as_float(mat[4])));
    return mesh_light_weight((int)mat[0] == kMatDiffuse, y, area);
}

__global__ void __launch_bounds__(256) k_mesh_weights(const MeshScene ms, double* w) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ms.n_tri) return;
    float area;
    w[t] = tri_weight(ms, t, area);
}

__global__ void __launch_bounds__(1024) k_mesh_compact(const double* w, uint32_t n_tri, uint32_t* tri, double* wl, uint32_t* count) {
    __shared__ uint32_t cnt[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n_tri + 1023u) / 1024u;
    const uint32_t lo = (uint32_t)min((uint64_t)tid * chunk, (uint64_t)n_tri), hi = (uint32_t)min((uint64_t)lo + chunk, (uint64_t)n_tri);
    uint32_t c = 0;
    for (uint32_t t = lo; t < hi; ++t) c += w[t] > 0.0 ? 1u : 0u;
    cnt[tid] = c;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {        // inclusive scan of the 1024 counts
        const uint32_t v = tid >= off ? cnt[tid - off] : 0u;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    uint32_t k = cnt[tid] - c;
    if (tid == 1023u) *count = cnt[1023];
    for (uint32_t t = lo; t < hi; ++t)
        if (w[t] > 0.0) { tri[k] = t; wl[k] = w[t]; ++k; }
}

__global__ void __launch_bounds__(64) k_mesh_alias(const double* wl, const uint32_t* count, double* q, uint32_t* list, uint2* alias, double* total) {
    if (threadIdx.x != 0) return;
    const uint32_t n = *count;
    double sum = 0.0;
    for (uint32_t k = 0; k < n; ++k) sum += wl[k];
    *total = sum;
    alias_vose(wl, n, sum, q, list, alias);
}

__global__ void __launch_bounds__(256) k_mesh_pdf(const MeshScene ms, const double* w, const double* total, float* pdfA) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ms.n_tri) return;
    float p = 0.0f;
    if (w[t] > 0.0) {
        F3 v0, v1, v2;
        mesh_tri_load(ms.blob + ms.off_tripos, t, v0, v1, v2);
        p = (float)(w[t] / (*total * (double)mesh_tri_area(v0, v1, v2)));
    }
    pdfA[t] = p;
}

// byte offsets in the one allocation of the tables (capacity: every triangle a light): total (double), count, alias (n uint2), tri (n), pdfA (n)
struct MeshLayout { size_t total, count, alias, tri, pdfA, bytes; };
MeshLayout mesh_layout(uint32_t n_tri) {
    MeshLayout l;
    l.total = 0; l.count = 8; l.alias = 16; l.tri = l.alias + (size_t)n_tri * 8; l.pdfA = l.tri + (size_t)n_tri * 4; l.bytes = l.pdfA + (size_t)n_tri * 4;
    return l;
}

}  // namespace

trc_status trc_mesh_light_build(trc_ctx* ctx) {
    if (ctx->mesh_built) return TRC_OK;
    const DScene& sc = ctx->ks.sc;
    const uint32_t n = sc.n_triangles;
    if (n == 0) { ctx->mesh_built = true; ctx->mesh_n_lights = 0; ctx->mesh_total = 0.0; return TRC_OK; }
    const MeshLayout L = mesh_layout(n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf tables, scratch;                         // scratch, per triangle: w, wl, q (float64) and the worklist
    TRC_TRY(tables.alloc(ctx, L.bytes, "mesh-light tables"));
    TRC_TRY(scratch.alloc(ctx, (size_t)n * 28, "mesh-light table scratch"));
    uint8_t* const t = tables.as<uint8_t>();
    double* w = scratch.as<double>();
    double* wl = w + n;
    double* q = wl + n;
    uint32_t* list = reinterpret_cast<uint32_t*>(q + n);
    double* total = reinterpret_cast<double*>(t + L.total);
    uint32_t* count = reinterpret_cast<uint32_t*>(t + L.count);
    const MeshScene ms{ctx->d_blob, sc.off_tripos, sc.off_triattr, sc.off_materials, sc.n_materials, n, ctx->d_vis};
    const unsigned grid = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_mesh_weights, dim3(grid), dim3(256), 0, ctx->stream, ms, w);
    hipLaunchKernelGGL(k_mesh_compact, dim3(1), dim3(1024), 0, ctx->stream, w, n, reinterpret_cast<uint32_t*>(t + L.tri), wl, count);
    hipLaunchKernelGGL(k_mesh_alias, dim3(1), dim3(64), 0, ctx->stream, wl, count, q, list, reinterpret_cast<uint2*>(t + L.alias), total);
    hipLaunchKernelGGL(k_mesh_pdf, dim3(grid), dim3(256), 0, ctx->stream, ms, w, total, reinterpret_cast<float*>(t + L.pdfA));
    struct { double total; uint32_t count, pad; } head = {0.0, 0u, 0u};
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "mesh-light tables", {{&head, t, sizeof head}}));
    ctx->d_meshl = static_cast<uint8_t*>(tables.release());
    ctx->mesh_n_lights = head.count;
    ctx->mesh_total = head.total;
    ctx->mesh_built = true;
    return TRC_OK;
}

void trc_mesh_light_free(trc_ctx* ctx) {
    if (ctx->d_meshl) (void)hipFree(ctx->d_meshl);
    ctx->d_meshl = nullptr;
    ctx->mesh_built = false;
    ctx->mesh_n_lights = 0;
    ctx->mesh_total = 0.0;
}

MeshLight trc_mesh_light_view(const trc_ctx* ctx) {
    MeshLight ml{};
    ml.squares = ctx->ks.sc.n_squares >= 7 ? 1u : 0u;
    if (ctx->d_meshl && ctx->mesh_n_lights) {
        const MeshLayout L = mesh_layout(ctx->ks.sc.n_triangles);
        ml.alias = reinterpret_cast<const uint2*>(ctx->d_meshl + L.alias);
        ml.tri = reinterpret_cast<const uint32_t*>(ctx->d_meshl + L.tri);
        ml.pdfA = reinterpret_cast<const float*>(ctx->d_meshl + L.pdfA);
        ml.n_lights = ctx->mesh_n_lights;
        ml.p_mesh = ctx->knobs.mesh_light_pick == 0 ? 0.0f : (ml.squares ? 0.5f : 1.0f);      // knob 0: the BSDF-only estimator (tracer_abi.h)
    }
    return ml;
}

#ifdef TRC_TEST_HOOKS
namespace {
// the kernels' sampler (dev_meshlight.hpp), one lane per item
__global__ void __launch_bounds__(256) k_mesh_light_test(const MeshLight ml, const uint32_t* tripos, const uint32_t* draws, const float* pos, uint32_t n,
                                                         uint32_t* tri, float* out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t* d = draws + 4 * (size_t)k;
    MeshSample s;
    mesh_light_sample(ml, tripos, d[0], d[1], __uint_as_float(d[2]), __uint_as_float(d[3]), f3(pos[3 * (size_t)k], pos[3 * (size_t)k + 1], pos[3 * (size_t)k + 2]), s);
    tri[k] = s.tri;
    float* o = out + 7 * (size_t)k;
    o[0] = s.p.x; o[1] = s.p.y; o[2] = s.p.z; o[3] = s.n.x; o[4] = s.n.y; o[5] = s.n.z; o[6] = s.pdfA;
}
}  // namespace

extern "C" {
trc_status trc_debug_mesh_light_tables(trc_ctx* ctx, uint32_t* alias, uint32_t* tri, float* pdfA, double* total, uint32_t* n_lights) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_debug_mesh_light_tables: no scene");
    TRC_TRY(trc_mesh_light_build(ctx));
    const uint32_t n_tri = ctx->ks.sc.n_triangles, n = ctx->mesh_n_lights;
    const MeshLayout L = mesh_layout(n_tri);
    trc_status st = TRC_OK;
    if (ctx->d_meshl) {
        if (alias && n && st == TRC_OK) st = trc_copy_to_host(ctx, alias, ctx->d_meshl + L.alias, (size_t)n * 8, ctx->stream);
        if (tri && n && st == TRC_OK) st = trc_copy_to_host(ctx, tri, ctx->d_meshl + L.tri, (size_t)n * 4, ctx->stream);
        if (pdfA && n_tri && st == TRC_OK) st = trc_copy_to_host(ctx, pdfA, ctx->d_meshl + L.pdfA, (size_t)n_tri * 4, ctx->stream);
    }
    if (total) *total = ctx->mesh_total;
    if (n_lights) *n_lights = n;
    return st;
}

trc_status trc_mesh_light_test(trc_ctx* ctx, const uint32_t* draws, const float* pos, size_t n, uint32_t* tri, float* out) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || (n && (!draws || !pos || !tri || !out))) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, "trc_mesh_light_test: no scene");
    if (n > 0x7FFFFFFFu / 7u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_mesh_light_test: too many items in one call");
    TRC_TRY(trc_mesh_light_build(ctx));
    if (ctx->mesh_n_lights == 0) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "trc_mesh_light_test: the scene has no light triangle");
    if (n == 0) return TRC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf buf;         // (freeing it waits for whatever a failed step left in flight)
    TRC_TRY(buf.alloc(ctx, n * (16 + 12 + 4 + 28), "mesh-light test"));
    uint8_t* const d = buf.as<uint8_t>();
    uint32_t* d_draws = reinterpret_cast<uint32_t*>(d);
    float* d_pos = reinterpret_cast<float*>(d + n * 16);
    uint32_t* d_tri = reinterpret_cast<uint32_t*>(d + n * 28);
    float* d_out = reinterpret_cast<float*>(d + n * 32);
    TRC_TRY(trc_copy_to_device(ctx, d_draws, draws, n * 16, ctx->stream));
    TRC_TRY(trc_copy_to_device(ctx, d_pos, pos, n * 12, ctx->stream));
    MeshLight ml = trc_mesh_light_view(ctx);
    hipLaunchKernelGGL(k_mesh_light_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ml, ctx->d_blob + ctx->ks.sc.off_tripos,
                       d_draws, d_pos, (uint32_t)n, d_tri, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_mesh_light_test: ") + hipGetErrorString(e));
    TRC_TRY(trc_copy_to_host(ctx, tri, d_tri, n * 4, ctx->stream));
    return trc_copy_to_host(ctx, out, d_out, n * 28, ctx->stream);
}
}  // extern "C"
#endif  // TRC_TEST_HOOKS
