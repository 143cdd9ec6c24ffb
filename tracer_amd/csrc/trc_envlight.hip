// trc_envlight.hip -- the sampling tables of the environment map as a light (TRC_FLAG_ENV_LIGHT, tracer_abi.h; sampled by
// dev_envlight.hpp in the k_render*_env kernels).  Built once per map, at the first flagged render after trc_set_environment_map:
//   k_env_weights   one thread per cell: the largest luminance among the texels the bilinear lookup can read inside the cell
//                   (3 x 3, clamped at the edges; negative or non-finite texels count 0) times cos(latitude of the cell centre)
//   k_env_rows      one lane per row: the row's sum and its alias table (Vose, float64)
//   k_env_marginal  one lane: the total and the alias table over the rows' sums
// Vose's method here is defined down to its order, so that the tables are a function of the map alone and tests/envlight_ref can
// restate them: q_i = w_i n / sum in float64; worklists filled by ascending index; both are stacks (LIFO); a pair sets
// threshold(q_small) / alias = the large entry and q_large = (q_large + q_small) - 1; what is left on either list has probability 1
// and is its own alias.  threshold(q) = floor(q 2^32), 2^32 - 1 for q >= 1: an entry is kept when a 32-bit draw is below it.
#include "trc_alias.hpp"
#include "trc_ctx.hpp"

#include <cfloat>

namespace {

__global__ void __launch_bounds__(256) k_env_weights(const float* rgb, uint32_t W, uint32_t H, float* weight) {
    const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= (size_t)W * H) return;
    const uint32_t i = (uint32_t)(c % W), j = (uint32_t)(c / W);
    float m = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const uint32_t y = (uint32_t)min(max((int)j + dy, 0), (int)H - 1);
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t x = (uint32_t)min(max((int)i + dx, 0), (int)W - 1);
            const float* t = rgb + 3 * ((size_t)y * W + x);
            float lum = rgb_to_y(f3(t[0], t[1], t[2]));
            if (!(lum > 0.0f && lum <= FLT_MAX)) lum = 0.0f;
            m = fmaxf(m, lum);
        }
    }
    const float cl = dm_cosf(kPi * (((float)j + 0.5f) / (float)H - 0.5f));
    weight[c] = m * fmaxf(cl, 0.0f);
}

__global__ void __launch_bounds__(64) k_env_rows(const float* weight, uint32_t W, uint32_t H, double* q, uint32_t* list, uint2* rows, double* rowsum) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= H) return;
    const size_t o = (size_t)j * W;
    double sum = 0.0;
    for (uint32_t i = 0; i < W; ++i) sum += (double)weight[o + i];
    rowsum[j] = sum;
    alias_vose(weight + o, W, sum, q + o, list + o, rows + o);
}

__global__ void __launch_bounds__(64) k_env_marginal(const double* rowsum, uint32_t H, double* q, uint32_t* list, uint2* marg, double* total) {
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (uint32_t j = 0; j < H; ++j) sum += rowsum[j];
    *total = sum;
    alias_vose(rowsum, H, sum, q, list, marg);
}

// byte offsets in the one allocation of the tables: rows (W H uint2), marg (H uint2), total (double), weight (W H float)
struct EnvLayout { size_t rows, marg, total, weight, bytes; };
EnvLayout env_layout(uint32_t W, uint32_t H) {
    EnvLayout l;
    const size_t n = (size_t)W * H;
    l.rows = 0; l.marg = n * 8; l.total = l.marg + (size_t)H * 8; l.weight = l.total + 8; l.bytes = l.weight + n * 4;
    return l;
}

}  // namespace

trc_status trc_env_light_build(trc_ctx* ctx) {
    if (ctx->d_envl) return TRC_OK;
    if (!ctx->d_envmap) return trc_fail(ctx, TRC_ERR_UNSUPPORTED, "TRC_FLAG_ENV_LIGHT: no environment map (trc_set_environment_map)");
    const uint32_t W = ctx->env_w, H = ctx->env_h;
    const size_t n = (size_t)W * H;
    const EnvLayout L = env_layout(W, H);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf tables, scratch;                         // scratch: q (float64) and the worklist per cell, the rows' sums, then the same for the marginal
    TRC_TRY(tables.alloc(ctx, L.bytes, "environment-light tables"));
    TRC_TRY(scratch.alloc(ctx, n * 12 + (size_t)H * 20, "environment-light table scratch"));
    uint8_t* const t = tables.as<uint8_t>();
    double* q = scratch.as<double>();
    double* rowsum = q + n;
    double* qm = rowsum + H;
    uint32_t* list = reinterpret_cast<uint32_t*>(qm + H);
    uint32_t* listm = list + n;
    float* weight = reinterpret_cast<float*>(t + L.weight);
    uint2* rows = reinterpret_cast<uint2*>(t + L.rows);
    uint2* marg = reinterpret_cast<uint2*>(t + L.marg);
    double* total = reinterpret_cast<double*>(t + L.total);
    TimedSection timed(ctx, ctx->stream);
    hipLaunchKernelGGL(k_env_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_envmap, W, H, weight);
    hipLaunchKernelGGL(k_env_rows, dim3((H + 63) / 64), dim3(64), 0, ctx->stream, weight, W, H, q, list, rows, rowsum);
    hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(64), 0, ctx->stream, rowsum, H, qm, listm, marg, total);
    timed.stop();
    double h_total = 0.0;
    TRC_TRY(trc_read_to_host(ctx, ctx->stream, "environment-light tables", {{&h_total, total, sizeof h_total}}));
    ctx->d_envl = static_cast<uint8_t*>(tables.release());
    ctx->envl_total = h_total;
    ctx->envl_build_ms = timed.ms();
    return TRC_OK;
}

void trc_env_light_free(trc_ctx* ctx) {
    if (ctx->d_envl) (void)hipFree(ctx->d_envl);
    ctx->d_envl = nullptr;
    ctx->envl_total = 0.0;
}

EnvLight trc_env_light_view(const trc_ctx* ctx) {
    const EnvLayout L = env_layout(ctx->env_w, ctx->env_h);
    EnvLight el{};
    el.rows = reinterpret_cast<const uint2*>(ctx->d_envl + L.rows);
    el.marg = reinterpret_cast<const uint2*>(ctx->d_envl + L.marg);
    el.weight = reinterpret_cast<const float*>(ctx->d_envl + L.weight);
    el.w = ctx->env_w; el.h = ctx->env_h;
    const bool lit = ctx->envl_total > 0.0;
    el.scale = lit ? (float)((double)ctx->env_w * (double)ctx->env_h / ctx->envl_total) : 0.0f;
    el.squares = ctx->ks.sc.n_squares >= 7 ? 1u : 0u;
    el.p_env = !lit ? 0.0f : (el.squares ? 0.5f : 1.0f);
    return el;
}

#ifdef TRC_TEST_HOOKS
namespace {
// the kernels' sampler and pdf (dev_envlight.hpp), one lane per item
__global__ void __launch_bounds__(256) k_env_light_test(const EnvLight el, const uint32_t* draws, uint32_t n, float* dir_pdf,
                                                        const float* dirs, uint32_t m, float* pdf) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) {
        const uint32_t* d = draws + 6 * (size_t)k;
        float p;
        const F3 v = env_light_sample(el, d[0], d[1], d[2], d[3], __uint_as_float(d[4]), __uint_as_float(d[5]), p);
        float* o = dir_pdf + 4 * (size_t)k;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = p;
    }
    if (k < m) pdf[k] = env_light_pdf(el, f3(dirs[3 * (size_t)k], dirs[3 * (size_t)k + 1], dirs[3 * (size_t)k + 2]));
}
}  // namespace

extern "C" {
trc_status trc_debug_env_tables(trc_ctx* ctx, float* weight, uint32_t* rows, uint32_t* marg, double* total, float* build_ms) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    TRC_TRY(trc_env_light_build(ctx));
    const EnvLayout L = env_layout(ctx->env_w, ctx->env_h);
    const size_t n = (size_t)ctx->env_w * ctx->env_h;
    trc_status st = TRC_OK;
    if (weight && st == TRC_OK) st = trc_copy_to_host(ctx, weight, ctx->d_envl + L.weight, n * 4, ctx->stream);
    if (rows && st == TRC_OK) st = trc_copy_to_host(ctx, rows, ctx->d_envl + L.rows, n * 8, ctx->stream);
    if (marg && st == TRC_OK) st = trc_copy_to_host(ctx, marg, ctx->d_envl + L.marg, (size_t)ctx->env_h * 8, ctx->stream);
    if (total) *total = ctx->envl_total;
    if (build_ms) *build_ms = ctx->envl_build_ms;
    return st;
}

trc_status trc_env_light_test(trc_ctx* ctx, const uint32_t* draws, size_t n, float* dir_pdf, const float* dirs, size_t m, float* pdf) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || (n && (!draws || !dir_pdf)) || (m && (!dirs || !pdf))) return TRC_ERR_INVALID_ARG;
    if (n > 0x7FFFFFFFu / 6u || m > 0x7FFFFFFFu / 6u) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_env_light_test: too many items in one call");
    TRC_TRY(trc_env_light_build(ctx));
    if (n == 0 && m == 0) return TRC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d;           // (freeing it waits for whatever a failed step left in flight)
    TRC_TRY(d.alloc(ctx, n * (24 + 16) + m * (12 + 4), "environment-light test"));
    uint32_t* d_draws = d.as<uint32_t>();
    float* d_out = reinterpret_cast<float*>(d.as<uint8_t>() + n * 24);
    float* d_dirs = d_out + 4 * n;
    float* d_pdf = d_dirs + 3 * m;
    if (n) TRC_TRY(trc_copy_to_device(ctx, d_draws, draws, n * 24, ctx->stream));
    if (m) TRC_TRY(trc_copy_to_device(ctx, d_dirs, dirs, m * 12, ctx->stream));
    const size_t items = n > m ? n : m;
    hipLaunchKernelGGL(k_env_light_test, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx->stream, trc_env_light_view(ctx),
                       d_draws, (uint32_t)n, d_out, d_dirs, (uint32_t)m, d_pdf);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return trc_fail(ctx, TRC_ERR_HIP, std::string("trc_env_light_test: ") + hipGetErrorString(e));
    if (n) TRC_TRY(trc_copy_to_host(ctx, dir_pdf, d_out, n * 16, ctx->stream));
    if (m) TRC_TRY(trc_copy_to_host(ctx, pdf, d_pdf, m * 4, ctx->stream));
    return TRC_OK;
}
}  // extern "C"
#endif  // TRC_TEST_HOOKS
