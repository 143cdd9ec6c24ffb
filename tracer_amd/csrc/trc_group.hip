// trc_group.hip -- multi-GPU: the RCCL loader, the three collectives (RCCL or the caller's table) and the trc_group_* compose
// family of the C ABI (tile reduce, sample shards, their pipelined forms).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "trc_ctx.hpp"

Rccl g_rccl;

// the one piece of process-wide state: resolved once, under a lock (contexts may be created from several threads)
static std::mutex g_rccl_lock;
bool trc_load_rccl(std::string& err) {
    std::lock_guard<std::mutex> guard(g_rccl_lock);
    Rccl& r = g_rccl;
    if (r.ready) return true;
    if (r.handle) { dlclose(r.handle); r = Rccl{}; }        // an earlier attempt found the library but not every symbol
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        r.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (r.handle) break;
    }
    if (!r.handle) { err = std::string("dlopen(librccl) failed: ") + dlerror(); return false; }
    r.GetUniqueId = (int (*)(void*))dlsym(r.handle, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(void**, int, IdBlob, int))dlsym(r.handle, "ncclCommInitRank");
    r.Reduce = (int (*)(const void*, void*, size_t, int, int, int, void*, hipStream_t))dlsym(r.handle, "ncclReduce");
    r.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.handle, "ncclAllReduce");
    r.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(r.handle, "ncclAllGather");
    r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(r.handle, "ncclSend");
    r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(r.handle, "ncclRecv");
    r.GroupStart = (int (*)())dlsym(r.handle, "ncclGroupStart");
    r.GroupEnd = (int (*)())dlsym(r.handle, "ncclGroupEnd");
    r.CommDestroy = (int (*)(void*))dlsym(r.handle, "ncclCommDestroy");
    r.GetErrorString = (const char* (*)(int))dlsym(r.handle, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.Reduce || !r.AllReduce || !r.AllGather || !r.CommDestroy) {
        err = "librccl: missing symbols";
        dlclose(r.handle);
        r = Rccl{};
        return false;
    }
    r.ready = true;
    return true;
}

// ----------------------------------------------------------------------- collectives: RCCL or the caller's table
namespace {

size_t dtype_bytes(int dtype) { return dtype == kNcclUint8 ? 1 : 4; }

std::string rccl_error(const char* what, int rc) {
    return std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
}

// host-staged table call: wait for the producers on `st`, bring `bytes` at `buf` to pinned host memory, let the caller's
// function work on it, put the result back (only where the collective defines one)
template <typename Call>
trc_status staged(trc_ctx* ctx, void* buf, size_t bytes, bool copy_back, hipStream_t st, const char* what, Call&& call) {
    if (bytes > ctx->h_stage_bytes) {
        if (ctx->h_stage) { (void)hipHostFree(ctx->h_stage); ctx->h_stage = nullptr; ctx->h_stage_bytes = 0; }
        HIP_TRY(ctx, hipHostMalloc(&ctx->h_stage, bytes, hipHostMallocDefault));
        ctx->h_stage_bytes = bytes;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_stage, buf, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const int rc = call(ctx->h_stage);
    if (rc != 0) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's collective returned " + std::to_string(rc));
    if (copy_back) {
        HIP_TRY(ctx, hipMemcpyAsync(buf, ctx->h_stage, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));          // the staging buffer is reused by the next collective
    }
    return TRC_OK;
}

}  // namespace

trc_status trc_coll_reduce(trc_ctx* ctx, void* buf, size_t count, int dtype, int op, int root, hipStream_t st, const char* what) {
    if (ctx->coll_active) {
        const trc_collectives& c = ctx->coll;
        if (!c.host_staged) {
            const int rc = c.reduce(c.user, buf, count, dtype, op, root, (void*)st);
            return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's collective returned " + std::to_string(rc));
        }
        return staged(ctx, buf, count * dtype_bytes(dtype), ctx->rank == root, st, what,
                      [&](void* h) { return c.reduce(c.user, h, count, dtype, op, root, nullptr); });
    }
    if (!ctx->comm) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + " before trc_group_init / trc_group_set_collectives");
    const int rc = g_rccl.Reduce(buf, buf, count, dtype, op, root, ctx->comm, st);      // in place on the root (sendbuff == recvbuff is allowed)
    return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, rccl_error(what, rc));
}

trc_status trc_coll_allreduce(trc_ctx* ctx, void* buf, size_t count, int dtype, int op, hipStream_t st, const char* what) {
    if (ctx->coll_active) {
        const trc_collectives& c = ctx->coll;
        if (!c.host_staged) {
            const int rc = c.allreduce(c.user, buf, count, dtype, op, (void*)st);
            return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's collective returned " + std::to_string(rc));
        }
        return staged(ctx, buf, count * dtype_bytes(dtype), true, st, what,
                      [&](void* h) { return c.allreduce(c.user, h, count, dtype, op, nullptr); });
    }
    if (!ctx->comm) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + " before trc_group_init / trc_group_set_collectives");
    const int rc = g_rccl.AllReduce(buf, buf, count, dtype, op, ctx->comm, st);
    return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, rccl_error(what, rc));
}

trc_status trc_coll_allgather(trc_ctx* ctx, void* buf, size_t bytes_per_rank, hipStream_t st, const char* what) {
    if (ctx->coll_active) {
        const trc_collectives& c = ctx->coll;
        if (!c.host_staged) {
            const int rc = c.allgather(c.user, buf, bytes_per_rank, (void*)st);
            return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's collective returned " + std::to_string(rc));
        }
        return staged(ctx, buf, bytes_per_rank * (size_t)ctx->nranks, true, st, what,
                      [&](void* h) { return c.allgather(c.user, h, bytes_per_rank, nullptr); });
    }
    if (!ctx->comm) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + " before trc_group_init / trc_group_set_collectives");
    const int rc = g_rccl.AllGather(static_cast<char*>(buf) + (size_t)ctx->rank * bytes_per_rank, buf, bytes_per_rank, kNcclUint8, ctx->comm, st);
    return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, rccl_error(what, rc));
}

extern "C" {
// ----------------------------------------------------------------------- multi-GPU (RCCL over xGMI)
trc_status trc_group_unique_id(uint8_t id[TRC_UNIQUE_ID_BYTES]) {
    if (!id) return TRC_ERR_INVALID_ARG;
    std::string err;
    if (!trc_load_rccl(err)) return TRC_ERR_RCCL;
    IdBlob blob;
    std::memset(&blob, 0, sizeof blob);
    if (g_rccl.GetUniqueId(&blob) != 0) return TRC_ERR_RCCL;
    std::memcpy(id, &blob, TRC_UNIQUE_ID_BYTES);
    return TRC_OK;
}

trc_status trc_group_init(trc_ctx* ctx, const uint8_t id[TRC_UNIQUE_ID_BYTES], int nranks, int rank) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return TRC_ERR_INVALID_ARG;
    std::string err;
    if (!trc_load_rccl(err)) return trc_fail(ctx, TRC_ERR_RCCL, err);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->comm) { g_rccl.CommDestroy(ctx->comm); ctx->comm = nullptr; }
    ctx->coll_active = false;
    IdBlob blob;
    std::memcpy(&blob, id, TRC_UNIQUE_ID_BYTES);
    int rc = g_rccl.CommInitRank(&ctx->comm, nranks, blob, rank);
    if (rc != 0) {
        ctx->comm = nullptr;
        return trc_fail(ctx, TRC_ERR_RCCL, std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"));
    }
    ctx->nranks = nranks; ctx->rank = rank;
    return TRC_OK;
}

trc_status trc_group_reduce_accum(trc_ctx* ctx, int root) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->grouped()) return trc_fail(ctx, TRC_ERR_RCCL, "trc_group_reduce_accum before trc_group_init / trc_group_set_collectives");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "no frame");
    if (root < 0 || root >= ctx->nranks) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t count = (size_t)ctx->width * ctx->height * 4;
    return trc_coll_reduce(ctx, ctx->d_accum, count, kNcclFloat, kNcclSum, root, ctx->stream, "reduce(sum) of the accumulator");
}

// Sample sharding (the alternative to tile sharding; the definition is in tracer_abi.h): the composed pixel is
// the rank-ORDERED sum of the ranks' accumulator texels over the number of sample groups.  Rank r owns the r-th of nranks
// equal pixel slices: all-to-all of the slices, k_fold_shards, gather (root) or all-gather (every rank) of the results.
__global__ void __launch_bounds__(256) k_fold_shards(const float4* __restrict__ in, float4* __restrict__ out, uint32_t n_px,
                                                     uint32_t slice_px, uint32_t nranks, float groups) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;
    float4 a = in[i];                                        // rank 0's texel starts the sum (not 0 + it: -0 stays -0)
    for (uint32_t p = 1; p < nranks; ++p) {
        const float4 b = in[(size_t)p * slice_px + i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    a.x /= groups; a.y /= groups; a.z /= groups; a.w /= groups;
    out[i] = a;
}

extern "C++" {
namespace {

// pixels of slice p when n_px pixels are cut into nranks slices of slice_px (the last ones may be short or empty)
inline size_t slice_count(size_t n_px, size_t slice_px, int p) {
    const size_t lo = std::min(n_px, (size_t)p * slice_px), hi = std::min(n_px, (size_t)(p + 1) * slice_px);
    return hi - lo;
}

// root >= 0: the composed frame lands in ctx->d_shard_out on the root; root < 0: on every rank.  `src` is left untouched.
trc_status compose_samples(trc_ctx* ctx, const float* src, int root, uint32_t groups, hipStream_t st, const char* what) {
    const int N = ctx->nranks, me = ctx->rank;
    const size_t n_px = (size_t)ctx->width * ctx->height;
    const size_t slice_px = (n_px + (size_t)N - 1) / (size_t)N;
    const size_t slice_f = slice_px * 4, slice_bytes = slice_px * 16, total_bytes = slice_bytes * (size_t)N;
    if (!ctx->d_shard_in || ctx->shard_px != slice_px || ctx->shard_nranks != N) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));
        if (ctx->d_composed == ctx->d_shard_out) ctx->d_composed = nullptr;     // never leave it pointing at freed memory (a failed hipMalloc below returns)
        (void)hipFree(ctx->d_shard_in); (void)hipFree(ctx->d_shard_out); ctx->d_shard_in = ctx->d_shard_out = nullptr;
        ctx->shard_px = 0; ctx->shard_nranks = 0;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_shard_in, total_bytes));
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_shard_out, total_bytes));
        // zero-filled in stream order with the first use (hipMemset runs on the NULL stream, which the context's
        // non-blocking streams do not wait for: it could land on top of the slices copied in below)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_shard_in, 0, total_bytes, st));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_shard_out, 0, total_bytes, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        ctx->shard_px = slice_px; ctx->shard_nranks = N;
    }
    const size_t mine = slice_count(n_px, slice_px, me);
    // 1. slice `me` of every rank's accumulator -> d_shard_in[p]
    if (ctx->coll_active) {
        const trc_collectives& c = ctx->coll;
        if (!c.alltoall || (root >= 0 ? !c.gather : !c.allgather))
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, std::string(what) + ": the collectives table has no alltoall / gather");
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_shard_in, src, n_px * 16, hipMemcpyDeviceToDevice, st));
        if (total_bytes > n_px * 16) HIP_TRY(ctx, hipMemsetAsync(reinterpret_cast<char*>(ctx->d_shard_in) + n_px * 16, 0, total_bytes - n_px * 16, st));
        if (!c.host_staged) {
            const int rc = c.alltoall(c.user, ctx->d_shard_in, slice_bytes, (void*)st);
            if (rc != 0) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's alltoall returned " + std::to_string(rc));
        } else {
            TRC_TRY(staged(ctx, ctx->d_shard_in, total_bytes, true, st, what, [&](void* h) { return c.alltoall(c.user, h, slice_bytes, nullptr); }));
        }
    } else {
        if (!ctx->comm) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + " before trc_group_init / trc_group_set_collectives");
        if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
            return trc_fail(ctx, TRC_ERR_UNSUPPORTED, std::string(what) + ": librccl has no ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd");
        if (mine) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_shard_in + (size_t)me * slice_f, src + (size_t)me * slice_f, mine * 16, hipMemcpyDeviceToDevice, st));
        int rc = g_rccl.GroupStart();
        for (int p = 0; p < N && rc == 0; ++p) {
            if (p == me) continue;
            const size_t theirs = slice_count(n_px, slice_px, p);
            if (theirs) rc = g_rccl.Send(src + (size_t)p * slice_f, theirs * 4, kNcclFloat, p, ctx->comm, st);
            if (rc == 0 && mine) rc = g_rccl.Recv(ctx->d_shard_in + (size_t)p * slice_f, mine * 4, kNcclFloat, p, ctx->comm, st);
        }
        const int rc_end = g_rccl.GroupEnd();
        if (rc != 0 || rc_end != 0) return trc_fail(ctx, TRC_ERR_RCCL, rccl_error(what, rc != 0 ? rc : rc_end));
    }
    // 2. fold the N texels of every pixel of the slice in rank order, divide by the number of sample groups
    if (mine) {
        hipLaunchKernelGGL(k_fold_shards, dim3((unsigned)((mine + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(ctx->d_shard_in),
                           reinterpret_cast<float4*>(ctx->d_shard_out + (size_t)me * slice_f), (uint32_t)mine, (uint32_t)slice_px, (uint32_t)N, (float)groups);
        HIP_TRY(ctx, hipGetLastError());
    }
    // 3. the composed slices to the root, or to everybody
    if (root < 0) return trc_coll_allgather(ctx, ctx->d_shard_out, slice_bytes, st, what);
    if (ctx->coll_active) {
        const trc_collectives& c = ctx->coll;
        if (!c.host_staged) {
            const int rc = c.gather(c.user, ctx->d_shard_out, slice_bytes, root, (void*)st);
            return rc == 0 ? TRC_OK : trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + ": the caller's gather returned " + std::to_string(rc));
        }
        return staged(ctx, ctx->d_shard_out, total_bytes, me == root, st, what, [&](void* h) { return c.gather(c.user, h, slice_bytes, root, nullptr); });
    }
    int rc = g_rccl.GroupStart();
    if (me == root) {
        for (int p = 0; p < N && rc == 0; ++p) {
            const size_t theirs = slice_count(n_px, slice_px, p);
            if (p != me && theirs) rc = g_rccl.Recv(ctx->d_shard_out + (size_t)p * slice_f, theirs * 4, kNcclFloat, p, ctx->comm, st);
        }
    } else if (mine) {
        rc = g_rccl.Send(ctx->d_shard_out + (size_t)me * slice_f, mine * 4, kNcclFloat, root, ctx->comm, st);
    }
    const int rc_end = g_rccl.GroupEnd();
    if (rc != 0 || rc_end != 0) return trc_fail(ctx, TRC_ERR_RCCL, rccl_error(what, rc != 0 ? rc : rc_end));
    return TRC_OK;
}

trc_status check_compose(trc_ctx* ctx, int root, uint32_t groups, const char* what) {
    if (!ctx->grouped()) return trc_fail(ctx, TRC_ERR_RCCL, std::string(what) + " before trc_group_init / trc_group_set_collectives");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "no frame");
    if (root >= ctx->nranks) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(what) + ": root");
    if (groups < 1 || (uint32_t)ctx->nranks % groups != 0) return trc_fail(ctx, TRC_ERR_INVALID_ARG, std::string(what) + ": nranks is not sample_groups x tile ranks");
    return TRC_OK;
}

}  // namespace
}  // extern "C++"

uint64_t trc_shard_seed(uint64_t seed, uint32_t sample_group) { return seed + (uint64_t)sample_group * 0x9E3779B97F4A7C15ull; }

trc_status trc_group_compose_samples(trc_ctx* ctx, int root, uint32_t sample_groups) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || root < 0) return TRC_ERR_INVALID_ARG;
    if (sample_groups == 0) sample_groups = (uint32_t)ctx->nranks;
    TRC_TRY(check_compose(ctx, root, sample_groups, "trc_group_compose_samples"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));    // an earlier pipelined compose still owns the slice buffers
    TRC_TRY(compose_samples(ctx, ctx->d_accum, root, sample_groups, ctx->stream, "compose of the sample shards"));
    ctx->d_composed = ctx->rank == root ? ctx->d_shard_out : nullptr;      // the composed frame exists on the root only
    return TRC_OK;
}

trc_status trc_group_allreduce_mean_accum(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    TRC_TRY(check_compose(ctx, -1, (uint32_t)ctx->nranks, "trc_group_allreduce_mean_accum"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));
    TRC_TRY(compose_samples(ctx, ctx->d_accum, -1, (uint32_t)ctx->nranks, ctx->stream, "compose of the sample shards"));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_accum, ctx->d_shard_out, (size_t)ctx->width * ctx->height * 16, hipMemcpyDeviceToDevice, ctx->stream));
    return TRC_OK;
}

// Pipelined variant: the reduce of the frame just rendered runs on a second stream while the context goes on
// rendering into its OTHER accumulator, so an xGMI ring reduce of a multi-view frame (265 MB at N = 8, ~6 ms)
// hides under the next step's render instead of adding to it.
extern "C++" {
namespace {
// the frame just rendered goes to the communication stream (`collective` is queued there), the context to its other accumulator
template <typename Collective>
trc_status compose_async(trc_ctx* ctx, Collective&& collective) {
    const size_t count = (size_t)ctx->width * ctx->height * 4;
    if (!ctx->comm_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_rendered, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_busy, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_busy_alt, hipEventDisableTiming));
    }
    if (!ctx->d_accum_alt) {
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_accum_alt, count * sizeof(float)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_accum_alt, 0, count * sizeof(float), ctx->stream));
        ctx->busy_alt = false;
    }
    // compose the current accumulator once everything queued so far on the render stream has finished
    HIP_TRY(ctx, hipEventRecord(ctx->ev_rendered, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_rendered, 0));
    TRC_TRY(collective());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_busy, ctx->comm_stream));
    ctx->busy = true;
    // swap accumulators (and their events); the render stream may touch the new current one only after ITS last compose
    std::swap(ctx->d_accum, ctx->d_accum_alt);
    std::swap(ctx->ev_busy, ctx->ev_busy_alt);
    std::swap(ctx->busy, ctx->busy_alt);
    if (ctx->busy) { HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_busy, 0)); ctx->busy = false; }
    return TRC_OK;
}
}  // namespace
}  // extern "C++"

trc_status trc_group_reduce_accum_async(trc_ctx* ctx, int root) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->grouped()) return trc_fail(ctx, TRC_ERR_RCCL, "trc_group_reduce_accum_async before trc_group_init / trc_group_set_collectives");
    if (!ctx->d_accum) return trc_fail(ctx, TRC_ERR_NO_FRAME, "no frame");
    if (root < 0 || root >= ctx->nranks) return TRC_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t count = (size_t)ctx->width * ctx->height * 4;
    float* frame = ctx->d_accum;
    trc_status s = compose_async(ctx, [&] { return trc_coll_reduce(ctx, frame, count, kNcclFloat, kNcclSum, root, ctx->comm_stream, "reduce(sum) of the accumulator"); });
    if (s == TRC_OK) ctx->d_composed = frame;
    return s;
}

trc_status trc_group_compose_samples_async(trc_ctx* ctx, int root, uint32_t sample_groups) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || root < 0) return TRC_ERR_INVALID_ARG;
    if (sample_groups == 0) sample_groups = (uint32_t)ctx->nranks;
    TRC_TRY(check_compose(ctx, root, sample_groups, "trc_group_compose_samples_async"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // Unlike the tile reduce (which composes IN the accumulator and therefore switches to the other one), the sample compose only
    // reads: it works on a SNAPSHOT of the accumulator (a 33 MB device copy: ~20 us) taken in render-stream order, so the rank
    // goes on accumulating in place -- a progressive host calls this after every trc_render and never clears.
    const size_t bytes = (size_t)ctx->width * ctx->height * 16;
    if (!ctx->comm_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_rendered, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_busy, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_busy_alt, hipEventDisableTiming));
    }
    if (!ctx->ev_snapshot_free) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_snapshot_free, hipEventDisableTiming));
    if (!ctx->d_shard_src) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_shard_src, bytes));
    if (ctx->snapshot_busy) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_snapshot_free, 0));      // the previous compose still reads it
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_shard_src, ctx->d_accum, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_rendered, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_rendered, 0));
    TRC_TRY(compose_samples(ctx, ctx->d_shard_src, root, sample_groups, ctx->comm_stream, "compose of the sample shards"));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_snapshot_free, ctx->comm_stream));
    ctx->snapshot_busy = true;
    ctx->d_composed = ctx->rank == root ? ctx->d_shard_out : nullptr;      // the composed frame exists on the root only
    return TRC_OK;
}

trc_status trc_download_composed(trc_ctx* ctx, float* rgba) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx || !rgba) return TRC_ERR_INVALID_ARG;
    if (!ctx->d_composed) return trc_fail(ctx, TRC_ERR_NO_FRAME, "trc_download_composed before trc_group_reduce_accum_async / trc_group_compose_samples");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->comm_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    TRC_TRY(trc_copy_to_host(ctx, rgba, ctx->d_composed, (size_t)ctx->width * ctx->height * 16, ctx->stream));
    return TRC_OK;
}

trc_status trc_group_finalize(trc_ctx* ctx) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (ctx->grouped()) {
        (void)hipSetDevice(ctx->device);
        if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->comm) g_rccl.CommDestroy(ctx->comm);
        ctx->comm = nullptr;
        ctx->coll_active = false;
    }
    ctx->nranks = 1; ctx->rank = 0;
    return TRC_OK;
}

trc_status trc_group_set_collectives(trc_ctx* ctx, const trc_collectives* table, int nranks, int rank) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!table) return trc_group_finalize(ctx);
    if (nranks < 1 || rank < 0 || rank >= nranks) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_group_set_collectives: rank / nranks");
    if (!table->reduce || !table->allreduce || !table->allgather) return trc_fail(ctx, TRC_ERR_INVALID_ARG, "trc_group_set_collectives: the table needs reduce, allreduce and allgather (alltoall / gather: only for sample shards)");
    TRC_TRY(trc_group_finalize(ctx));
    ctx->coll = *table;
    ctx->coll_active = true;
    ctx->nranks = nranks; ctx->rank = rank;
    return TRC_OK;
}

}  // extern "C"
