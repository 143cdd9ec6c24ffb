// trc_refit.hpp -- what the three units of moving geometry call of one another: trc_refit.hip (new vertices by copy, the refit, the
// state's lifetime), trc_deform.hip (vertices computed on the device: pose, skin, morph) and trc_normals.hip (normals re-derived).  A
// call that moves vertices is  trc_enter_scene; its own checks; trc_refit_begin; its uploads; trc_scene_changed; trc_refit_open; its
// kernel; trc_refit_tail.  The state is trc_ctx::refit (trc_ctx.hpp: RefitState)
#pragma once

#include "trc_ctx.hpp"

constexpr uint32_t kPoseCountWord = 8;      // word of RefitState::Maps::d_root that counts the overflows of every pose, skin and morph
inline uint32_t* trc_overflow_counter(trc_ctx* ctx) { return reinterpret_cast<uint32_t*>(ctx->refit.maps.d_root) + kPoseCountWord; }

// What every entry point of the family opens with; `who` names it.  What follows differs between them and stays with each
inline trc_status trc_enter_scene(trc_ctx* ctx, const char* who) {
    TRC_TRY(trc_flush(ctx));
    if (!ctx) return TRC_ERR_INVALID_ARG;
    if (!ctx->has_scene) return trc_fail(ctx, TRC_ERR_NO_SCENE, std::string(who) + ": no scene");
    return TRC_OK;
}
// trc_refit.hip:
trc_status trc_refit_events(trc_ctx* ctx, const char* who);      // RefitState::ev, once per scene
// what a call does before anything changes: the pinned read-back buffer, the maps of the uploaded tree (behind whatever the stream
// still holds; the only part of a call that waits for the device, once per scene and tree), the events
trc_status trc_refit_begin(trc_ctx* ctx, const char* who);
trc_status trc_rest_ensure(trc_ctx* ctx, const char* what);      // RefitState::d_rest: d_verts as the first pose, skin or morph of a scene finds them
inline trc_status trc_refit_open(trc_ctx* ctx) { HIP_TRY(ctx, hipEventRecord(ctx->refit.ev[0], ctx->stream)); return TRC_OK; }      // the start event, in front of the call's kernels
trc_status trc_refit_close(trc_ctx* ctx);                        // a launch of theirs that failed, else the stop event behind them: the time is to be read
// k_refit_triangles: the 48 B and 64 B records of the triangles that name a vertex of [first, first + count) from d_verts
void trc_refit_launch_triangles(trc_ctx* ctx, uint32_t first, uint32_t count);
// ... and behind the call's vertices, on the context's stream: those records, every box of the tree, trc_refit_close, the root box on
// its way back (with the overflow counter where `counted`: a kernel ran in front that counts).  Where the range is a hull, a triangle
// of the hull that no vertex of the call touched gets the bits it had, and keeps its material
trc_status trc_refit_tail(trc_ctx* ctx, uint32_t first, uint32_t count, bool counted);
trc_status trc_refit_read_time(trc_ctx* ctx);                    // RefitState::ms from the event pair if it is still to be read; waits for the stop event
