// skin_check.hpp -- what trc_skin_bind and trc_skin_vertices (trc_deform.hip) refuse before they touch the device: the influence table
// of a binding and the bone palette of a frame.  Nothing of HIP is included, so the sanitizer driver (tools/sanitize/driver.cpp) calls
// the same code with hostile input.  Every bone index the kernel uses has passed both checks: an index of the table is below
// TRC_SKIN_MAX_BONES and at most *max_bone, and a palette is accepted only when it holds more bones than that.
#pragma once

#include <cmath>
#include <cstdint>

#include "tracer_abi.h"

// Palettes of up to this many bones are staged in LDS by k_skin_vertices_lds, seven 16-byte columns (112 B) per bone: 28 KiB of a
// CU's 160 KiB, so five workgroups of 256 threads still fit in a CU.  Larger palettes are gathered from global memory.
constexpr uint32_t kSkinLdsBones = 256;

// nullptr: the table is acceptable and *max_bone is the largest bone index it names (0 for an empty table).  Otherwise the reason, and
// *max_bone is not written.  The range must end within n_vertex (first + count is never formed in 32 bits: it may wrap), every
// weight must be finite and every bone index below TRC_SKIN_MAX_BONES, whatever its weight.
inline const char* trc_skin_influence_check(const trc_skin_influence* influences, uint32_t first, uint32_t count, uint32_t n_vertex, uint32_t* max_bone) {
    if (count == 0) { *max_bone = 0; return nullptr; }
    if (!influences) return "influences == NULL with count > 0";
    if (first > n_vertex || count > n_vertex - first) return "first + count > n_vertex";
    uint32_t largest = 0;
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 4; ++k) {
            if (!std::isfinite(influences[i].weight[k])) return "a weight that is not finite";
            if (influences[i].bone[k] >= TRC_SKIN_MAX_BONES) return "a bone index >= TRC_SKIN_MAX_BONES";
            if (influences[i].bone[k] > largest) largest = influences[i].bone[k];
        }
    *max_bone = largest;
    return nullptr;
}

// nullptr: a palette of n_bones > 0 bones is acceptable for a binding whose largest bone index is max_bone.  The 12 + 9 matrix
// entries that are read of every bone must be finite; the .w lanes and column 3 of the normal matrix may hold anything.
inline const char* trc_skin_palette_check(const trc_skin_bone* bones, uint32_t n_bones, uint32_t max_bone) {
    if (!bones) return "bones == NULL with n_bones > 0";
    if (n_bones > TRC_SKIN_MAX_BONES) return "n_bones > TRC_SKIN_MAX_BONES";
    if (n_bones <= max_bone) return "n_bones <= the binding's largest bone index";
    for (uint32_t i = 0; i < n_bones; ++i) {
        for (int c = 0; c < 4; ++c) {
            const trc_float4& m = bones[i].model_matrix.columns[c];
            if (!std::isfinite(m.x) || !std::isfinite(m.y) || !std::isfinite(m.z)) return "a model_matrix entry that is not finite";
        }
        for (int c = 0; c < 3; ++c) {
            const trc_float4& m = bones[i].normal_matrix.columns[c];
            if (!std::isfinite(m.x) || !std::isfinite(m.y) || !std::isfinite(m.z)) return "a normal_matrix entry that is not finite";
        }
    }
    return nullptr;
}
