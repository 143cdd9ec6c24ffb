// pose_ranges.hpp -- what trc_pose_vertices (trc_deform.hip) refuses before it touches the device: the range table and the matrix
// entries the kernel reads.  Nothing of HIP is included, so the sanitizer driver (tools/sanitize/driver.cpp) calls the same code
// with hostile tables.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "tracer_abi.h"

// nullptr: the table is acceptable and `order` holds the poses' indices sorted by `first`.  Otherwise the reason, and `order` is
// not to be used.  Every range must be non-empty and end within n_vertex (first + count is never formed in 32 bits: it may wrap),
// no two ranges may share a vertex, and the 12 + 9 matrix entries that are read must be finite.
inline const char* trc_pose_table_check(const trc_pose* poses, uint32_t n_poses, uint32_t n_vertex, std::vector<uint32_t>& order) {
    order.clear();
    if (n_poses == 0) return nullptr;
    if (!poses) return "poses == NULL with n_poses > 0";
    for (uint32_t i = 0; i < n_poses; ++i) {
        const trc_pose& p = poses[i];
        if (p.count == 0) return "a range with count == 0";
        if (p.first > n_vertex || p.count > n_vertex - p.first) return "first + count > n_vertex";
        for (int c = 0; c < 4; ++c) {
            const trc_float4& m = p.model_matrix.columns[c];
            if (!std::isfinite(m.x) || !std::isfinite(m.y) || !std::isfinite(m.z)) return "a model_matrix entry that is not finite";
        }
        for (int c = 0; c < 3; ++c) {
            const trc_float4& m = p.normal_matrix.columns[c];
            if (!std::isfinite(m.x) || !std::isfinite(m.y) || !std::isfinite(m.z)) return "a normal_matrix entry that is not finite";
        }
    }
    order.resize(n_poses);
    for (uint32_t i = 0; i < n_poses; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [poses](uint32_t a, uint32_t b) { return poses[a].first < poses[b].first; });
    for (uint32_t i = 1; i < n_poses; ++i) {
        const trc_pose &a = poses[order[i - 1]], &b = poses[order[i]];
        if (b.first - a.first < a.count) return "two ranges overlap";      // sorted: b.first >= a.first, and a.first + a.count <= n_vertex
    }
    return nullptr;
}
