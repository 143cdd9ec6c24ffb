// dev_trileaf.hpp -- the leaf box of a triangle as trc_abi.hip k_triangle_leaves writes it at an upload, as a function for the refit
// (trc_refit.hip).  The upload kernel keeps its own text, so that its code stays what it was; tests/test_gpu_update_vertices_single.py
// holds the two to the same bits (test_unchanged_vertices_leave_a_device_tree_as_it_was).
#pragma once

#include <cfloat>

#include "tracer_abi.h"

namespace trcdev {

// BVH::buildNode for a triangle (AAPLRenderer.mm:575-589 + BVH.hh:273-314): the box of the three vertices -- std::max({a, b, c}) /
// std::min({a, b, c}) keep the first of equals -- taken corner by corner through the identity matrix (column sums in the reference's
// order, so a -0 comes out as the host's arithmetic leaves it) into fmin / fmax from +-FLT_MAX (the second operand on a tie, as the
// host's minss / maxss).
__device__ __forceinline__ void triangle_leaf_box(const trc_TriangleVertex& a, const trc_TriangleVertex& b, const trc_TriangleVertex& c,
                                                  float mn[3], float mx[3]) {
    float ele[2][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float hi = a.v[k]; if (hi < b.v[k]) hi = b.v[k]; if (hi < c.v[k]) hi = c.v[k];
        float lo = a.v[k]; if (b.v[k] < lo) lo = b.v[k]; if (c.v[k] < lo) lo = c.v[k];
        ele[0][k] = lo; ele[1][k] = hi;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { mn[q] = FLT_MAX; mx[q] = -FLT_MAX; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float x = ele[i][0], y = ele[j][1], z = ele[k][2];
                const float w[3] = {1.0f * x + 0.0f * y + 0.0f * z + 0.0f * 1.0f, 0.0f * x + 1.0f * y + 0.0f * z + 0.0f * 1.0f,
                                    0.0f * x + 0.0f * y + 1.0f * z + 0.0f * 1.0f};
#pragma unroll
                for (int q = 0; q < 3; ++q) { mn[q] = mn[q] < w[q] ? mn[q] : w[q]; mx[q] = mx[q] > w[q] ? mx[q] : w[q]; }
            }
}

// BVH::buildNode for an analytic primitive (trc_host_build_node): the eight corners of `box` in the order i, j, k under the xyz rows
// of `m`, each row ((m0 * x + m1 * y) + m2 * z) + m3 * 1, into fmin / fmax from +-FLT_MAX with the second operand kept on a tie
__device__ __forceinline__ void primitive_leaf_box(const trc_AABB& box, const trc_float4x4& m, float mn[3], float mx[3]) {
    const float ele[2][3] = {{box.mini.x, box.mini.y, box.mini.z}, {box.maxi.x, box.maxi.y, box.maxi.z}};
    const float col[4][3] = {{m.columns[0].x, m.columns[0].y, m.columns[0].z}, {m.columns[1].x, m.columns[1].y, m.columns[1].z},
                             {m.columns[2].x, m.columns[2].y, m.columns[2].z}, {m.columns[3].x, m.columns[3].y, m.columns[3].z}};
#pragma unroll
    for (int q = 0; q < 3; ++q) { mn[q] = FLT_MAX; mx[q] = -FLT_MAX; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float x = ele[i][0], y = ele[j][1], z = ele[k][2];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float w = col[0][q] * x + col[1][q] * y + col[2][q] * z + col[3][q] * 1.0f;
                    mn[q] = mn[q] < w ? mn[q] : w; mx[q] = mx[q] > w ? mx[q] : w;
                }
            }
}

}  // namespace trcdev
