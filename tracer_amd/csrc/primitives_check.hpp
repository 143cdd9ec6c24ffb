// primitives_check.hpp -- what trc_update_primitives (trc_primitives.hip) refuses before it touches the device: the three ranges and
// every field of a record that the repack kernel or the leaf-box arithmetic reads.  Nothing of HIP is included, so the sanitizer
// driver (tools/sanitize/driver.cpp) calls the same code with hostile tables.
#pragma once

#include <cmath>
#include <cstdint>

#include "tracer_abi.h"

constexpr float kPrimitiveValueBound = 1e37f;      // trc_update_vertices' bound on a position

inline bool trc_primitive_value_ok(float v) { return std::fabs(v) <= kPrimitiveValueBound; }      // false for a NaN too
inline bool trc_primitive_columns_ok(const trc_float4x4& m, int ncols) {                          // the xyz rows: what is read of a matrix
    for (int c = 0; c < ncols; ++c)
        if (!trc_primitive_value_ok(m.columns[c].x) || !trc_primitive_value_ok(m.columns[c].y) || !trc_primitive_value_ok(m.columns[c].z)) return false;
    return true;
}
inline bool trc_primitive_box_ok(const trc_AABB& b) {
    return trc_primitive_value_ok(b.mini.x) && trc_primitive_value_ok(b.mini.y) && trc_primitive_value_ok(b.mini.z) &&
           trc_primitive_value_ok(b.maxi.x) && trc_primitive_value_ok(b.maxi.y) && trc_primitive_value_ok(b.maxi.z);
}

// nullptr: the call is acceptable.  Otherwise the reason.  n_sphere, n_square, n_cube and n_material are the uploaded scene's counts;
// first + n is never formed in 32 bits (it may wrap).  A range with n == 0 is not looked at, whatever its pointer and its first.
inline const char* trc_primitive_ranges_check(const trc_primitive_ranges* r, uint32_t n_sphere, uint32_t n_square, uint32_t n_cube, uint32_t n_material) {
    if (!r) return "ranges == NULL";
    if (r->n_sphere != 0) {
        if (!r->spheres) return "spheres == NULL with n_sphere > 0";
        if (r->first_sphere > n_sphere || r->n_sphere > n_sphere - r->first_sphere) return "first_sphere + n_sphere > the scene's n_sphere";
    }
    if (r->n_square != 0) {
        if (!r->squares) return "squares == NULL with n_square > 0";
        if (r->first_square > n_square || r->n_square > n_square - r->first_square) return "first_square + n_square > the scene's n_square";
    }
    if (r->n_cube != 0) {
        if (!r->cubes) return "cubes == NULL with n_cube > 0";
        if (r->first_cube > n_cube || r->n_cube > n_cube - r->first_cube) return "first_cube + n_cube > the scene's n_cube";
    }
    for (uint32_t i = 0; i < r->n_sphere; ++i) {
        const trc_Sphere& s = r->spheres[i];
        if (s.material >= n_material) return "sphere material out of range";
        if (!trc_primitive_value_ok(s.radius) || !trc_primitive_value_ok(s.center.x) || !trc_primitive_value_ok(s.center.y) || !trc_primitive_value_ok(s.center.z) ||
            !trc_primitive_box_ok(s.boundingBOX) || !trc_primitive_columns_ok(s.model_matrix, 4))
            return "a sphere value that is not finite or beyond 1e37";
    }
    for (uint32_t i = 0; i < r->n_square; ++i) {
        const trc_Square& s = r->squares[i];
        if (s.material >= n_material) return "square material out of range";
        if (s.axis_i > 2 || s.axis_j > 2 || s.axis_k > 2) return "square axis out of range";
        if (!trc_primitive_value_ok(s.range_i.x) || !trc_primitive_value_ok(s.range_i.y) || !trc_primitive_value_ok(s.range_j.x) || !trc_primitive_value_ok(s.range_j.y) ||
            !trc_primitive_value_ok(s.value_k) || !trc_primitive_box_ok(s.boundingBOX) || !trc_primitive_columns_ok(s.model_matrix, 4))
            return "a square value that is not finite or beyond 1e37";
    }
    for (uint32_t i = 0; i < r->n_cube; ++i) {
        const trc_Cube& c = r->cubes[i];
        if (c.material >= n_material) return "cube material out of range";
        if (!trc_primitive_columns_ok(c.inverse_matrix, 4) || !trc_primitive_columns_ok(c.model_matrix, 4) || !trc_primitive_columns_ok(c.normal_matrix, 3) ||
            !trc_primitive_box_ok(c.box))
            return "a cube value that is not finite or beyond 1e37";
    }
    return nullptr;
}
