// trc_alias.hpp -- Vose's alias table, defined down to its order, as the builders of the light-sampling tables run it on the
// device (trc_envlight.hip: the environment map's rows and marginal; trc_meshlight.hip: the emissive triangles), so that a table
// is a function of its weights alone and the CPU restatements under tests/ can state it again:
// q_i = w_i n / sum in float64; worklists filled by ascending index; both are stacks (LIFO); a pair sets threshold(q_small) /
// alias = the large entry and q_large = (q_large + q_small) - 1; what is left on either list has probability 1 and is its own alias.
// threshold(q) = floor(q 2^32), 2^32 - 1 for q >= 1: an entry is kept when a 32-bit draw is below it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ inline uint32_t alias_threshold(double q) {
    return q >= 1.0 ? 0xFFFFFFFFu : (q <= 0.0 ? 0u : (uint32_t)(q * 4294967296.0));
}
// Vose's alias table of n weights w (sum = their float64 sum, ascending): q / list are n words of scratch each
template <class T>
__device__ inline void alias_vose(const T* w, uint32_t n, double sum, double* q, uint32_t* list, uint2* out) {
    for (uint32_t i = 0; i < n; ++i) q[i] = sum > 0.0 ? ((double)w[i] * (double)n) / sum : 1.0;
    uint32_t ns = 0, nl = 0;                    // small: list[0 .. ns), large: list[n - nl .. n), top at list[n - nl]
    for (uint32_t i = 0; i < n; ++i) {
        if (q[i] < 1.0) list[ns++] = i;
        else list[n - 1 - nl++] = i;
    }
    while (ns != 0 && nl != 0) {
        const uint32_t l = list[--ns];
        const uint32_t g = list[n - 1 - --nl];
        out[l] = make_uint2(alias_threshold(q[l]), g);
        q[g] = (q[g] + q[l]) - 1.0;
        if (q[g] < 1.0) list[ns++] = g;
        else list[n - 1 - nl++] = g;
    }
    while (nl != 0) { const uint32_t g = list[n - 1 - --nl]; out[g] = make_uint2(0xFFFFFFFFu, g); }
    while (ns != 0) { const uint32_t l = list[--ns]; out[l] = make_uint2(0xFFFFFFFFu, l); }
}
