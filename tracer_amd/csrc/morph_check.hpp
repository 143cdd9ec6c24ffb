// morph_check.hpp -- what trc_morph_bind and trc_morph_vertices (trc_deform.hip) refuse before they touch the device: the delta table of
// a binding and the weights of a frame, and the compaction of the weights into the ACTIVE LIST the kernels walk.  Nothing of HIP is
// included, so the sanitizer driver (tools/sanitize/driver.cpp) calls the same code with hostile input.  Every target index the kernel
// uses comes from the active list, which names only k < n_weights == the binding's n_targets <= TRC_MORPH_MAX_TARGETS.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "tracer_abi.h"

// one entry of the active list: a target whose weight is not zero.  8 bytes, read by the kernels with one scalar load
struct trc_morph_active { uint32_t target; float weight; };
static_assert(sizeof(trc_morph_active) == 8, "trc_morph_active");

// an empty table (it removes the binding): nothing of it is read, whatever the other arguments
inline bool trc_morph_table_empty(uint32_t n_targets, uint32_t count) { return n_targets == 0 || count == 0; }

// nullptr: the table is acceptable.  Otherwise the reason.  The range must end within n_vertex (first + count is never formed in 32
// bits: it may wrap), n_targets must not pass the cap -- refused before a delta is read -- and all six components of every delta must
// be finite.  The table holds n_targets * count records: the product is formed in size_t, it passes 2^32 for tables that are legal.
inline const char* trc_morph_table_check(const trc_morph_delta* deltas, uint32_t n_targets, uint32_t first, uint32_t count, uint32_t n_vertex) {
    if (trc_morph_table_empty(n_targets, count)) return nullptr;
    if (!deltas) return "deltas == NULL with a non-empty table";
    if (first > n_vertex || count > n_vertex - first) return "first + count > n_vertex";
    if (n_targets > TRC_MORPH_MAX_TARGETS) return "n_targets > TRC_MORPH_MAX_TARGETS";
    const size_t total = (size_t)n_targets * count;
    for (size_t r = 0; r < total; ++r)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(deltas[r].dv[c]) || !std::isfinite(deltas[r].dn[c])) return "a delta component that is not finite";
    return nullptr;
}

// nullptr: the weights are acceptable for a binding of n_targets targets, and `active` is the list of (k, weights[k]) for every
// weights[k] that is not zero (neither +0 nor -0 counts), k ascending.  Otherwise the reason, and `active` is empty.
inline const char* trc_morph_weights_check(const float* weights, uint32_t n_weights, uint32_t n_targets, std::vector<trc_morph_active>& active) {
    active.clear();
    if (!weights) return "weights == NULL";
    if (n_weights != n_targets) return "n_weights != the binding's n_targets";
    for (uint32_t k = 0; k < n_weights; ++k)
        if (!std::isfinite(weights[k])) return "a weight that is not finite";
    for (uint32_t k = 0; k < n_weights; ++k)
        if (weights[k] != 0.0f) active.push_back(trc_morph_active{k, weights[k]});
    return nullptr;
}
