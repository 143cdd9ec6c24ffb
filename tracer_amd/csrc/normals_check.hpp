// normals_check.hpp -- what trc_recompute_normals (trc_normals.hip) decides on the host before it touches the device: whether the vertex
// range is acceptable, and how many low key bits the sort of the adjacency build has to look at.  Nothing of HIP is included, so a
// stand-alone CPU program (tests/test_normals_cpu.py's probe) calls the same code.
#pragma once

#include <cstdint>

// nullptr: vertices [first, first + count) lie within the scene's n_vertex.  Otherwise the reason.  first + count is never formed in
// 32 bits: it may wrap (trc_update_vertices' test).  An empty range names no vertex and is acceptable wherever it starts: the call
// returns TRC_OK for count == 0 before it looks at first
inline const char* trc_normals_range_check(uint32_t first, uint32_t count, uint32_t n_vertex) {
    if (count == 0) return nullptr;
    if (first > n_vertex || count > n_vertex - first) return "first + count > n_vertex";
    return nullptr;
}

// the key bits that tell the vertex indices 0 .. n_vertex - 1 apart, at least 1: the adjacency build sorts the corners by their vertex
// with the tree builds' radix sort, 8 bits per pass, and a mesh of 2 601 vertices needs two of its four passes
inline uint32_t trc_normals_key_bits(uint32_t n_vertex) {
    uint32_t bits = 1;
    while (bits < 32u && ((n_vertex - (n_vertex ? 1u : 0u)) >> bits) != 0u) ++bits;
    return bits;
}
