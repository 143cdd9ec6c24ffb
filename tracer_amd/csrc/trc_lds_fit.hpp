// trc_lds_fit.hpp -- two pieces of plain arithmetic, shared with a stand-alone CPU program (tests/test_lds_fit.py): how many workgroups
// a CU's LDS holds under a given allocation granule (trc_debug_last_residency reports it for 1280 bytes beside the runtime's answer,
// which counts bytes; the planner itself asks the runtime), and the one word that a 7-row primary-replay memo keeps material, side,
// tag and replay count in (render_block).  No HIP, no library: includes <stdint.h> only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TRC_FIT_FN __host__ __device__ __forceinline__
#else
#define TRC_FIT_FN inline
#endif

// Workgroups of `bytes` of LDS each that `lds_per_cu` bytes hold when LDS is granted in blocks of `granule` bytes: 6592 B is 24
// workgroups per 160 KB at 512 B and 21 at 1280 B.
TRC_FIT_FN uint32_t trc_lds_workgroups(uint32_t bytes, uint32_t granule, uint32_t lds_per_cu) {
    if (granule == 0u) return 0u;
    const uint32_t granted = (bytes + granule - 1u) / granule * granule;
    return granted ? lds_per_cu / granted : 0xFFFFFFFFu;
}

// The packed memo word (TRC_REPLAY_DENSE 7: trc_render_config.hpp).  Top two bits say what the column holds:
//   00  no record; bits 0..29 count the camera rays answered from the memo before the record was lost (kMemoNone of the 8-row layout)
//   01  a camera ray that ends its sample by itself (tag == kTagNone of the 8-row layout): its radiance is in the rows of p
//   1s  a hit: s = sn is gn (kMemoSameSide), bits 28..29 the tag's primitive type (a leaf's: 0..3), bits 20..27 the material,
//       bits 0..19 the tag's index.  A hit whose material or index needs more bits is not kept (the pixel walks, as for uv).
constexpr uint32_t kPackIndexBits = 20u, kPackMatBits = 8u, kPackTypeBits = 2u;
constexpr uint32_t kPackHit = 0x80000000u, kPackSameSide = 0x40000000u, kPackEnds = 0x40000000u;
constexpr uint32_t kPackCountMax = 0x3FFFFFFFu;      // replays a lost record can still report
constexpr uint32_t kPackMatMax = (1u << kPackMatBits) - 1u, kPackIndexMax = (1u << kPackIndexBits) - 1u;
static_assert(2u + kPackTypeBits + kPackMatBits + kPackIndexBits == 32u, "packed memo word: kind 2 + type 2 + material 8 + index 20 bits");
static_assert(kPackCountMax >= 65535u, "the replay count of a lost record");

TRC_FIT_FN bool trc_memo_packable(uint32_t material, uint32_t tag_type, uint32_t tag_index) {
    return material <= kPackMatMax && tag_type < (1u << kPackTypeBits) && tag_index <= kPackIndexMax;
}
TRC_FIT_FN uint32_t trc_memo_pack_hit(uint32_t material, bool same_side, uint32_t tag_type, uint32_t tag_index) {
    return kPackHit | (same_side ? kPackSameSide : 0u) | (tag_type << (kPackMatBits + kPackIndexBits)) | (material << kPackIndexBits) | tag_index;
}
TRC_FIT_FN uint32_t trc_memo_pack_none(uint32_t replays) { return replays < kPackCountMax ? replays : kPackCountMax; }
TRC_FIT_FN uint32_t trc_memo_pack_ends() { return kPackEnds; }
TRC_FIT_FN bool trc_memo_is_none(uint32_t w) { return (w >> 30) == 0u; }
TRC_FIT_FN bool trc_memo_is_ends(uint32_t w) { return (w >> 30) == 1u; }
TRC_FIT_FN bool trc_memo_is_hit(uint32_t w) { return (w & kPackHit) != 0u; }
TRC_FIT_FN uint32_t trc_memo_count(uint32_t w) { return w & kPackCountMax; }
TRC_FIT_FN bool trc_memo_same_side(uint32_t w) { return (w & kPackSameSide) != 0u; }
TRC_FIT_FN uint32_t trc_memo_material(uint32_t w) { return (w >> kPackIndexBits) & kPackMatMax; }
TRC_FIT_FN uint32_t trc_memo_tag_type(uint32_t w) { return (w >> (kPackMatBits + kPackIndexBits)) & ((1u << kPackTypeBits) - 1u); }
TRC_FIT_FN uint32_t trc_memo_tag_index(uint32_t w) { return w & kPackIndexMax; }
