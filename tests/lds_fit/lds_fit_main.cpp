// Stand-alone CPU program over tracer_amd/csrc/trc_lds_fit.hpp (tests/test_lds_fit.py): the LDS arithmetic and the packed memo word,
// exactly the functions the planner's records and the render kernels use, compiled by the host compiler.
//   lds_fit_main wg BYTES GRANULE LDS_PER_CU     -> workgroups per CU
//   lds_fit_main limits                          -> largest material, tag type, tag index and replay count the word holds
//   lds_fit_main hit MATERIAL SIDE TYPE INDEX    -> word is_none is_ends is_hit material side type index packable
//   lds_fit_main none COUNT | ends               -> word is_none is_ends is_hit count
//   lds_fit_main sweep                           -> one `hit` line per material x side x a few tags, `none` lines for counts 0 .. 65535
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "trc_lds_fit.hpp"

static void hit_line(uint32_t m, uint32_t side, uint32_t type, uint32_t index) {
    const uint32_t w = trc_memo_pack_hit(m, side != 0u, type, index);
    std::printf("hit %u %u %u %u -> %u %d %d %d %u %d %u %u %d\n", m, side, type, index, w, (int)trc_memo_is_none(w), (int)trc_memo_is_ends(w),
                (int)trc_memo_is_hit(w), trc_memo_material(w), (int)trc_memo_same_side(w), trc_memo_tag_type(w), trc_memo_tag_index(w),
                (int)trc_memo_packable(m, type, index));
}
static void state_line(const char* name, uint32_t arg, uint32_t w) {
    std::printf("%s %u -> %u %d %d %d %u\n", name, arg, w, (int)trc_memo_is_none(w), (int)trc_memo_is_ends(w), (int)trc_memo_is_hit(w), trc_memo_count(w));
}

int main(int argc, char** argv) {
    auto num = [&](int i) { return (uint32_t)std::strtoul(argv[i], nullptr, 0); };
    if (argc == 5 && !std::strcmp(argv[1], "wg")) { std::printf("%u\n", trc_lds_workgroups(num(2), num(3), num(4))); return 0; }
    if (argc == 2 && !std::strcmp(argv[1], "limits")) { std::printf("%u %u %u %u\n", kPackMatMax, (1u << kPackTypeBits) - 1u, kPackIndexMax, kPackCountMax); return 0; }
    if (argc == 6 && !std::strcmp(argv[1], "hit")) { hit_line(num(2), num(3), num(4), num(5)); return 0; }
    if (argc == 3 && !std::strcmp(argv[1], "none")) { state_line("none", num(2), trc_memo_pack_none(num(2))); return 0; }
    if (argc == 2 && !std::strcmp(argv[1], "ends")) { state_line("ends", 0u, trc_memo_pack_ends()); return 0; }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const uint32_t tags[][2] = {{0u, 0u}, {1u, 6u}, {2u, 2u}, {3u, kPackIndexMax}, {3u, 12345u}};
        for (uint32_t m = 0; m <= kPackMatMax; ++m)
            for (uint32_t side = 0; side < 2u; ++side)
                for (const auto& t : tags) hit_line(m, side, t[0], t[1]);
        for (uint32_t c = 0; c <= 65535u; ++c) state_line("none", c, trc_memo_pack_none(c));
        state_line("ends", 0u, trc_memo_pack_ends());
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of lds_fit_main.cpp\n");
    return 2;
}
