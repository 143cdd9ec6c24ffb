"""The LDS arithmetic and the packed memo word of tracer_amd/csrc/trc_lds_fit.hpp, through a stand-alone CPU program
(tests/lds_fit/lds_fit_main.cpp) that the host compiler builds from the header the planner and the render kernels include.

Workgroups per CU: the headline scene's k_render_dense workgroup (staged scene 3008 B + 6 stack rows + memo rows of 256 B) under the
two allocation granules in question -- 512 B, which the launch plans used to assume, and 1280 B (320 dwords).  The packed word: what
the 7-row memo keeps in one row must come back out, and its three kinds (no record + replay count, a ray that ends its sample, a hit)
must never be mistaken for one another -- the 8-row layout told them apart by kMemoNone in one word and kTagNone in the other."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lds_fit") / "lds_fit_main"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tracer_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "lds_fit", "lds_fit_main.cpp")])
    return lambda *args: subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout


def _wg(prog, nbytes, granule):
    return int(prog("wg", nbytes, granule, LDS_PER_CU))


def test_the_headline_workgroup_under_both_granules(prog):
    assert 3008 + 6 * 256 + 8 * 256 == 6592 and 3008 + 6 * 256 + 7 * 256 == 6336 and 3008 + 6 * 256 == 4544
    assert _wg(prog, 6592, 512) == 24 and _wg(prog, 6592, 1280) == 21          # 8 memo rows: six waves per SIMD only if the granule is 512 B
    assert _wg(prog, 6336, 512) >= 24 and _wg(prog, 6336, 1280) >= 24          # 7 rows: 24 either way
    assert _wg(prog, 4544, 512) >= 24 and _wg(prog, 4544, 1280) >= 24          # no memo rows (before the replay; the memo in global memory)
    assert _wg(prog, 7680, 1280) == 21 and _wg(prog, 7681, 1280) == 18 and _wg(prog, 1, 1280) == 128      # whole granules
    assert _wg(prog, 5632, 512) == 29 and _wg(prog, 5632, 1280) == 25          # k_render at seven waves on a tree in memory plans for 28


def test_the_packed_memo_word_round_trips(prog):
    mat_max, type_max, index_max, count_max = map(int, prog("limits").split())
    assert mat_max >= 19 and type_max == 3 and count_max >= 65535              # Triangle.hh's material 19; leaf tag types 0 .. 3
    seen_hits, n_none = 0, 0
    for line in prog("sweep").splitlines():
        left, right = line.split(" -> ")
        kind, *args = left.split()
        out = [int(x) for x in right.split()]
        word, is_none, is_ends, is_hit = out[:4]
        assert is_none + is_ends + is_hit == 1, line                            # exactly one kind
        assert 0 <= word <= 0xFFFFFFFF
        if kind == "hit":
            m, side, typ, index = map(int, args)
            assert is_hit and out[4:8] == [m, side, typ, index] and out[8] == 1, line
            seen_hits += 1
        elif kind == "none":
            assert is_none and out[4] == int(args[0]), line                     # the replay count of a column that lost its record
            n_none += 1
        else:
            assert kind == "ends" and is_ends, line
    assert seen_hits == (mat_max + 1) * 2 * 5 and n_none == 65536
    # what the word cannot hold is refused (the kernel then keeps no record and the pixel walks), and a count saturates
    assert prog("hit", mat_max + 1, 0, 0, 0).split()[-1] == "0" and prog("hit", 0, 0, 0, index_max + 1).split()[-1] == "0"
    assert prog("hit", 0, 1, type_max + 1, 0).split()[-1] == "0"
    big = [int(x) for x in prog("none", 0xFFFFFFFF).split(" -> ")[1].split()]
    assert big[1:4] == [1, 0, 0] and big[4] == count_max
