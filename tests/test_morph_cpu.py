"""trc_morph_bind / trc_morph_vertices on the CPU: the ABI names them without a new version number, the definition (tests/morph_ref.py)
can be told from its near misses on exactly the tables, weights and rest vertices the GPU tests use, the host's compaction of the
weights (tracer_amd/csrc/morph_check.hpp) is the definition's active list, and a tree refitted around morphed vertices bounds them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import morph_ref as mr
import refit_ref as rr
from conftest import random_rays
from oracle import pyoracle
from test_pose_cpu import small_ball
from test_skin_cpu import bindings, rest_of
from tracer_amd import abi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = (1, 3, 33)              # 33: past the kernel's unroll factor of four, with a remainder of one
# the rest vertices whose nx the GPU tests set to -0 through trc_update_vertices: inside both bindings of the residence
PLANTED = {"lds": (5, 6, 7), "mem": (70, 71, 72)}


def planted_rest(residence):
    v = rest_of(residence).copy()
    v[list(PLANTED[residence]), 3] = F(-0.0)
    return v


_DELTAS = {}


def deltas_of(count, n_targets):
    if (count, n_targets) not in _DELTAS:
        _DELTAS[count, n_targets] = mr.deltas(n_targets, count)
    return _DELTAS[count, n_targets]


CASES = [(r, f, c, nt, kind) for r in ("lds", "mem") for f, c in bindings(r) for nt in TARGETS for kind in mr.WEIGHT_KINDS]


def test_abi_names_morph_vertices():
    for name in ("trc_morph_bind", "trc_morph_vertices"):
        assert name in abi.DEVICE_SYMBOLS, name
    assert abi.TRC_ABI_VERSION == 13                                  # an addition under 13: the number stays
    assert C.sizeof(abi.MorphDelta) == 24 and abi.MorphDelta.dn.offset == 12
    assert abi.TRC_MORPH_MAX_TARGETS == mr.MAX_TARGETS == 1024
    header = open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
    assert re.search(r"#define\s+TRC_MORPH_MAX_TARGETS\s+1024u", header)
    assert re.search(r"#define\s+TRC_ABI_VERSION\s+13\b", header)
    for name in ("trc_morph_bind", "trc_morph_vertices"):
        assert re.search(r"trc_status\s+" + name + r"\s*\(", header), name


# ---------------------------------------------------------------------------------------------------- near misses
def contracted(rest6, d, w):
    """acc = fma(w, d, acc): the product is exact in float64, one rounding per target"""
    acc = rest6.copy()
    for k, wk in mr.active(w):
        acc = (np.float64(wk) * d[k].astype(np.float64) + acc.astype(np.float64)).astype(F)
    return acc


def deltas_first(rest6, d, w):
    """the weighted deltas summed among themselves, the rest values added last"""
    total = None
    for k, wk in mr.active(w):
        p = wk * d[k]
        total = p if total is None else total + p
    return rest6.copy() if total is None else rest6 + total


def descending(rest6, d, w):
    acc = rest6.copy()
    for k, wk in reversed(mr.active(w)):
        p = wk * d[k]
        acc = acc + p
    return acc


def in_double(rest6, d, w):
    """float64 accumulation, rounded once at the end"""
    acc = rest6.astype(np.float64)
    for k, wk in mr.active(w):
        acc = acc + np.float64(wk) * d[k].astype(np.float64)
    return acc.astype(F)


def zeros_multiplied(rest6, d, w):
    """every target takes part, the ones with a weight of zero included: -0 + (+0 * d) is +0"""
    acc = rest6.copy()
    for k in range(len(w)):
        p = w[k] * d[k]
        acc = acc + p
    return acc


def applicable(n_active, n_zero):
    """The near misses that CAN differ from the definition on weights with n_active non-zero and n_zero zero entries.  With one active
    target there is one product and one sum: no order to get wrong, and the sum of the deltas is the delta.  A multiplied zero weight
    adds +-0, which changes a value only where that value is a -0 still: with an active target in front the planted -0 has become
    w * d already, so this near miss is told apart on the all-zero weights, where the definition returns the rest bits."""
    out = []
    if n_active >= 1:
        out += [contracted, in_double]
    if n_active >= 2:
        out += [deltas_first, descending]
    if n_active == 0 and n_zero >= 1:
        out += [zeros_multiplied]
    return out


@pytest.mark.parametrize("residence,first,count,n_targets,kind", CASES)
def test_the_test_data_tell_the_definition_from_its_near_misses(residence, first, count, n_targets, kind):
    v0 = planted_rest(residence)
    assert len(v0) > 700 if residence == "mem" else len(v0) > 18
    d, w = deltas_of(count, n_targets), mr.weights(n_targets, kind)
    assert mr.valid_binding(first, d, len(v0)) and mr.valid_weights(w, n_targets)
    act = mr.active(w)
    n_zero = n_targets - len(act)
    assert [k for k, _ in act] == sorted(k for k, _ in act) and all(wk != 0 for _, wk in act)
    if kind == "zero":
        assert len(act) == 0 and not np.signbit(w).all() and (n_targets == 1 or np.signbit(w).any())      # both zeros
    elif kind == "alternating":
        assert len(act) == (n_targets + 1) // 2 and (n_targets < 4 or np.signbit(w[w == 0]).any())
    else:
        assert n_zero == 0 and ((w < 0).any() == (kind == "negative"))
    planted = [p - first for p in PLANTED[residence]]
    assert all(0 <= p < count for p in planted)
    rest6 = v0[first:first + count, :6]
    assert np.signbit(rest6[planted, 3]).all() and (rest6[planted, 3] == 0).all()
    want = mr.morph(v0, v0, first, d, w)[first:first + count]
    assert want.dtype == F and np.array_equal(want[:, 6:].view(np.uint32), v0[first:first + count, 6:].view(np.uint32))
    if act:
        assert (want[:, :6].view(np.uint32) != rest6.view(np.uint32)).any(axis=1).all()       # every bound vertex moves
    else:
        assert np.array_equal(want.view(np.uint32), v0[first:first + count].view(np.uint32))   # the rest bits, the -0 included
    assert np.abs(want[:, :3]).max() < 1e4
    misses = applicable(len(act), n_zero)
    assert misses
    for near_miss in misses:
        got = near_miss(rest6.copy(), d, w)
        assert got.dtype == F and np.allclose(got, want[:, :6], rtol=1e-4, atol=1e-3), near_miss.__name__       # near ...
        assert (got.view(np.uint32) != want[:, :6].view(np.uint32)).any(), near_miss.__name__                    # ... and a miss


def test_every_near_miss_is_told_apart_somewhere():
    seen = set()
    for _, _, _, nt, kind in CASES:
        w = mr.weights(nt, kind)
        n_active = len(mr.active(w))
        seen.update(f.__name__ for f in applicable(n_active, nt - n_active))
    assert seen == {"contracted", "deltas_first", "descending", "in_double", "zeros_multiplied"}


# ---------------------------------------------------------------------------------------------------- the host's compaction
PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "morph_check.hpp"
// argv: n_targets, then the weights as 8 hex digits each.  Prints "refused" or one "target weight-bits" line per active entry
int main(int argc, char** argv) {
    const uint32_t n_targets = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    std::vector<float> w;
    for (int i = 2; i < argc; ++i) { const uint32_t u = (uint32_t)std::strtoul(argv[i], nullptr, 16); float f; std::memcpy(&f, &u, 4); w.push_back(f); }
    std::vector<trc_morph_active> active(3, trc_morph_active{99u, 1.0f});      // what it held before is gone either way
    if (trc_morph_weights_check(w.empty() ? nullptr : w.data(), (uint32_t)w.size(), n_targets, active)) { std::printf("refused %zu\n", active.size()); return 0; }
    for (const trc_morph_active& a : active) { uint32_t u; std::memcpy(&u, &a.weight, 4); std::printf("%u %08x\n", a.target, u); }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("morph_check")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])

    def run(n_targets, w):
        words = [f"{u:08x}" for u in np.asarray(w, dtype=F).view(np.uint32)]
        return subprocess.run([str(exe), str(n_targets), *words], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")[:-1]
    return run


def test_compaction_is_the_definition_s_active_list(probe):
    for nt in TARGETS + (8,):
        for kind in mr.WEIGHT_KINDS:
            w = mr.weights(nt, kind)
            want = [f"{k} {np.asarray(wk, F).view(np.uint32):08x}" for k, wk in mr.active(w)]
            assert probe(nt, w) == want, (nt, kind)
    tiny = np.array([0.0, 1e-45, -0.0, -1e-45], F)                     # a denormal is not zero
    assert probe(4, tiny) == ["1 00000001", "3 80000001"]
    assert probe(3, [1, 2]) == ["refused 0"] and probe(1, [1, 2]) == ["refused 0"] and probe(0, []) == ["refused 0"]      # off by one; NULL
    for bad in (np.nan, np.inf, -np.inf):
        assert probe(3, [0.5, 0, bad]) == ["refused 0"]


# ---------------------------------------------------------------------------------------------------- properties
def test_morph_is_from_rest_and_leaves_the_rest_alone():
    sc = small_ball()                      # kept alive: its view points into memory the scene owns
    v = rr.vertices_of(sc.view)
    d, w = mr.deltas(3, 5), mr.weights(3, "negative")
    current = v + F(1)
    got = mr.morph(v, current, 3, d, w)
    assert (got[:3] == current[:3]).all() and (got[8:] == current[8:]).all()
    assert (got[3:8] == mr.morph(v, v, 3, d, w)[3:8]).all() and (got[3:8, :6] != v[3:8, :6]).any(axis=1).all()
    assert np.array_equal(mr.morph(v, current, 3, d, mr.weights(3, "zero"))[3:8].view(np.uint32), v[3:8].view(np.uint32))


def test_valid_restates_the_refusals():
    d = mr.deltas(3, 6)
    assert mr.valid_binding(4, d, 10) and mr.valid_binding(99, d[:0], 10) and mr.valid_binding(99, d[:, :0], 10)
    assert not mr.valid_binding(5, d, 10) and not mr.valid_binding(0xFFFFFFFF, d, 10)
    for bad in (np.nan, np.inf, -np.inf):
        for c in (1, 4):
            d2 = d.copy(); d2[2, 3, c] = bad
            assert not mr.valid_binding(0, d2, 10)
    assert mr.valid_binding(0, np.zeros((mr.MAX_TARGETS, 1, 6), F), 10) and not mr.valid_binding(0, np.zeros((mr.MAX_TARGETS + 1, 1, 6), F), 10)
    assert mr.valid_weights([0, 1, -2], 3) and not mr.valid_weights([0, 1], 3) and not mr.valid_weights([0, 1, np.nan], 3)


def test_refitted_tree_bounds_the_morphed_mesh():
    """after a morph the oracle finds through the refitted tree what it finds without any tree"""
    sc = small_ball()
    v0 = rr.vertices_of(sc.view)
    v = mr.morph(v0, v0, 0, mr.deltas(3, len(v0)) * F(4), mr.weights(3, "negative"))
    moved = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)
    rays = random_rays(3000, 5, inside_only=True)
    a, c = pyoracle.trace_rays(moved.view, rays), pyoracle.trace_rays(moved.view, rays, brute=True)
    for f in ("hit", "pType", "pIndex", "t"):
        assert (a[f].view(np.uint32) == c[f].view(np.uint32)).all(), f
    assert (a["pType"][a["hit"] != 0] == abi.PRIM_TRIANGLE).any()
