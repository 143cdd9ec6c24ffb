"""trc_recompute_normals on the CPU: the ABI names it without a new version number, the definition (tests/normals_ref.py) can be told
from its near misses on exactly the meshes the GPU tests use, the vertices that keep their bits and the sums the side rule negates are
the planted ones, a range restricts what is written and not what is read, and the host's range check
(tracer_amd/csrc/normals_check.hpp) is the definition's.

The meshes: the two balls of test_gpu_update_vertices.scene ("lds": 35 vertices / 48 triangles, "mem": 2 601 / 5 000), whose valences
are 1, 2, 3 and 6 only, and normals_ref.fan ("fan": 74 / 72) with a hub of valence 70, a vertex no triangle names, two named by a
triangle of no area, one named twice by one triangle, and half of the rim wound against the stored normals.  All after refit_ref.twist.

One figure of the issue cannot hold as written: "the kept set is never more than 5 % of a mesh".  The kept set of the small ball is its
two poles, as the issue itself states, and 2 of 35 vertices are 5.7 %.  The test asserts the kept set itself for every mesh, vertex by
vertex, and the 5 % on the two meshes where the stated sets allow it (2 of 2 601, 3 of 74)."""
import os
import re
import subprocess

import numpy as np
import pytest

import normals_ref as nr
import refit_ref as rr
from test_gpu_update_vertices import scene
from test_skin_cpu import bindings
from tracer_amd import abi, host

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIST = (0.5, 0.9)
MESHES = ("lds", "mem", "fan")
_FAN = {}


def mesh_scene(name, analytic_leaves_only=False):
    """scene() of the GPU tests, and the fan placed in the same Cornell box; kept alive here: a view points into memory its scene owns"""
    if name != "fan":
        return scene(name, analytic_leaves_only)
    if analytic_leaves_only not in _FAN:
        v, i, _ = nr.fan()
        _FAN[analytic_leaves_only] = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.from_arrays(v, i), analytic_leaves_only=analytic_leaves_only)
    return _FAN[analytic_leaves_only]


def indices_of(name):
    return rr.indices_of(mesh_scene(name).view)


def rest_of(name):
    return rr.vertices_of(mesh_scene(name).view)


def twisted(name):
    return rr.twist(rest_of(name), *TWIST)


def ranges(name):
    """[(first, count)]: the ragged and the whole range of test_skin_cpu.bindings; the fan's as the small ball's (its hub, vertex 0, lies
    outside the ragged one and its triangles inside)"""
    if name != "fan":
        return bindings(name)
    n = len(rest_of(name))
    return [(3, n - 5), (0, n)]


def expected_kept(name):
    n = len(rest_of(name))
    if name != "fan":
        return [0, n - 1]                                       # the poles: valence 1, a triangle of no area each
    planted = nr.fan()[2]
    return sorted([planted["unnamed"], *planted["zero_area"]])


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_abi_names_recompute_normals():
    assert "trc_recompute_normals" in abi.DEVICE_SYMBOLS
    assert abi.TRC_ABI_VERSION == 13                                  # an addition under 13: the number stays
    header = open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
    assert re.search(r"#define\s+TRC_ABI_VERSION\s+13\b", header)
    assert re.search(r"trc_status\s+trc_recompute_normals\s*\(\s*trc_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+first\s*,\s*uint32_t\s+count\s*\)\s*;", header)
    assert re.search(r"added under 13, the number stays: trc_recompute_normals", header)


# ---------------------------------------------------------------------------------------------------- the data are not vacuous
def test_the_fan_is_what_it_says():
    v, idx, planted = nr.fan()
    val = nr.valences(idx, len(v))
    assert val[planted["hub"]] == nr.HUB_VALENCE == 70 > 64 and val[planted["unnamed"]] == 0
    tri = idx.reshape(-1, 3)
    for z in planted["zero_area"]:
        assert val[z] == 1 and not nr.face_terms(v, idx)[(tri == z).any(axis=1)].any()
    assert ((tri == planted["twice"]).sum(axis=1) == 2).sum() == 1
    assert len(planted["opposed"]) == 34 and planted["hub"] not in planted["opposed"]
    assert len(rest_of("fan")) == len(v) == 74 and np.array_equal(indices_of("fan"), idx)      # the scene keeps the order of both


@pytest.mark.parametrize("moved", [False, True], ids=["rest", "twisted"])
@pytest.mark.parametrize("name", MESHES)
def test_kept_set_flips_and_unit_length(name, moved):
    v, idx = twisted(name) if moved else rest_of(name), indices_of(name)
    n = len(v)
    assert (n, len(idx) // 3) == {"lds": (35, 48), "mem": (2601, 5000), "fan": (74, 72)}[name]
    want = nr.recompute(v, idx)
    assert want.dtype == F
    changed = (bits(want) != bits(v)).any(axis=1)
    kept = list(np.nonzero(~changed)[0])
    assert kept == expected_kept(name) == list(nr.kept(v, idx)), kept
    if name != "lds":
        assert len(kept) <= 0.05 * n                                  # (the small ball: 2 of 35, see the module's docstring)
    assert np.array_equal(bits(want[:, :3]), bits(v[:, :3])) and np.array_equal(bits(want[:, 6:]), bits(v[:, 6:]))
    assert (bits(want[changed, 3:6]) != bits(v[changed, 3:6])).any(axis=1).all()
    # unit length within 2 ulp: the length in float64 of the float32 normal against 1
    length = np.sqrt((want[changed, 3:6].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2 * np.finfo(F).eps
    flipped = nr.flipped(v, idx)
    if name == "fan":
        assert sorted(flipped) == sorted(nr.fan()[2]["opposed"])      # the half wound against its normals, and only that half
    else:
        assert sorted(flipped) == sorted(np.nonzero(changed)[0])      # Mesh.ball is wound against its normals everywhere
        unflipped = nr.recompute(v, idx, side_rule=False)
        cos = (unflipped[changed, 3:6].astype(np.float64) * want[changed, 3:6]).sum(axis=1)
        assert np.allclose(cos, -1.0, atol=1e-6)
    # ... and the new normal lies on the side of the one the vertex held
    assert ((want[changed, 3:6].astype(np.float64) * v[changed, 3:6]).sum(axis=1) > 0).all()


# ---------------------------------------------------------------------------------------------------- near misses
def fms(a, b, c, d):
    """fma(a, b, -(c * d)): the second product rounded, the first exact in float64, one rounding of the difference"""
    t = c * d
    return (a.astype(np.float64) * b.astype(np.float64) - t.astype(np.float64)).astype(F)


def contracted_terms(v, idx):
    e1, e2 = nr.edges(v, idx)
    c = np.empty_like(e1)
    c[:, 0] = fms(e1[:, 1], e2[:, 2], e1[:, 2], e2[:, 1])
    c[:, 1] = fms(e1[:, 2], e2[:, 0], e1[:, 0], e2[:, 2])
    c[:, 2] = fms(e1[:, 0], e2[:, 1], e1[:, 1], e2[:, 0])
    return c


def unit_terms(v, idx):
    """the face normals normalised before they are summed: every triangle weighs the same"""
    c = nr.face_terms(v, idx)
    l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return np.where(l[:, None] > 0, c / np.where(l > 0, l, F(1))[:, None], F(0)).astype(F)


def by_reciprocal_root(s):
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        l = np.sqrt(q)
        r = F(1) / l
        return s * r[:, None], np.isfinite(l) & (l > 0)


def contracted(v, idx):
    return nr.recompute(v, idx, terms=contracted_terms)


def descending(v, idx):
    return nr.recompute(v, idx, sums=lambda c, i, n: nr.vertex_sums(c, i, n, descending=True))


def in_double(v, idx):
    return nr.recompute(v, idx, sums=lambda c, i, n: nr.vertex_sums(c, i, n, dtype=np.float64).astype(F))


def unweighted(v, idx):
    return nr.recompute(v, idx, terms=unit_terms)


def reciprocal_root(v, idx):
    return nr.recompute(v, idx, normalise=by_reciprocal_root)


def no_side_rule(v, idx):
    return nr.recompute(v, idx, side_rule=False)


NEAR_MISSES = (contracted, descending, in_double, unweighted, reciprocal_root, no_side_rule)


def applicable(valence, n_flipped):
    """The near misses that CAN differ from the definition on a mesh with these valences.  A sum of one or two terms has no order to
    get wrong and no intermediate rounding to skip: both need a vertex of three corners.  Equal weights differ from areas where a vertex
    has two triangles.  The side rule shows where it negates a sum."""
    out = [contracted, reciprocal_root]
    if valence.max() >= 3:
        out += [descending, in_double]
    if valence.max() >= 2:
        out += [unweighted]
    if n_flipped:
        out += [no_side_rule]
    return out


@pytest.mark.parametrize("name", MESHES)
def test_the_test_data_tell_the_definition_from_its_near_misses(name):
    v, idx = twisted(name), indices_of(name)
    want = nr.recompute(v, idx)
    changed = (bits(want) != bits(v)).any(axis=1)
    misses = applicable(nr.valences(idx, len(v)), len(nr.flipped(v, idx)))
    assert set(misses) == set(NEAR_MISSES)                                # every mesh tells every near miss apart
    for near_miss in misses:
        got = near_miss(v, idx)
        assert got.dtype == F and (bits(got) != bits(want)).any(), near_miss.__name__                   # a miss ...
        assert np.array_equal(bits(got[:, :3]), bits(want[:, :3])) and np.array_equal(bits(got[:, 6:]), bits(want[:, 6:]))
        if near_miss is no_side_rule:                                     # ... that is not near: the other side, exactly
            f = nr.flipped(v, idx)
            assert np.array_equal(bits(got[f, 3:6]), bits(-want[f, 3:6])), near_miss.__name__
        elif near_miss is unweighted:
            # both are positive combinations of the same unit face normals wherever a vertex's triangles are wound alike: the same
            # hemisphere there (the fan's hub and the two rim vertices between its halves sum opposed unit normals: nothing near is
            # left of them); on the balls, whose triangles around a vertex differ in area by the ratio of two latitude bands, near
            alike = changed.copy()
            if name == "fan":
                alike[[nr.fan()[2]["hub"], 1, 1 + nr.HUB_VALENCE // 2]] = False
            assert ((got[alike, 3:6].astype(np.float64) * want[alike, 3:6]).sum(axis=1) > 0.5).all(), near_miss.__name__
            assert name == "fan" or np.allclose(got[changed, 3:6], want[changed, 3:6], rtol=0, atol=0.2), near_miss.__name__
        else:
            # ... and near: a few units in the last place, on the vertices that have a sum.  (Where the definition's sum is exactly
            # zero a contracted cross product of a triangle without area leaves the rounding error of one product behind, and that
            # residue is normalised into a normal of its own: a vertex the definition keeps is a place where a miss need not be near)
            assert np.allclose(got[changed, 3:6], want[changed, 3:6], rtol=0, atol=1e-6), near_miss.__name__


# ---------------------------------------------------------------------------------------------------- the range
@pytest.mark.parametrize("name", MESHES)
def test_a_range_restricts_what_is_written_not_what_is_read(name):
    v, idx = twisted(name), indices_of(name)
    whole = nr.recompute(v, idx)
    for first, count in ranges(name):
        assert nr.valid_range(first, count, len(v))
        got = nr.recompute(v, idx, first, count)
        m = nr.in_range(len(v), first, count)
        assert np.array_equal(bits(got[m]), bits(whole[m]))              # shared triangles are read whole: the range's vertices get the whole mesh's normals
        assert np.array_equal(bits(got[~m]), bits(v[~m]))
    first, count = ranges(name)[0]
    m = nr.in_range(len(v), first, count)
    tri = idx.reshape(-1, 3)
    assert (m[tri].any(axis=1) & ~m[tri].all(axis=1)).any()              # the ragged range cuts through triangles
    assert np.array_equal(bits(nr.recompute(v, idx, 5, 0)), bits(v))     # an empty range writes nothing
    # the definition reads the normals the vertices hold: a second call finds unit normals on the right side and returns the same bits
    assert np.array_equal(bits(nr.recompute(whole, idx)), bits(whole))


# ---------------------------------------------------------------------------------------------------- the host's range check
PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "normals_check.hpp"
// argv: first count n_vertex.  Prints "ok" or "refused", and the key bits of the adjacency build's sort for n_vertex
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const uint32_t first = (uint32_t)std::strtoul(argv[1], nullptr, 10), count = (uint32_t)std::strtoul(argv[2], nullptr, 10), n = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    std::printf("%s %u\n", trc_normals_range_check(first, count, n) ? "refused" : "ok", trc_normals_key_bits(n));
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("normals_check")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])

    def run(first, count, n_vertex):
        out = subprocess.run([str(exe), str(first), str(count), str(n_vertex)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
        return out[0] == "ok", int(out[1])
    return run


def test_range_check_is_the_definition_s(probe):
    big = 0xFFFFFFFF
    cases = [(0, 35, 35), (3, 32, 35), (34, 1, 35),                      # up to the last vertex
             (0, 36, 35), (3, 33, 35), (35, 1, 35), (34, 2, 35),         # the off-by-one
             (big, 1, 35), (big, big, 35), (2, big, 35), (big, 2, big), (big - 1, 1, big),      # first + count wraps
             (0, 0, 35), (35, 0, 35), (36, 0, 35), (big, 0, 35), (0, 0, 0), (0, 1, 0)]          # count == 0 names no vertex
    for first, count, n in cases:
        ok, key_bits = probe(first, count, n)
        assert ok == nr.valid_range(first, count, n), (first, count, n)
        assert key_bits == nr.key_bits(n), n
    assert [probe(*c)[0] for c in cases[:3]] == [True] * 3 and not any(probe(*c)[0] for c in cases[3:11]) and probe(*cases[11])[0]
    assert all(probe(*c)[0] for c in cases[12:17]) and not probe(*cases[17])[0]
    # the sort looks at whole 8-bit digits: every vertex index of the test meshes lies below 2 ^ (its passes * 8)
    for n in (1, 2, 35, 74, 256, 257, 2601, 65536, 65537, 499849, 1 << 24, (1 << 24) + 1):
        b = probe(0, n, n)[1]
        assert b == nr.key_bits(n) and (n - 1) >> b == 0 and (b == 1 or (n - 1) >> (b - 1) == 1)
