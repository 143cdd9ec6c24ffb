"""trc_update_primitives on the CPU: the ABI names it without a new version number, the host helpers build the scene builders'
records, the definition (tests/primitives_ref.py) is trc_host_build_node's arithmetic and leaves an unmoved tree alone, a refitted
tree finds what a freshly built one finds, and the host's checks (tracer_amd/csrc/primitives_check.hpp) refuse what the header lists."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import primitives_ref as pr
import refit_ref as rr
from conftest import random_rays
from oracle import pyoracle
from tracer_amd import abi, host

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SCENE = {}


def cornell():
    if "s" not in _SCENE:
        _SCENE["s"] = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    return _SCENE["s"]


# ---------------------------------------------------------------------------------------------------- the ABI
def test_abi_names_update_primitives():
    assert "trc_update_primitives" in abi.DEVICE_SYMBOLS
    for name in ("trc_host_make_sphere", "trc_host_make_square", "trc_host_make_cube"):
        assert name in abi.HOST_SYMBOLS
    assert abi.TRC_ABI_VERSION == 13                                  # an addition under 13: the number stays
    header = open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
    assert re.search(r"#define\s+TRC_ABI_VERSION\s+13\b", header)
    assert re.search(r"trc_status\s+trc_update_primitives\s*\(\s*trc_ctx\s*\*\s*ctx\s*,\s*const\s+trc_primitive_ranges\s*\*\s*r\s*\)\s*;", header)
    # the struct as a C compiler on this ABI lays it out: pointer, two words, three times
    R = abi.PrimitiveRanges
    assert C.sizeof(R) == 48
    want = {"spheres": 0, "first_sphere": 8, "n_sphere": 12, "squares": 16, "first_square": 24, "n_square": 28, "cubes": 32, "first_cube": 40, "n_cube": 44}
    assert {n: getattr(R, n).offset for n, _ in R._fields_} == want


def test_struct_layout_is_the_header_s(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "tracer_abi.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(trc_primitive_ranges),'
                   ' offsetof(trc_primitive_ranges, spheres), offsetof(trc_primitive_ranges, first_sphere), offsetof(trc_primitive_ranges, n_sphere),'
                   ' offsetof(trc_primitive_ranges, squares), offsetof(trc_primitive_ranges, first_square), offsetof(trc_primitive_ranges, n_square),'
                   ' offsetof(trc_primitive_ranges, cubes), offsetof(trc_primitive_ranges, first_cube), offsetof(trc_primitive_ranges, n_cube)); }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    R = abi.PrimitiveRanges
    assert got == [C.sizeof(R)] + [getattr(R, n).offset for n, _ in R._fields_]


# ---------------------------------------------------------------------------------------------------- the host helpers
def test_helpers_reproduce_the_cornell_records():
    v = cornell().view
    sp, sq, cb = pr.spheres_of(v), pr.squares_of(v), pr.cubes_of(v)
    assert (len(sp), len(sq), len(cb)) == (12, 7, 3)
    radii = [64.0] + [40.0] * 11                                       # (the record holds radius + 1e-4: the helper takes the builder's argument)
    for k, s in enumerate(sp):
        got = host.make_sphere(radii[k], (s.center.x, s.center.y, s.center.z), s.material)
        assert bytes(got) == bytes(s), k
    for k, s in enumerate(sq):
        got = host.make_square(s.axis_i, s.range_i.x, s.range_i.y, s.axis_j, s.range_j.x, s.range_j.y, s.axis_k, s.value_k, s.material)
        assert bytes(got) == bytes(s), k
    for k, c in enumerate(cb):
        assert bytes(host.make_cube(c.material, c.model_matrix)) == bytes(c), k
        m = np.array([[getattr(c.model_matrix.columns[col], "xyzw"[row]) for col in range(4)] for row in range(4)], F)
        assert bytes(host.make_cube(c.material, m)) == bytes(c), k     # ... and from a (4, 4) array m[r][c]


# ---------------------------------------------------------------------------------------------------- the leaf box
def special_matrices(rs):
    out = []
    for _ in range(40):
        a = rs.uniform(-3, 3)
        ax = rs.normal(size=3); ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        S = np.diag(rs.choice([-1.0, 1.0], 3) * rs.uniform(0.1, 300, 3))      # negative scales
        m = np.eye(4); m[:3, :3] = R @ S; m[:3, 3] = rs.uniform(-500, 500, 3)
        out.append(m.astype(F))
    for _ in range(20):                                                      # -0 entries, exact ties between corners
        m = np.zeros((4, 4), F); m[3, 3] = 1
        perm = rs.permutation(3)
        for r in range(3):
            m[r, perm[r]] = rs.choice([-1.0, 1.0, 2.0, -0.5])
        m[m == 0] = rs.choice([0.0, -0.0], (m == 0).sum())
        m[:3, 3] = rs.choice([0.0, -0.0, 1.0, -7.5], 3)
        out.append(m)
    return out


def test_leaf_box_is_build_node_s():
    rs = np.random.RandomState(11)
    n = 0
    for m in special_matrices(rs):
        for _ in range(4):
            lo = rs.uniform(-50, 50, 3).astype(F); hi = (lo + rs.uniform(0, 80, 3)).astype(F)
            if rs.rand() < 0.3:
                lo[rs.randint(3)] = F(-0.0); hi[rs.randint(3)] = F(0.0)      # a corner on a signed zero
            if rs.rand() < 0.2:
                hi[1] = lo[1]                                               # a flat box: four pairs of equal corners
            ref = host.build_node(tuple(float(x) for x in lo), tuple(float(x) for x in hi), abi.PRIM_CUBE, 0, m)
            want = np.array([ref.bBOX.mini.x, ref.bBOX.mini.y, ref.bBOX.mini.z, ref.bBOX.maxi.x, ref.bBOX.maxi.y, ref.bBOX.maxi.z], F)
            got = np.concatenate(pr.leaf_box(lo, hi, [[m[r, c] for r in range(3)] for c in range(4)]))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (m, lo, hi)
            n += 1
    assert n == 240


def test_records_are_fill_primitives_bits():
    """the packing against values worked out by hand: sphere 0 and the light square of the Cornell scene"""
    v = cornell().view
    s = pr.pack_sphere(pr.spheres_of(v)[0])
    assert list(s[:4].view(F)) == [F(200), F(250), F(200), F(64) + F(0.0001)] and s[4] == 7 and not s[5:].any()
    q = pr.pack_square(pr.squares_of(v)[5])
    assert list(q[:5].view(F)) == [F(400), F(555), F(200), F(355), F(555 - 0.1)]
    assert q[5:6].view(F)[0] == F(1) / (F(2) * F(155) * F(155)) and q[6] == (0 | 2 << 2 | 1 << 4) and q[7] == 3
    c = pr.cubes_of(v)[1]
    k = pr.pack_cube(c)
    assert k[12 + 9:12 + 12].view(F).tolist() == [130.0, 1.0, 65.0] and k[33:39].view(F).tolist() == [0, 0, 0, 1, 1, 1] and k[39] == 19
    assert k[24 + 3:24 + 6].view(F).tolist() == [c.normal_matrix.columns[1].x, c.normal_matrix.columns[1].y, c.normal_matrix.columns[1].z]


# ---------------------------------------------------------------------------------------------------- the refit
def test_unmoved_primitives_leave_a_host_tree_as_it_was():
    for sc in (cornell(), host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1)), host.HostScene(abi.SCENE_CORNELL_VOLUME)):
        nodes = sc.bvh_array().copy()
        v = sc.view
        got = pr.refit(nodes, *pr.motion(v, 0.0), rr.vertices_of(v) if v.n_vertex else None, rr.indices_of(v) if v.n_vertex else None)
        assert np.array_equal(got, nodes)


RAY_SEED, N_RAYS = 5, 4000


def test_refitted_tree_finds_what_a_fresh_tree_finds():
    sc = cornell()
    nodes = sc.bvh_array().copy()
    lists = pr.motion(sc.view)
    refitted = pr.Moved(sc.view, pr.refit(nodes, *lists), *lists)
    fresh = pr.Moved(sc.view, rr.raw(host.build_tree(pr.leaves(nodes, *lists))), *lists)
    assert not np.array_equal(rr.raw(fresh.nodes)[:, :6], nodes[:, :6])         # the fresh build is another tree
    rays = random_rays(N_RAYS, RAY_SEED)
    a, b = pyoracle.trace_rays(refitted.view, rays), pyoracle.trace_rays(fresh.view, rays)
    before = pyoracle.trace_rays(sc.view, rays)
    differ = np.zeros(N_RAYS, bool)
    for f in ("hit", "pType", "pIndex", "t", "p", "gn", "sn"):
        d = a[f].view(np.uint32) != b[f].view(np.uint32)
        differ |= d.reshape(N_RAYS, -1).any(axis=1)
    # two trees may resolve a tie in t between two primitives differently, and nothing else: the rays that differ hit at the same t
    assert (a["t"][differ].view(np.uint32) == b["t"][differ].view(np.uint32)).all() and (a["hit"][differ] == b["hit"][differ]).all()
    assert differ.sum() <= 0.01 * N_RAYS, differ.sum()
    moved = (a["t"].view(np.uint32) != before["t"].view(np.uint32)) | (a["pIndex"] != before["pIndex"])
    assert moved.sum() > 200 and (a["hit"] != 0).sum() > 1500                    # the motion is seen, and the rays hit (many start outside the box)


# ---------------------------------------------------------------------------------------------------- the host's checks
PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "primitives_check.hpp"
// argv: file.  The file: 12 words -- first / n of spheres, squares, cubes; the scene's three counts and n_material; a mask of lists
// to pass as NULL (1 spheres, 2 squares, 4 cubes); 1: pass r == NULL -- then the records.  Prints "ok" or the reason
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[12];
    if (std::fread(h, 4, 12, f) != 12) return 2;
    std::vector<trc_Sphere> sp(h[1]); std::vector<trc_Square> sq(h[3]); std::vector<trc_Cube> cb(h[5]);
    if (h[1] && std::fread(sp.data(), sizeof(trc_Sphere), h[1], f) != h[1]) return 2;
    if (h[3] && std::fread(sq.data(), sizeof(trc_Square), h[3], f) != h[3]) return 2;
    if (h[5] && std::fread(cb.data(), sizeof(trc_Cube), h[5], f) != h[5]) return 2;
    std::fclose(f);
    trc_primitive_ranges r{};
    r.spheres = (h[10] & 1u) || !h[1] ? nullptr : sp.data(); r.first_sphere = h[0]; r.n_sphere = h[1];
    r.squares = (h[10] & 2u) || !h[3] ? nullptr : sq.data(); r.first_square = h[2]; r.n_square = h[3];
    r.cubes = (h[10] & 4u) || !h[5] ? nullptr : cb.data(); r.first_cube = h[4]; r.n_cube = h[5];
    const char* why = trc_primitive_ranges_check(h[11] ? nullptr : &r, h[6], h[7], h[8], h[9]);
    std::printf("%s\n", why ? why : "ok");
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("primitives_check")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    count = [0]

    def run(spheres=(), squares=(), cubes=(), first=(0, 0, 0), scene=(12, 7, 3), n_material=20, null_mask=0, null_r=0):
        n = [len(spheres), len(squares), len(cubes)]
        path = d / f"case{count[0]}.bin"; count[0] += 1
        with open(path, "wb") as f:
            head = [first[0], n[0], first[1], n[1], first[2], n[2], *scene, n_material, null_mask, null_r]
            f.write(struct.pack("<12I", *head))
            for lst in (spheres, squares, cubes):
                for rec in lst:
                    f.write(bytes(rec))
        return subprocess.run([str(exe), str(path)], capture_output=True, text=True, check=True, timeout=60).stdout.strip()
    return run


def test_checks_accept_the_cornell_lists_and_refuse_what_the_header_lists(probe):
    v = cornell().view
    sp, sq, cb = list(pr.spheres_of(v)), list(pr.squares_of(v)), list(pr.cubes_of(v))
    big = 0xFFFFFFFF
    assert probe(sp, sq, cb) == "ok"
    assert probe(*(list(l) for l in pr.motion(v))) == "ok"
    assert probe() == "ok"                                                       # all counts zero, lists NULL
    assert probe(sp[:1], first=(11, 0, 0)) == "ok" and probe([], sq[:2], first=(0, 5, 0)) == "ok" and probe([], [], cb[:1], first=(0, 0, 2)) == "ok"
    assert probe(first=(big, big, big)) == "ok"                                  # a range with n == 0 names nothing
    assert "NULL" in probe(null_r=1)
    for mask, lists in ((1, (sp[:2], [], [])), (2, ([], sq[:2], [])), (4, ([], [], cb[:2]))):
        assert "NULL" in probe(*lists, null_mask=mask)
    # first + n beyond the count, with and without a wrap of the 32-bit sum
    for first, lists in (((11, 0, 0), (sp[:2], [], [])), ((12, 0, 0), (sp[:1], [], [])), ((big, 0, 0), (sp[:1], [], [])), ((big - 1, 0, 0), (sp[:3], [], [])),
                         ((0, 6, 0), ([], sq[:2], [])), ((0, big, 0), ([], sq[:2], [])), ((0, 0, 3), ([], [], cb[:1])), ((0, 0, big), ([], [], cb[:2]))):
        assert "beyond" in probe(*lists, first=first) or ">" in probe(*lists, first=first), first
    assert probe(sp, scene=(11, 7, 3)) != "ok" and probe([], sq, scene=(12, 6, 3)) != "ok" and probe([], [], cb, scene=(12, 7, 2)) != "ok"

    def edited(rec, fn):
        c = type(rec).from_buffer_copy(bytes(rec)); fn(c); return c
    # materials
    assert "material" in probe([edited(sp[0], lambda s: setattr(s, "material", 20))])
    assert "material" in probe([], [edited(sq[0], lambda s: setattr(s, "material", big))])
    assert "material" in probe([], [], [edited(cb[0], lambda s: setattr(s, "material", 20))])
    assert probe([edited(sp[0], lambda s: setattr(s, "material", 19))]) == "ok"
    # axes
    for name in ("axis_i", "axis_j", "axis_k"):
        assert "axis" in probe([], [edited(sq[3], lambda s, name=name: setattr(s, name, 3))])
    # values: a NaN, an infinity and 2e37 in every field that is read; 1e37 itself passes
    sphere_fields = [lambda s, x: setattr(s, "radius", x), lambda s, x: setattr(s.center, "y", x), lambda s, x: setattr(s.boundingBOX.mini, "x", x),
                     lambda s, x: setattr(s.boundingBOX.maxi, "z", x), lambda s, x: setattr(s.model_matrix.columns[3], "y", x), lambda s, x: setattr(s.model_matrix.columns[0], "z", x)]
    square_fields = [lambda s, x: setattr(s.range_i, "x", x), lambda s, x: setattr(s.range_i, "y", x), lambda s, x: setattr(s.range_j, "x", x), lambda s, x: setattr(s.range_j, "y", x),
                     lambda s, x: setattr(s, "value_k", x), lambda s, x: setattr(s.boundingBOX.maxi, "y", x), lambda s, x: setattr(s.model_matrix.columns[2], "x", x)]
    cube_fields = [lambda s, x: setattr(s.inverse_matrix.columns[3], "z", x), lambda s, x: setattr(s.model_matrix.columns[1], "y", x), lambda s, x: setattr(s.normal_matrix.columns[2], "x", x),
                   lambda s, x: setattr(s.box.mini, "z", x), lambda s, x: setattr(s.box.maxi, "x", x)]
    for bad in (float("nan"), float("inf"), -float("inf"), 2e37, -2e37):
        for fn in sphere_fields:
            assert "sphere value" in probe([sp[1], edited(sp[2], lambda s: fn(s, bad))])
        for fn in square_fields:
            assert "square value" in probe([], [edited(sq[5], lambda s: fn(s, bad))])
        for fn in cube_fields:
            assert "cube value" in probe([], [], [cb[0], cb[1], edited(cb[2], lambda s: fn(s, bad))])
    assert probe([edited(sp[2], lambda s: setattr(s.center, "x", 1e37))]) == "ok"
    # what is not read may hold anything: the w row of a matrix, the fourth normal column, a sphere's inverse
    assert probe([edited(sp[2], lambda s: setattr(s.inverse_matrix.columns[0], "x", float("nan")))]) == "ok"
    assert probe([], [], [edited(cb[0], lambda s: setattr(s.normal_matrix.columns[3], "x", float("inf")))]) == "ok"
    assert probe([], [], [edited(cb[0], lambda s: setattr(s.model_matrix.columns[0], "w", float("nan")))]) == "ok"
