"""trc_host_scene_load_pbrt_flags (include/tracer_abi.h): flags 0 is trc_host_scene_load_pbrt byte for byte, and
TRC_PBRT_TRIANGLE_MATERIALS gives every mesh shape its own material -- behind index 19, which keeps what the plain load puts there --
with one index per triangle from trc_host_scene_triangle_materials (the input of trc_upload_triangle_materials)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tracer_amd import abi, host
from test_pbrt_scene import CORNELL, INSTANCED, QUADRICS, WEDGE_PLY

# a matte floor mesh (a 3 x 3 grid: not a rectangle of two triangles, so it stays triangles), a glass tetrahedron on it and an
# emitting disk (tessellated) above them; a sphere and a rectangle light keep the analytic paths in the picture
MIXED = '''LookAt 0 4 -10  0 1 0  0 1 0
Camera "perspective" "float fov" [ 45 ]
Film "image" "integer xresolution" [ 64 ] "integer yresolution" [ 48 ]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 5 5 5 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -1 6 -1  1 6 -1  1 6 1  -1 6 1 ]
AttributeEnd
Material "matte" "rgb Kd" [ 0.6 0.5 0.4 ]
Shape "trianglemesh" "integer indices" [ 0 1 4 0 4 3  1 2 5 1 5 4  3 4 7 3 7 6  4 5 8 4 8 7 ]
      "point P" [ -5 0 -5  0 0 -5  5 0 -5  -5 0 0  0 0 0  5 0 0  -5 0 5  0 0 5  5 0 5 ]
AttributeBegin
  Material "glass" "rgb Kt" [ 0.9 0.95 1 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2  0 2 3  0 3 1  1 3 2 ]
        "point P" [ -1 0 -1   1 0 -1   0 0 1   0 1.5 0 ]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 7 6 5 ]
  Translate 2 3 0
  Rotate 90 1 0 0
  Shape "disk" "float radius" 0.75
AttributeEnd
AttributeBegin
  Material "plastic" "rgb Kd" [ 0.1 0.2 0.7 ]
  Translate -2.5 1 0
  Shape "sphere" "float radius" 1
AttributeEnd
WorldEnd
'''


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    (tmp_path / "wedge.ply").write_text(WEDGE_PLY)
    return str(p)


def raw(ptr, n, ctype):
    """the bytes of n records at a ctypes pointer"""
    return C.string_at(ptr, n * C.sizeof(ctype)) if n else b""


def load_flags(path, flags):
    """trc_host_scene_load_pbrt_flags(path, flags) through the library itself -> (HostScene, camera, info, shapes)"""
    return host.HostScene.from_pbrt(path, flags=flags)


def arrays(scene):
    v = scene.view
    return [raw(v.bvhList, v.n_bvh, abi.BVH), raw(v.sphereList, v.n_sphere, abi.Sphere), raw(v.squareList, v.n_square, abi.Square),
            raw(v.cubeList, v.n_cube, abi.Cube), raw(v.triList, v.n_vertex, abi.TriangleVertex),
            raw(v.idxList, v.n_index, C.c_uint32), raw(v.materials, v.n_material, abi.Material)]


FIXTURES = {"cornell": CORNELL, "quadrics": QUADRICS, "instanced": INSTANCED, "mixed": MIXED}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbrt_plain_load.json")


def digests(scene, cam, info, shapes):
    """sha256 of every scene array, the camera, the info record and the shape records of one load"""
    parts = dict(zip(("bvh", "spheres", "squares", "cubes", "vertices", "indices", "materials"), arrays(scene)))
    parts.update(camera=bytes(cam), info=bytes(info), shapes=b"".join(bytes(s) for s in shapes))
    return {k: hashlib.sha256(v).hexdigest() for k, v in parts.items()}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_flags_zero_is_the_plain_load_of_before(tmp_path, name):
    """the plain load and the flags-0 load both give what the library gave before per-triangle materials existed, byte for byte
    (tests/golden/pbrt_plain_load.json, recorded with that library by tests/golden/make_pbrt_plain_load.py)"""
    path = write(tmp_path, "scene.pbrt", FIXTURES[name])
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    a = host.HostScene.from_pbrt(path)
    b = load_flags(path, 0)
    assert digests(*a) == want
    assert digests(*b) == want
    assert b[0].triangle_materials().size == 0 and a[0].triangle_materials().size == 0


def test_unknown_flag_bits_are_refused(tmp_path):
    path = write(tmp_path, "scene.pbrt", MIXED)
    with pytest.raises(RuntimeError):
        load_flags(path, 2)


def material(view, i):
    m = view.materials[int(i)]
    return m.type, (m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z), m.textureInfo.type


def test_each_mesh_names_its_own_material(tmp_path):
    path = write(tmp_path, "mixed.pbrt", MIXED)
    plain, _, pinfo, pshapes = host.HostScene.from_pbrt(path)
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(path, triangle_materials=True)
    v, pv = sc.view, plain.view
    # the plain load: one material for all triangles (the floor's), the other two meshes only counted
    assert pinfo.n_triangle_material_conflicts == 2 and info.n_triangle_material_conflicts == 0
    # geometry and the plain table are unchanged: the new materials come behind it, 19 included
    assert arrays(sc)[:6] == arrays(plain)[:6]
    assert v.n_material > pv.n_material > 19
    assert raw(v.materials, pv.n_material, abi.Material) == raw(pv.materials, pv.n_material, abi.Material)
    assert tri.dtype == np.uint32 and tri.shape == (v.n_index // 3,) and (tri < v.n_material).all()
    meshes = [s for s in shapes if s.mapped_type == abi.PRIM_TRIANGLE]
    assert [s.kind for s in meshes] == [abi.PBRT_SHAPE_TRIANGLEMESH, abi.PBRT_SHAPE_TRIANGLEMESH, abi.PBRT_SHAPE_DISK]
    want = [(abi.MAT_LAMBERT, (0.6, 0.5, 0.4)), (abi.MAT_GLASS, (0.9, 0.95, 1.0)), (abi.MAT_DIFFUSE, (7.0, 6.0, 5.0))]
    covered = np.zeros(tri.size, bool)
    for s, (mtype, colour) in zip(meshes, want):
        rng = slice(s.mapped_index, s.mapped_index + s.n_indices // 3)
        assert (tri[rng] == s.mapped_material).all() and not covered[rng].any()
        covered[rng] = True
        t, alb, tex = material(v, s.mapped_material)
        assert t == mtype and np.allclose(alb, colour) and tex == abi.TEX_CONSTANT
        assert s.mapped_material > 19
    assert covered.all()
    assert len({s.mapped_material for s in meshes}) == 3
    # every other shape record is the plain load's
    for s, p in zip(shapes, pshapes):
        if s.mapped_type != abi.PRIM_TRIANGLE:
            assert bytes(s) == bytes(p)
        else:
            assert p.mapped_material == 19
    # the glass mesh keeps the specular flag and eta of the table's glass
    m = v.materials[int(meshes[1].mapped_material)]
    assert m.specular == 1 and m.eta == np.float32(1.5)


def test_checkerboard_and_plymesh_meshes(tmp_path):
    """CORNELL: a plastic tetrahedron, a checkerboard cylinder + disk and a matte PLY wedge -- three materials for four meshes"""
    path = write(tmp_path, "cornell.pbrt", CORNELL)
    plain, _, pinfo, _ = host.HostScene.from_pbrt(path)
    sc, _, info, shapes, tri = host.HostScene.from_pbrt(path, triangle_materials=True)
    assert info.n_triangle_material_conflicts == 0 and pinfo.n_triangle_material_conflicts > 0
    v = sc.view
    assert raw(v.materials, 20, abi.Material) == raw(plain.view.materials, 20, abi.Material)
    meshes = [s for s in shapes if s.mapped_type == abi.PRIM_TRIANGLE]
    assert [s.kind for s in meshes] == [abi.PBRT_SHAPE_TRIANGLEMESH, abi.PBRT_SHAPE_CYLINDER, abi.PBRT_SHAPE_DISK, abi.PBRT_SHAPE_PLYMESH]
    for s in meshes:
        assert (tri[s.mapped_index: s.mapped_index + s.n_indices // 3] == s.mapped_material).all()
    assert material(v, meshes[0].mapped_material)[:2] == (abi.MAT_PLASTIC, (np.float32(0.2), np.float32(0.3), np.float32(0.8)))
    cyl, disk = material(v, meshes[1].mapped_material), material(v, meshes[2].mapped_material)
    assert meshes[1].mapped_material == meshes[2].mapped_material and cyl[2] == abi.TEX_CHECKER and cyl[0] == abi.MAT_LAMBERT
    assert np.allclose(cyl[1], (0.8, 0.7, 0.2)) and disk == cyl
    assert material(v, meshes[3].mapped_material)[:2] == (abi.MAT_LAMBERT, (np.float32(0.4), np.float32(0.6), np.float32(0.3)))


def test_instances_carry_their_templates_material(tmp_path):
    path = write(tmp_path, "instanced.pbrt", INSTANCED)
    sc, _, info, shapes, tri = host.HostScene.from_pbrt(path, triangle_materials=True)
    v = sc.view
    meshes = [s for s in shapes if s.mapped_type == abi.PRIM_TRIANGLE]
    assert len(meshes) == 2 and v.n_index == 6 and tri.size == 2           # the template's triangle, placed twice
    assert meshes[0].mapped_material == meshes[1].mapped_material == tri[0] == tri[1]
    t, alb, _ = material(v, tri[0])
    assert t == abi.MAT_LAMBERT and np.allclose(alb, (0.2, 0.4, 0.6))
    # the instances' spheres keep their glass
    assert material(v, v.sphereList[0].material)[0] == abi.MAT_GLASS


def test_no_array_without_the_flag(tmp_path):
    path = write(tmp_path, "mixed.pbrt", MIXED)
    sc, *_ = host.HostScene.from_pbrt(path)
    assert sc.triangle_materials().size == 0
    made = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(6, 6, 0.1))
    assert made.view.n_index > 0 and made.triangle_materials().size == 0
    p, n = C.POINTER(C.c_uint32)(), C.c_uint32(7)
    host.lib().trc_host_scene_triangle_materials(made._h, C.byref(p), C.byref(n))
    assert n.value == 0
