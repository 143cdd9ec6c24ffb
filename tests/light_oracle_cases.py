"""The cases of tests/test_gpu_light_oracle.py: scenes, maps, the launch each case asks for, and the oracle's frame of each (cached: a
frame does not depend on the launch shape, so the shapes of one scene share it).  tests/test_oracle_lights.py runs the same cases
through the oracle alone and checks that they reach every branch of the oracle's traceMISLight.  No GPU is touched here."""
import os
import re
import sys
import tempfile

import numpy as np

from oracle import pyoracle as po
from tracer_amd import abi, host

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "envlight_ref"))
import envlight_loader as el  # noqa: E402

F = np.float32
W, H = 61, 45              # neither side a multiple of 8: the edge blocks are partly empty
SEED = 9
MIS, PATH, VOLUME = abi.INTEGRATOR_MIS, abi.INTEGRATOR_PATH, abi.INTEGRATOR_VOLUME
PLASTIC_SLOT, DIM_EMITTER_SLOT = 8, 9       # Cornell's table has no Plastic and one emitter: two of its unused entries become them

_TMP = tempfile.TemporaryDirectory(prefix="light_oracle_")
_SCENES, _ORACLE = {}, {}


class SceneSet:
    """a scene, its camera for the W x H frame, the per-triangle materials (or None) and the images (or [])"""

    def __init__(self, scene, cam, tri=None, images=()):
        self.scene, self.view, self.cam, self.tri, self.images = scene, scene.view, cam, tri, list(images)


def _random_images(view, rng, sizes=((13, 7), (64, 64), (1, 9), (32, 5))):
    """a random, non-uniform image on every non-emitter material (tests/test_gpu_textures.py: random_textures)"""
    imgs = []
    for i in range(view.n_material):
        m = view.materials[i]
        if m.type == abi.MAT_DIFFUSE:
            continue
        h, w = sizes[len(imgs) % len(sizes)]
        imgs.append(rng.random((h, w, 3), dtype=F))
        m.textureInfo.type = abi.TEX_IMAGE
        m.textureInfo.textureIndex = len(imgs) - 1
    return imgs


def cornell(residence, tex=False, random_materials=True, lamp19=False):
    """Cornell + the 48-triangle ball (the whole tree in LDS) or the 1104-triangle one (read from memory); every triangle a random
    material of the whole table, in which entry 8 is made a Plastic and entry 9 a second, dimmer emitter.  random_materials=False: no
    array, every triangle is material 19 (the kernels that do not read a triangle's material run); lamp19 then makes entry 19 an emitter,
    so that the mesh is a light without an array"""
    key = ("cornell", residence, tex, random_materials, lamp19)
    if key not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.ball(24, 24, 1.0)
        sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
        v = sc.view
        v.materials[PLASTIC_SLOT].type = abi.MAT_PLASTIC
        v.materials[PLASTIC_SLOT].textureInfo.albedo.x, v.materials[PLASTIC_SLOT].textureInfo.albedo.y, v.materials[PLASTIC_SLOT].textureInfo.albedo.z = 0.7, 0.6, 0.3
        v.materials[DIM_EMITTER_SLOT].type = abi.MAT_DIFFUSE
        v.materials[DIM_EMITTER_SLOT].textureInfo.albedo.x, v.materials[DIM_EMITTER_SLOT].textureInfo.albedo.y, v.materials[DIM_EMITTER_SLOT].textureInfo.albedo.z = 2.0, 1.0, 0.5
        if lamp19:
            v.materials[19].type = abi.MAT_DIFFUSE
            v.materials[19].textureInfo.albedo.x, v.materials[19].textureInfo.albedo.y, v.materials[19].textureInfo.albedo.z = 3.0, 2.5, 2.0
        rng = np.random.default_rng(100 + (residence == "mem"))
        tri = rng.integers(0, v.n_material, v.n_index // 3).astype(np.uint32) if random_materials else None
        imgs = _random_images(v, np.random.default_rng(7)) if tex else []
        _SCENES[key] = SceneSet(sc, host.prepare_camera(W, H), tri, imgs)
    return _SCENES[key]


def _from_pbrt(name, text, triangle_materials):
    text = re.sub(r'"integer xresolution" \[ \d+ \] "integer yresolution" \[ \d+ \]', f'"integer xresolution" [ {W} ] "integer yresolution" [ {H} ]', text)
    path = os.path.join(_TMP.name, name + ".pbrt")
    with open(path, "w") as f:
        f.write(text)
    out = host.HostScene.from_pbrt(path, triangle_materials=triangle_materials)
    assert out[2].xres == W and out[2].yres == H
    return SceneSet(out[0], out[1], out[4] if triangle_materials else None)


def room():
    """the closed Lambert room of tests/test_gpu_mesh_lights.py: 14 triangles, a two-triangle lamp, no square"""
    if "room" not in _SCENES:
        from test_gpu_mesh_lights import room_pbrt
        _SCENES["room"] = _from_pbrt("room", room_pbrt(), True)
        assert _SCENES["room"].view.n_square == 0
    return _SCENES["room"]


def floor():
    """the two Lambert squares under the sky of tests/test_gpu_envlight.py::test_environment_only_scene: no square light"""
    if "floor" not in _SCENES:
        from test_gpu_envlight import FLOOR_PBRT
        _SCENES["floor"] = _from_pbrt("floor", FLOOR_PBRT, False)
        assert _SCENES["floor"].view.n_square < 7
    return _SCENES["floor"]


def coplanar():
    """A lamp triangle in the plane of the wall it lights (x = 0), for the guard on the mesh sample's liPDF.  The wall's vertex normals
    are (1, 1, 0), not its geometric normal: the shading normal keeps a y component, so a sample on the lamp above has wi.z > 0, while
    offset_ray moves the shading point and the lamp's point by the same 2^-16 in x (both |x| < 1/32, both normals' x = 1): the
    direction to the sample has x = 0 exactly, cosL = 0 and liPDF = inf."""
    if "coplanar" not in _SCENES:
        text = f'''LookAt 3 0.2 0  0 0 0  0 1 0
Camera "perspective" "float fov" [ 50 ]
Film "image" "integer xresolution" [ {W} ] "integer yresolution" [ {H} ]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 10 10 10 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ 0 2 -1  0 2 1  0 3.5 0 ] "normal N" [ 1 0 0  1 0 0  1 0 0 ]
AttributeEnd
Material "matte" "rgb Kd" [ 0.6 0.6 0.6 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 0 -1.5 -2  0 -1.5 2  0 1.5 1.5  0 1.5 -1.7 ] "normal N" [ 1 1 0  1 1 0  1 1 0  1 1 0 ]
WorldEnd
'''
        _SCENES["coplanar"] = _from_pbrt("coplanar", text, True)
    return _SCENES["coplanar"]


def env_map(name):
    if name == "sun":
        return el.sun_sky(32, 16, sun_radius=0.25, sun_power=200.0)
    if name == "sky":          # the floor's: the sun above the horizon
        return el.sun_sky(32, 16, sun=(0.3, 0.7), sun_radius=0.3, sun_power=300.0)
    assert name == "spiky"     # exactly black texels, a black band where Cornell's open side looks (cells of pdf 0) and one very bright texel
    rng = np.random.default_rng(5)
    img = rng.random((16, 32, 3), dtype=F)
    img[rng.random((16, 32)) < 0.4] = 0.0
    img[:, 4:13] = 0.0
    img[11, 20] = (30000.0, 20000.0, 10000.0)
    return img


class Case:
    def __init__(self, id, scene, light=None, shape="one", env=None, spp=None, max_depth=8, integrator=MIS, pick=1, frame0=0, second=0):
        self.id, self.scene_fn, self.light, self.shape, self.env = id, scene, light, shape, env
        self.spp = spp if spp is not None else (2 if shape == "strip" else 16)
        self.max_depth, self.integrator, self.pick, self.frame0, self.second = max_depth, integrator, pick, frame0, second

    @property
    def scene(self):
        return self.scene_fn()

    def oracle_key(self):
        return (self.scene_fn.__name__, getattr(self.scene_fn, "args", ()), self.light, self.env, self.spp, self.max_depth, self.integrator, self.pick, self.frame0, self.second)

    def __repr__(self):
        return self.id


def _bind(fn, *args):
    def f():
        return fn(*args)
    f.__name__, f.args = fn.__name__, args
    return f


def matrix():
    """{Env, Mesh} x {LDS, memory} x {one, strip, pwg where it exists} x {no image, random images} x {the kernels that read each
    triangle's material, over a random array; the plain ones, every triangle material 19}: every non-null Env, EnvTex, Mesh and MeshTex
    entry of render_kernels<LDS, MIS>() and of its trimat twin.  Without an array the mesh cases make entry 19 an emitter: the whole
    ball is the light."""
    out = []
    for family in ("trimat", "plain19"):
        for light in ("env", "mesh"):
            for residence in ("lds", "mem"):
                for shape in ("one", "strip") + (("pwg",) if residence == "mem" else ()):
                    for tex in (False, True):
                        scene = _bind(cornell, residence, tex) if family == "trimat" else _bind(cornell, residence, tex, False, light == "mesh")
                        out.append(Case(f"{light}-{residence}-{shape}-{'tex' if tex else 'notex'}-{family}", scene, light, shape,
                                        env="sun" if light == "env" else None))
    return out


def further():
    """on the cheapest shape (one wavefront per block, the LDS-resident scene)"""
    lds = _bind(cornell, "lds", False)
    out = []
    for light in ("env", "mesh"):
        e = "sun" if light == "env" else None
        out += [Case(f"{light}-depth{d}", lds, light, env=e, max_depth=d) for d in (1, 2)]       # (8 is the matrix's)
        out.append(Case(f"{light}-second-launch", lds, light, env=e, spp=8, second=8))
    out.append(Case("env-spiky-map", lds, "env", env="spiky"))
    out.append(Case("env-no-squares", floor, "env", env="sky"))
    out.append(Case("env-no-squares-depth1", floor, "env", env="sky", max_depth=1))
    out.append(Case("env-no-squares-emitter", room, "env", env="sky"))        # (the closed room under a map: its lamp is hit by BSDF rays alone)
    out.append(Case("mesh-no-squares", room, "mesh"))
    out.append(Case("mesh-pick0", lds, "mesh", pick=0))
    out.append(Case("mesh-no-squares-pick0", room, "mesh", pick=0))
    out.append(Case("mesh-coplanar-lamp", coplanar, "mesh", max_depth=2))
    return out


def beyond():
    """random per-triangle materials and random images without a light flag: the three integrators, and the Tex variants of
    one / strip / pwg"""
    out = []
    for integ, name in ((PATH, "path"), (MIS, "mis"), (VOLUME, "volume")):
        out.append(Case(f"trimat-{name}", _bind(cornell, "lds", False), integrator=integ))
        for residence in ("lds", "mem"):
            for shape in ("one", "strip") + (("pwg",) if residence == "mem" else ()):
                out.append(Case(f"tex-{name}-{residence}-{shape}", _bind(cornell, residence, True, False), shape=shape, integrator=integ))
    return out


def oracle_frame(case):
    """(accum, rng, stats) of the case in the oracle; a second launch (case.second samples) continues the first's frame count"""
    key = case.oracle_key()
    if key not in _ORACLE:
        s = case.scene
        po.set_environment_map(env_map(case.env) if case.env else None)
        try:
            rng = host.fill_rng(SEED, W, H)
            kw = dict(max_depth=case.max_depth, integrator=case.integrator, env_light=case.light == "env", mesh_lights=case.light == "mesh",
                      mesh_light_pick=case.pick, triangle_materials=s.tri, textures=s.images)
            acc, st = po.render(s.view, s.cam, W, H, rng, spp=case.spp, frame0=case.frame0, **kw)
            if case.second:
                acc, st2 = po.render(s.view, s.cam, W, H, rng, accum=acc, spp=case.second, frame0=case.frame0 + case.spp, **kw)
                st.rays += st2.rays; st.paths += st2.paths; st.shaded += st2.shaded
        finally:
            po.set_environment_map(None)
        _ORACLE[key] = (acc, rng, st)
    return _ORACLE[key]
