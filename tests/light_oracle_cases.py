"""The cases of tests/test_gpu_light_oracle.py: scenes, maps, the launch each case asks for, and the oracle's frame of each (cached: a
frame does not depend on the launch shape, so the shapes of one scene share it).  tests/test_oracle_lights.py runs the same cases
through the oracle alone and checks that they reach every branch of the oracle's traceMISLight.  Below them: the enumeration and the
cases of the kernel census (tests/test_gpu_kernel_census.py), and the scenes, cameras and primary-hit prediction of the replay matrix
(tests/test_gpu_primary_replay.py; tests/test_replay_scenes.py checks both on the CPU).  No GPU is touched here."""
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

    def __init__(self, scene, cam, tri=None, images=(), view=None):
        self.scene, self.view, self.cam, self.tri, self.images = scene, view if view is not None else scene.view, cam, tri, list(images)


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


def cornell(residence, tex=False, random_materials=True, lamp19=False, checker=False, tri_materials=None):
    """Cornell + the 48-triangle ball (the whole tree in LDS) or the 1104-triangle one (read from memory); every triangle a random
    material of the whole table, in which entry 8 is made a Plastic and entry 9 a second, dimmer emitter.  random_materials=False: no
    array, every triangle is material 19 (the kernels that do not read a triangle's material run); lamp19 then makes entry 19 an emitter,
    so that the mesh is a light without an array; checker makes every cube's material a checker texture (its colour reads rec.uv:
    tests/test_gpu_lds_fit.py), over the image if there is one -- the cubes' materials are 0, 19 and 2, so without an array the mesh's
    triangles are checkered with them.  "tiny": the 12-triangle ball (6 of them with area), the largest whose workgroup k_render_dense
    still holds 24 of per CU (its LDS is the 6592 bytes of trc_render_config.hpp; the 48-triangle ball's 9408 bytes are refused the dense
    kernel), with tri_materials = the array of its materials: replay_camera sees its triangles 1 and 6"""
    key = ("cornell", residence, tex, random_materials, lamp19, checker, tri_materials)
    if key not in _SCENES:
        mesh = {"lds": (4, 6, 0.1), "mem": (24, 24, 1.0), "tiny": (2, 3, 0.1)}[residence]
        mesh = host.Mesh.ball(*mesh)
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
        if tri_materials is not None:
            tri = np.array(tri_materials, np.uint32)
            assert random_materials and len(tri) == v.n_index // 3
        imgs = _random_images(v, np.random.default_rng(7)) if tex else []
        if checker:
            assert v.n_cube > 0
            for i in range(v.n_cube):
                v.materials[v.cubeList[i].material].textureInfo.type = abi.TEX_CHECKER
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
    """sobol = TRC_FLAG_SOBOL, stats = TRC_FLAG_COLLECT_STATS, env_rgb = the constant environment (trc_set_environment), cam = a
    function of (width, height) that gives the camera instead of the scene's own (replay_camera)"""

    def __init__(self, id, scene, light=None, shape="one", env=None, spp=None, max_depth=8, integrator=MIS, pick=1, frame0=0, second=0,
                 sobol=False, stats=False, env_rgb=(0.0, 0.0, 0.0), cam=None):
        self.id, self.scene_fn, self.light, self.shape, self.env = id, scene, light, shape, env
        self.spp = spp if spp is not None else (2 if shape == "strip" else 16)
        self.max_depth, self.integrator, self.pick, self.frame0, self.second = max_depth, integrator, pick, frame0, second
        self.sobol, self.stats, self.env_rgb, self.cam_fn = sobol, stats, tuple(env_rgb), cam

    @property
    def scene(self):
        return self.scene_fn()

    @property
    def camera(self):
        return self.cam_fn(W, H) if self.cam_fn else self.scene.cam

    def oracle_key(self):
        return (self.scene_fn.__name__, getattr(self.scene_fn, "args", ()), self.light, self.env, self.spp, self.max_depth, self.integrator, self.pick, self.frame0, self.second,
                self.sobol, self.env_rgb, getattr(self.cam_fn, "__name__", None))

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
        s, cam = case.scene, case.camera
        po.set_environment_map(env_map(case.env) if case.env else None)
        try:
            rng = host.fill_rng(SEED, W, H)
            kw = dict(max_depth=case.max_depth, integrator=case.integrator, env_light=case.light == "env", mesh_lights=case.light == "mesh",
                      mesh_light_pick=case.pick, triangle_materials=s.tri, textures=s.images, sobol=case.sobol, env=case.env_rgb)
            acc, st = po.render(s.view, cam, W, H, rng, spp=case.spp, frame0=case.frame0, **kw)
            if case.second:
                acc, st2 = po.render(s.view, cam, W, H, rng, accum=acc, spp=case.second, frame0=case.frame0 + case.spp, **kw)
                for f, _ in abi.Stats._fields_:
                    if isinstance(getattr(st, f), int):
                        setattr(st, f, getattr(st, f) + getattr(st2, f))
        finally:
            po.set_environment_map(None)
        _ORACLE[key] = (acc, rng, st)
    return _ORACLE[key]


# ---------------------------------------------------------------------- the census of the kernel tables (tests/test_gpu_kernel_census.py)
ENV_RGB = (0.3, 0.4, 0.6)                                   # a constant environment that is not black: an escaping ray carries it
FAMILIES = ("plain", "trimat")                              # the tables and their per-triangle-material twins (namespace trimat)
INTEGRATOR_NAMES = {PATH: "path", MIS: "mis", VOLUME: "volume"}
LIGHT_VARIANTS = ("env", "env_tex", "mesh", "mesh_tex")
_KNOWN_VARIANTS, _KNOWN_SHAPES = ("plain", "stats", "sobol", "tex") + LIGHT_VARIANTS, ("one", "strip", "pwg", "dense")


def _in_table(integrator, variant, residence, shape):
    """render_kernels<LDS, INTEGRATOR>() (trc_render_kernels.hpp), restated: is this entry non-null?  A variant or a shape this
    function has not heard of is taken to be everywhere, so that it shows as unreached until the census learns its rule."""
    if variant not in _KNOWN_VARIANTS or shape not in _KNOWN_SHAPES:
        return True
    if shape == "dense":                                    # k_render_dense: one kernel beside the tables, tracePath on a tree in LDS
        return integrator == PATH and variant == "plain" and residence == "lds"
    if shape == "pwg" and residence == "lds":               # persistent workgroups: trees read from memory only
        return False
    if variant in LIGHT_VARIANTS:
        return integrator == MIS
    if variant == "sobol":
        return integrator != VOLUME
    if variant == "stats":                                  # no statistics twin of the strip / persistent kernels
        return shape == "one"
    return True


def table_entries():
    """every entry of the kernel tables as (family, integrator, variant, residence, shape), from what the library names"""
    return [(f, i, v, r, sh) for f in FAMILIES for i in (PATH, MIS, VOLUME) for v in abi.KERNEL_VARIANTS for r in ("lds", "mem")
            for sh in abi.KERNEL_SHAPES if _in_table(i, v, r, sh)]


def census_cases():
    """one case for every entry that tests/test_gpu_light_oracle.py does not assert (the light variants of both families, the Tex
    entries of the plain one) and that is no dense launch (a frame of its own size: test_gpu_kernel_census.py renders those)"""
    out = []
    for (family, integ, variant, residence, shape) in table_entries():
        if variant in LIGHT_VARIANTS or (family == "plain" and variant == "tex") or shape == "dense":
            continue
        c = Case(f"{family}-{INTEGRATOR_NAMES[integ]}-{variant}-{residence}-{shape}", _bind(cornell, residence, variant == "tex", family == "trimat"),
                 shape=shape, spp=2 if shape == "strip" else 8, integrator=integ, sobol=variant == "sobol", stats=variant == "stats", env_rgb=ENV_RGB)
        c.entry = (family, integ, variant, residence, shape)
        out.append(c)
    return out


# ---------------------------------------------------------------------- the replay matrix (tests/test_gpu_primary_replay.py)
REPLAY_EYES = [((500.0, 40.0, -450.0), (200.0, 450.0, 250.0)),      # the matrix's camera
               ((455.0, 70.0, -500.0), (215.0, 430.0, 260.0)),      # the same, moved a little (a second launch from another eye)
               ((-450.0, 200.0, -350.0), (278.0, 278.0, 278.0))]    # from the far left: triangles of the small ball whose sn is -gn


def replay_camera(w, h, which=0):
    """pulled back from Cornell's open side and off its axis, aperture 0: part of the frame escapes, the lamp is seen from below, the
    ball and the cubes are in view (tests/test_replay_scenes.py holds it to that).  No component of lookFrom is zero."""
    look_from, look_at = REPLAY_EYES[which]
    return host.make_camera(look_from, look_at, (0.0, 1.0, 0.0), 0.0, w / h, float(np.deg2rad(50.0)), 10.0)


REPLAY_SCENES = {"trimat": ("mem", False, True, False, False), "tex": ("mem", True, False, False, True), "trimat+tex": ("mem", True, True, False, True),
                 # triangle 1 the dim emitter and 6 the Plastic (kept in the packed word); 1 kept and 6 of a cube's material (checkered: it reads uv);
                 # triangle 3, which the camera on the far left sees from its far side, a Lambert / the Plastic: the lobe knows sn from -sn
                 "dense-trimat": ("tiny", False, True, False, False, (11, 9, 15, 4, 0, 13, 8, 7, 3, 12, 17, 5)),
                 "dense-trimat-checker": ("tiny", False, True, False, True, (11, 12, 15, 8, 0, 13, 2, 7, 3, 9, 17, 5))}


def replay_scene(name):
    """the 1104-triangle ball (persistent workgroups) with random per-triangle materials / random images and checker cubes, every triangle
    material 19 / both; the 12-triangle ball (the dense kernel) with a material per triangle, plain and with checker cubes"""
    return cornell(*REPLAY_SCENES[name])


def primary_hits(s, cam, w, h, view_height=0):
    """what the camera ray of every pixel of the w x h frame meets, from the oracle's trace_rays (aperture 0: castRay's own arithmetic,
    v of a stacked view as kernelPathTracing takes it) -> (h, w) arrays: hit, emitter (the ray ends on a Diffuse material), triangle,
    material, and uv_read -- a hit that is no emitter, on a cube or a triangle whose material is a checker texture: its colour reads
    rec.uv, which a memo of fewer than 10 rows does not keep (render_block: memo_store); back -- a hit whose sn is not its gn (the
    memo keeps gn and one bit for the side)"""
    vh = view_height if 0 < view_height < h else h
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs.astype(F) / F(w)).ravel()
    v = ((ys % vh).astype(F) / F(vh)).ravel()
    f = lambda a: np.array([a.x, a.y, a.z], dtype=F)
    sample = f(cam.cornerLowLeft)[None] + f(cam.horizontal)[None] * u[:, None] + f(cam.vertical)[None] * v[:, None]
    o = np.repeat(f(cam.lookFrom)[None], len(u), 0)
    hits = po.trace_rays(s.view, po.make_rays(o, (sample - o).astype(F)), triangle_materials=s.tri)
    mat_type = np.array([s.view.materials[i].type for i in range(s.view.n_material)])
    tex_type = np.array([s.view.materials[i].textureInfo.type for i in range(s.view.n_material)])
    hit = hits["hit"] != 0
    material = np.where(hit, hits["material"], 0)
    emitter = hit & (mat_type[material] == abi.MAT_DIFFUSE)
    uv_read = hit & ~emitter & np.isin(hits["pType"], (abi.PRIM_CUBE, abi.PRIM_TRIANGLE)) & (tex_type[material] == abi.TEX_CHECKER)
    back = hit & (hits["sn"].view(np.uint32) != hits["gn"].view(np.uint32)).any(axis=1)
    sh = lambda a: a.reshape(h, w)
    return dict(hit=sh(hit), emitter=sh(emitter), triangle=sh(hit & (hits["pType"] == abi.PRIM_TRIANGLE)), material=sh(material), uv_read=sh(uv_read),
                back=sh(back))


def kept_pixels(hits, memo_rows):
    """the pixels whose primary hit the memo keeps: all of them with 10 rows, all but the uv readers with 7 or 8"""
    return np.ones_like(hits["hit"]) if memo_rows >= 10 else ~hits["uv_read"]
