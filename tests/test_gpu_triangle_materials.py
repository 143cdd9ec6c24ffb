"""Per-triangle materials on the GPU (trc_upload_triangle_materials, include/tracer_abi.h): refusals that change nothing, an all-19
array that changes nothing, relabelling invariance bit for bit (every integrator, SPPM, the work counters, the G-buffer, three upload
paths, both tree residences, strips / persistent workgroups / small blocks, the fast-math build), trc_trace_rays' hit.material, the
G-buffer's id and albedo planes, and a mesh area light over a mesh floor against a float64 integral."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, camera_rays, random_rays
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
INTEGRATORS = [abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS, abi.INTEGRATOR_VOLUME]

_SCENES = {}


def scene(residence, analytic_leaves_only=False):
    """'lds': Cornell + a 48-triangle ball (the whole tree is staged in LDS); 'mem': Cornell + coatball.obj (config 3's mesh)"""
    key = (residence, analytic_leaves_only)
    if key not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.golden("coatball")
        _SCENES[key] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=analytic_leaves_only)
    return _SCENES[key]


def with_materials(view, mats):
    """a copy of a scene view over another material table (the caller keeps `mats` alive)"""
    v = abi.Scene.from_buffer_copy(view)
    v.materials = C.cast(mats, C.POINTER(abi.Material))
    v.n_material = len(mats)
    return v


class Relabelled:
    """Material 19 copied to a new slot k = n_material, a different material (an orange Lambert) put at 19, and every analytic
    primitive that named 19 (Cornell's small cube, testMaterial) pointed at k: only the triangles still name 19."""

    def __init__(self, view):
        n = view.n_material
        self.k = n
        self.mats = (abi.Material * (n + 1))()
        for i in range(n):
            self.mats[i] = view.materials[i]
        self.mats[n] = view.materials[19]
        other = abi.Material()
        other.type, other.medium, other.roughness = abi.MAT_LAMBERT, abi.MEDIUM_NIL, 1.0
        other.textureInfo.type = abi.TEX_CONSTANT
        other.textureInfo.albedo.x, other.textureInfo.albedo.y, other.textureInfo.albedo.z = 0.8, 0.4, 0.1
        self.mats[19] = other
        self._keep = []

    def view(self, base):
        """a copy of `base` over the relabelled table and primitive arrays"""
        v = with_materials(base, self.mats)
        for ptr, count, ctype in (("sphereList", "n_sphere", abi.Sphere), ("squareList", "n_square", abi.Square), ("cubeList", "n_cube", abi.Cube)):
            n = getattr(base, count)
            if n == 0:
                continue
            arr = (ctype * n)()
            for i in range(n):
                arr[i] = getattr(base, ptr)[i]
                if arr[i].material == 19:
                    arr[i].material = self.k
            self._keep.append(arr)
            setattr(v, ptr, C.cast(arr, C.POINTER(ctype)))
        return v


def upload(t, residence, path, rel=None):
    if path == "scene":
        v = scene(residence).view
        t.upload_scene(v if rel is None else rel.view(v))
    elif path == "lbvh":
        v = scene(residence).leaves_view()
        t.upload_scene_lbvh(v if rel is None else rel.view(v))
    else:
        v = scene(residence, analytic_leaves_only=True).view
        t.upload_scene_device(v if rel is None else rel.view(v), abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES)


def n_tri(residence):
    return scene(residence).view.n_index // 3


def render(t, spp, integrator, small=None, stats=False, seed=9):
    t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    t.seed(seed); t.clear_accum(); t.reset_stats()
    t.render(spp=spp, integrator=integrator, small_blocks=small, collect_stats=stats)
    st = t.stats()
    counters = tuple(getattr(st, f) for f, _ in abi.Stats._fields_ if f not in ("kernel_ms", "schedule_ms", "launches"))
    return t.download_accum(), t.download_rng(), counters


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        with pytest.raises(TracerError) as e:
            fresh.upload_triangle_materials(np.full(3, 19, np.uint32))
        assert e.value.status == abi.ERR_NO_SCENE
        with pytest.raises(TracerError) as e:
            fresh.upload_triangle_materials(None)
        assert e.value.status == abi.ERR_NO_SCENE
    rel = Relabelled(scene("lds").view); k = rel.k
    upload(gpu, "lds", "scene", rel)
    n = n_tri("lds")
    gpu.upload_triangle_materials(np.full(n, k, np.uint32))
    before = render(gpu, 8, abi.INTEGRATOR_MIS)
    bad = [np.zeros(0, np.uint32), np.full(n - 1, 19, np.uint32), np.full(n + 1, 19, np.uint32), np.full(n, len(rel.mats), np.uint32),
           np.r_[np.full(n - 1, 19, np.uint32), np.uint32(0xFFFFFFFF)]]
    for arr in bad:
        with pytest.raises(TracerError) as e:
            gpu.upload_triangle_materials(arr)
        assert e.value.status == abi.ERR_INVALID_ARG
        assert same(render(gpu, 8, abi.INTEGRATOR_MIS), before)
    # material == NULL with n > 0
    assert gpu._L.trc_upload_triangle_materials(gpu._h, None, n) == abi.ERR_INVALID_ARG
    assert same(render(gpu, 8, abi.INTEGRATOR_MIS), before)


# ----------------------------------------------------------------------------------------------------------- all 19
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_all_19_changes_nothing(gpu, integrator):
    upload(gpu, "mem", "scene")
    plain = render(gpu, 4, integrator)
    gpu.upload_triangle_materials(np.full(n_tri("mem"), 19, np.uint32))
    assert same(render(gpu, 4, integrator), plain)
    gpu.upload_triangle_materials(None)
    assert same(render(gpu, 4, integrator), plain)


def test_all_19_changes_nothing_sppm(gpu):
    upload(gpu, "mem", "scene")
    plain = sppm_run(gpu)
    gpu.upload_triangle_materials(np.full(n_tri("mem"), 19, np.uint32))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sppm_run(gpu), plain))


# ----------------------------------------------------------------------------------------------------------- relabelling
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_relabelled_frames_are_bit_identical(gpu, residence, integrator):
    rel = Relabelled(scene(residence).view); k = rel.k
    for spp, small in ((1, None), (16, None), (16, True)):          # strips of blocks, whole blocks (persistent on 'mem'), 4x4 blocks
        upload(gpu, residence, "scene")
        want = render(gpu, spp, integrator, small)
        upload(gpu, residence, "scene", rel)
        other = render(gpu, spp, integrator, small)
        assert not same(other, want)                                   # 19 is another material now ...
        gpu.upload_triangle_materials(np.full(n_tri(residence), k, np.uint32))
        assert same(render(gpu, spp, integrator, small), want)        # ... and the triangles name its copy
        gpu.upload_triangle_materials(None)                            # back to 19
        assert same(render(gpu, spp, integrator, small), other)


@pytest.mark.parametrize("path", ["lbvh", "device"])
@pytest.mark.parametrize("integrator", [abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS])
def test_relabelled_frames_other_upload_paths(gpu, path, integrator):
    rel = Relabelled(scene("mem").view); k = rel.k
    upload(gpu, "mem", path)
    want = render(gpu, 4, integrator)
    upload(gpu, "mem", path, rel)
    gpu.upload_triangle_materials(np.full(n_tri("mem"), k, np.uint32))
    assert same(render(gpu, 4, integrator), want)
    upload(gpu, "mem", path, rel)                                     # a new upload is back to 19
    assert not same(render(gpu, 4, integrator), want)


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_relabelled_counters(gpu, residence):
    rel = Relabelled(scene(residence).view); k = rel.k
    for integrator in INTEGRATORS:
        upload(gpu, residence, "scene")
        want = render(gpu, 2, integrator, stats=True)
        upload(gpu, residence, "scene", rel)
        gpu.upload_triangle_materials(np.full(n_tri(residence), k, np.uint32))
        got = render(gpu, 2, integrator, stats=True)
        assert same(got, want) and got[2][1] > 0 and got[2][8] > 0      # rays, triangle leaves


def sppm_run(t, frames=3):
    t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    t.seed(5); t.sppm_init(77); t.sppm_frames(frames)
    cam, pho, mark, count, _ = t.sppm_download()
    return t.download_accum(), t.download_rng(), cam, pho, mark, count


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_relabelled_sppm_records(gpu, residence):
    rel = Relabelled(scene(residence).view); k = rel.k
    upload(gpu, residence, "scene")
    want = sppm_run(gpu)
    upload(gpu, residence, "scene", rel)
    gpu.upload_triangle_materials(np.full(n_tri(residence), k, np.uint32))
    got = sppm_run(gpu)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_relabelled_gbuffer(gpu, residence):
    rel = Relabelled(scene(residence).view); k = rel.k
    upload(gpu, residence, "scene")
    render(gpu, 1, abi.INTEGRATOR_PATH)
    gpu.denoise()
    want = gpu.download_gbuffer()
    upload(gpu, residence, "scene", rel)
    gpu.upload_triangle_materials(np.full(n_tri(residence), k, np.uint32))
    render(gpu, 1, abi.INTEGRATOR_PATH)
    gpu.denoise()
    got = gpu.download_gbuffer()
    for plane in ("depth", "normal", "albedo"):
        assert got[plane].tobytes() == want[plane].tobytes(), plane
    assert (want["id"] == 19).any()
    assert np.array_equal(got["id"], np.where(want["id"] == 19, np.uint32(k), want["id"]))


def test_relabelled_frames_fast_math():
    with Tracer(0, fast_math=True) as t:
        rel = Relabelled(scene("mem").view); k = rel.k
        for integrator in (abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS):
            upload(t, "mem", "scene")
            want = render(t, 4, integrator)
            upload(t, "mem", "scene", rel)
            t.upload_triangle_materials(np.full(n_tri("mem"), k, np.uint32))
            assert same(render(t, 4, integrator), want)


# ----------------------------------------------------------------------------------------------------------- trc_trace_rays
@pytest.mark.parametrize("production", [False, True])
def test_trace_rays_report_each_triangles_material(gpu, production):
    sc = scene("mem")
    n = n_tri("mem")
    table = np.random.default_rng(3).integers(0, sc.view.n_material, n).astype(np.uint32)
    rays = np.concatenate([camera_rays(host.prepare_camera(320, 240), 320, 240), random_rays(20000, 5, inside_only=True)])
    gpu.upload_scene(sc.view)
    plain = gpu.trace_rays(rays, production=production)
    gpu.upload_triangle_materials(table)
    got = gpu.trace_rays(rays, production=production)
    tri = (got["hit"] != 0) & (got["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 1000 and ((got["hit"] != 0) & ~tri).sum() > 1000
    assert np.array_equal(got["material"][tri], table[got["pIndex"][tri]])
    assert (plain["material"][tri] == 19).all()
    assert np.array_equal(got["material"][~tri], plain["material"][~tri])
    for f in got.dtype.names:
        if f != "material":
            assert got[f].tobytes() == plain[f].tobytes(), f


# ----------------------------------------------------------------------------------------------------------- G-buffer
def test_gbuffer_id_and_albedo_follow_the_triangles(gpu):
    sc = scene("mem")
    v = sc.view
    n = n_tri("mem")
    # four new Lambert materials with Constant albedos (the checker of 19 would make the albedo depend on uv), shuffled over the triangles
    alb4 = ((0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.5, 0.25, 0.75))
    mats = (abi.Material * (v.n_material + len(alb4)))()
    for i in range(v.n_material):
        mats[i] = v.materials[i]
    for j, alb in enumerate(alb4):
        m = abi.Material()
        m.type, m.medium, m.roughness = abi.MAT_LAMBERT, abi.MEDIUM_NIL, 1.0
        m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z = alb
        mats[v.n_material + j] = m
    table = (v.n_material + np.random.default_rng(8).permutation(n) % len(alb4)).astype(np.uint32)
    gpu.upload_scene(with_materials(v, mats))
    gpu.upload_triangle_materials(table)
    render(gpu, 1, abi.INTEGRATOR_PATH)
    gpu.denoise()
    g = gpu.download_gbuffer().ravel()
    hits = gpu.trace_rays(camera_rays(host.prepare_camera(W, H), W, H), production=True)
    hit = hits["hit"] != 0
    tri = hit & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 100
    want_id = np.where(tri, table[np.where(tri, hits["pIndex"], 0)], hits["material"])
    assert np.array_equal(g["id"][hit], want_id[hit])
    albedo = np.array([[m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z] for m in mats], F)
    for m_idx in np.unique(g["id"][tri]):
        sel = tri & (g["id"] == m_idx)
        assert np.array_equal(g["albedo"][sel], np.broadcast_to(albedo[m_idx], (sel.sum(), 3)))
    assert len(np.unique(g["id"][tri])) == 4


TWO_MESHES = '''LookAt 0 6 0  0 0 0  0 0 1
Camera "perspective" "float fov" [ 60 ]
Film "image" "integer xresolution" [ 64 ] "integer yresolution" [ 48 ]
WorldBegin
Material "matte" "rgb Kd" [ 0.5 0.5 0.5 ]
Shape "trianglemesh" "integer indices" [ 0 1 4 0 4 3  1 2 5 1 5 4 ] "point P" [ -4 0 -3  -2 0 -3  -0.1 0 -3  -4 0 3  -2 0 3  -0.1 0 3 ]
Material "matte" "rgb Kd" [ 0.25 0.5 0.75 ]
Shape "trianglemesh" "integer indices" [ 0 1 4 0 4 3  1 2 5 1 5 4 ] "point P" [ 0.1 0 -3  2 0 -3  4 0 -3  0.1 0 3  2 0 3  4 0 3 ]
WorldEnd
'''


def test_gbuffer_two_meshes_two_images(gpu, tmp_path):
    """Two meshes whose materials are Image materials naming two uniform images: each shows its own image's colour"""
    p = tmp_path / "two.pbrt"
    p.write_text(TWO_MESHES)
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(str(p), triangle_materials=True)
    v = sc.view
    meshes = [s for s in shapes if s.mapped_type == abi.PRIM_TRIANGLE]
    ma, mb = meshes[0].mapped_material, meshes[1].mapped_material
    assert ma != mb and ma > 19 and mb > 19
    mats = (abi.Material * v.n_material)()
    for i in range(v.n_material):
        mats[i] = v.materials[i]
    colours = [F([0.25, 0.5, 1.0]), F([1.0, 0.125, 0.0])]
    for img, m in enumerate((ma, mb)):
        mats[m].textureInfo.type = abi.TEX_IMAGE
        mats[m].textureInfo.textureIndex = img
    try:
        gpu.upload_scene(with_materials(v, mats))
        gpu.upload_textures([np.broadcast_to(c, (4, 4, 3)).copy() for c in colours])
        gpu.upload_triangle_materials(tri)
        gpu.set_camera(cam); gpu.resize(info.xres, info.yres); gpu.seed(3); gpu.clear_accum()
        gpu.render(spp=1, integrator=abi.INTEGRATOR_PATH)
        gpu.denoise()
        g = gpu.download_gbuffer().ravel()
    finally:
        gpu.upload_textures([])
    for m, c in ((ma, colours[0]), (mb, colours[1])):
        sel = g["id"] == m
        assert sel.sum() > 100, m
        assert np.array_equal(g["albedo"][sel], np.broadcast_to(c, (sel.sum(), 3)))
    assert not (g["id"] == 19).any()


# ----------------------------------------------------------------------------------------------------------- area light
LIGHT_H, LIGHT_A, LE, RHO = 2.0, 0.5, 4.0, 0.6
LIGHT_OVER_FLOOR = f'''LookAt 0 1.5 0  0 0 0  0 0 1
Camera "perspective" "float fov" [ 70 ]
Film "image" "integer xresolution" [ 40 ] "integer yresolution" [ 40 ]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ {LE} {LE} {LE} ]
  Shape "trianglemesh" "integer indices" [ 0 1 4  1 2 4  2 3 4  3 0 4 ]
        "point P" [ -{LIGHT_A} {LIGHT_H} -{LIGHT_A}  {LIGHT_A} {LIGHT_H} -{LIGHT_A}  {LIGHT_A} {LIGHT_H} {LIGHT_A}  -{LIGHT_A} {LIGHT_H} {LIGHT_A}  0 {LIGHT_H} 0 ]
        "normal N" [ 0 -1 0  0 -1 0  0 -1 0  0 -1 0  0 -1 0 ]
AttributeEnd
Material "matte" "rgb Kd" [ {RHO} {RHO} {RHO} ]
# the floor's inner vertex is off the centre pixel's ray (a ray through a shared vertex may slip between the triangles)
Shape "trianglemesh" "integer indices" [ 0 1 4 0 4 3  1 2 5 1 5 4  3 4 7 3 7 6  4 5 8 4 8 7 ]
      "point P" [ -20 0 -20  0.37 0 -20  20 0 -20  -20 0 0.29  0.37 0 0.29  20 0 0.29  -20 0 20  0.37 0 20  20 0 20 ]
      "normal N" [ 0 1 0  0 1 0  0 1 0  0 1 0  0 1 0  0 1 0  0 1 0  0 1 0  0 1 0 ]
WorldEnd
'''


def floor_radiance(points):
    """rho / pi * integral over the light of Le |cos_l| cos_l cos_f / r^2 dA, float64 (Gauss-Legendre, 48 x 48 nodes).
    The integrand is what the kernels do: a Lambert bounce (cosine sampled: weight rho) that reaches the emitter, which returns
    Le * |dot(-d, -gn)| (dev_integrator.hpp path_step; gn = the light's unit vertex normal); cos_l cos_f / r^2 dA = cos_f d(omega)."""
    x, w = np.polynomial.legendre.leggauss(48)
    lx, lz = np.meshgrid(x * LIGHT_A, x * LIGHT_A, indexing="ij")
    wa = np.outer(w, w) * LIGHT_A * LIGHT_A
    out = np.empty(len(points))
    for i, (px, pz) in enumerate(points):
        dx, dz = lx - px, lz - pz
        r2 = dx * dx + dz * dz + LIGHT_H * LIGHT_H
        cos = LIGHT_H / np.sqrt(r2)                       # cos_l = cos_f: the light faces straight down onto the floor
        out[i] = (wa * LE * cos * cos * cos / r2).sum()
    return np.float64(np.float32(RHO)) / np.pi * out


def test_mesh_area_light_over_a_mesh_floor(gpu, tmp_path):
    p = tmp_path / "light.pbrt"
    p.write_text(LIGHT_OVER_FLOOR)
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(str(p), triangle_materials=True)
    v = sc.view
    assert v.n_square == 0 and v.n_sphere == 0 and info.n_triangle_material_conflicts == 0
    light, floor = [s for s in shapes if s.mapped_type == abi.PRIM_TRIANGLE]
    assert v.materials[int(light.mapped_material)].type == abi.MAT_DIFFUSE and v.materials[19].type == abi.MAT_DIFFUSE
    assert v.materials[int(floor.mapped_material)].type == abi.MAT_LAMBERT
    w_, h_ = info.xres, info.yres
    gpu.upload_scene(v); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(w_, h_)
    # without the array the floor is the light's material (19 = the first mesh's): it glows with Le
    gpu.seed(1); gpu.clear_accum(); gpu.render(spp=4, max_depth=2, integrator=abi.INTEGRATOR_PATH)
    glow = gpu.download_accum()[..., :3].astype(np.float64)
    gpu.upload_triangle_materials(tri)
    frames = []
    for seed in range(16):
        gpu.seed(100 + seed); gpu.clear_accum()
        gpu.render(spp=256, max_depth=2, integrator=abi.INTEGRATOR_PATH)
        frames.append(gpu.download_accum()[..., :3].astype(np.float64))
    frames = np.stack(frames)                                 # (16, h, w, 3): independent estimates of every pixel
    # every sample of pixel (x, y) starts on the ray through u = x / W, v = y / H (no sub-pixel jitter, B-2; lens radius 0): its floor point
    f = lambda a: np.array([a.x, a.y, a.z], np.float64)
    eye, cll, hor, ver = f(cam.lookFrom), f(cam.cornerLowLeft), f(cam.horizontal), f(cam.vertical)
    ys, xs = np.mgrid[0:h_, 0:w_]
    d = cll[None, None] + hor[None, None] * (xs / np.float64(w_))[..., None] + ver[None, None] * (ys / np.float64(h_))[..., None] - eye
    pts = eye[None, None] + d * (-eye[1] / d[..., 1])[..., None]
    want = floor_radiance(pts[..., [0, 2]].reshape(-1, 2)).reshape(h_, w_)
    mean = frames.mean(axis=0)
    se = frames.std(axis=0, ddof=1) / np.sqrt(len(frames))
    assert want.max() > 0.05 and (se > 0).all(), np.argwhere(se[..., 0] == 0)[:5]
    z = (mean - want[..., None]) / se
    assert np.abs(z).max() < 6, np.abs(z).max()
    assert abs(z.mean()) < 0.2, z.mean()                      # no bias over the 1600 pixels
    assert np.abs(mean.mean() / want.mean() - 1) < 0.01
    # the glowing floor of the call-less frame is nowhere near it
    assert glow.mean() > 3 * want.mean()
    gpu.upload_triangle_materials(None)


# ----------------------------------------------------------------------------------------------------------- example host
def test_example_renders_per_triangle_materials(gpu, tmp_path):
    p = tmp_path / "light.pbrt"
    p.write_text(LIGHT_OVER_FLOOR)
    exe = os.path.join(ROOT, "examples", "trc_render")
    out = tmp_path / "frame.png"
    r = subprocess.run([exe, "--pbrt", str(p), "--triangle-materials", "--spp", "16", "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    img = host.load_png(str(out))
    assert img.shape[:2] == (40, 40) and img.max() > 0
    sc, cam, info, shapes, tri = host.HostScene.from_pbrt(str(p), triangle_materials=True)
    gpu.upload_scene(sc.view); gpu.upload_triangle_materials(tri); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0))
    gpu.resize(info.xres, info.yres); gpu.seed(0x5EED0000); gpu.clear_accum()
    gpu.render(spp=16, integrator=abi.INTEGRATOR_PATH)
    want, _ = gpu.tonemap()
    assert np.array_equal((img * 255 + 0.5).astype(np.uint8)[::-1], want[..., :3])
    r = subprocess.run([exe, "--triangle-materials", "--spp", "1", "--out", str(tmp_path / "x.png")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2
