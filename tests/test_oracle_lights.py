"""The oracle's statement of the project's own four features (oracle/README.md: per-triangle materials, image textures,
TRC_FLAG_ENV_LIGHT, TRC_FLAG_MESH_LIGHTS), pinned on the CPU: with no feature in effect the frame is the reference restatement's bit
for bit; the two lights land on float64 quadrature of their closed forms; and the cases of tests/test_gpu_light_oracle.py reach every
branch of traceMISLight, which is what makes that file's small frames sufficient."""
import numpy as np
import pytest

import light_oracle_cases as lc
from conftest import camera_rays
from oracle import pyoracle as po
from tracer_amd import abi, host

F = np.float32
INTEGRATORS = [abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS, abi.INTEGRATOR_VOLUME]


# ---------------------------------------------------------------------------------------------------- 1. no feature, same frame
def _scene(name):
    if name == "spheres":
        return host.HostScene(abi.SCENE_CORNELL_SPHERES)
    return host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1))


def _frame(view, cam, W, H, integrator, **kw):
    rng = host.fill_rng(21, W, H)
    acc, st = po.render(view, cam, W, H, rng, spp=4, integrator=integrator, **kw)
    return acc, rng, st


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
    for f in ("paths", "rays", "shaded", "n_descend", "n_return", "n_leaf_sphere", "n_leaf_square", "n_leaf_cube", "n_leaf_triangle", "n_hit_triangle"):
        assert getattr(a[2], f) == getattr(b[2], f), f


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", ["spheres", "ball"])
def test_no_feature_in_effect_is_the_reference_restatement(name, integrator):
    """a black map, no light triangle, an all-19 triangle array, or uniform images equal to the albedo: accumulator, RNG texture and
    counters of the plain call (tests/test_oracle_render.py holds that one to the committed frames)"""
    W, H = 32, 24
    sc, cam = _scene(name), host.prepare_camera(32, 24)
    v = sc.view
    plain = _frame(v, cam, W, H, integrator)
    assert plain[0][..., :3].max() > 0
    n_tri = v.n_index // 3
    _same(plain, _frame(v, cam, W, H, integrator, triangle_materials=np.full(max(n_tri, 1), 19, np.uint32)))
    if integrator == abi.INTEGRATOR_MIS:
        po.set_environment_map(np.zeros((8, 16, 3), F))
        try:
            _same(plain, _frame(v, cam, W, H, integrator, env_light=True))
        finally:
            po.set_environment_map(None)
        po.branch_counts(reset=True)
        _same(plain, _frame(v, cam, W, H, integrator, mesh_lights=True))               # material 19 is no emitter: no light triangle
        visited = po.branch_counts(reset=True)
        assert visited["pick_square5"] > 0 and visited["pick_light"] == 0              # (traceMISLight ran, with p = 0)
    # uniform images against the same scene with Constant albedo of the images' colours (colours whose bilinear blend is exact:
    # tests/test_gpu_textures.py uniform_pair), and an index not below the number of images against the material's own albedo
    from test_gpu_textures import uniform_pair
    tex, const, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES if name == "spheres" else abi.SCENE_CORNELL_MESH,
                                    None if name == "spheres" else host.Mesh.ball(4, 6, 0.1), seed=5)
    const_frame = _frame(const.view, cam, W, H, integrator)
    _same(const_frame, _frame(tex.view, cam, W, H, integrator, textures=imgs))
    assert not np.array_equal(const_frame[0].view(np.uint32), plain[0].view(np.uint32))
    own = _scene(name)                                                                    # every non-emitter material Constant, its own albedo
    for i in range(own.view.n_material):
        if own.view.materials[i].type != abi.MAT_DIFFUSE:
            own.view.materials[i].textureInfo.type = abi.TEX_CONSTANT
    own_frame = _frame(own.view, cam, W, H, integrator)
    _same(own_frame, _frame(tex.view, cam, W, H, integrator))                             # nothing uploaded: an Image material is its albedo
    for i in range(tex.view.n_material):
        tex.view.materials[i].textureInfo.textureIndex += len(imgs)                       # every index past the images
    _same(own_frame, _frame(tex.view, cam, W, H, integrator, textures=imgs))


def test_image_lookup_is_the_stated_one():
    """the Image case of texture_value through orc_material_F (a Lambert material: F = colour * wi.z / pi) against the float32 restatement
    at the top of tests/test_gpu_textures.py, the non-finite-uv rule included"""
    from test_gpu_textures import ref_sample
    import ctypes as C
    rng = np.random.default_rng(2)
    img = rng.random((7, 13, 3), dtype=F)
    m = abi.Material()
    m.type = abi.MAT_LAMBERT
    m.textureInfo.type, m.textureInfo.textureIndex = abi.TEX_IMAGE, 0
    m.textureInfo.albedo.x = m.textureInfo.albedo.y = m.textureInfo.albedo.z = 0.25
    uv = np.concatenate([rng.uniform(-0.5, 1.5, (2000, 2)).astype(F),
                         np.array([[np.nan, 0.3], [0.3, np.inf], [-np.inf, 0.2], [3e38, 0.5], [7.0, -5.0], [0, 0], [1, 1], [0.5, 1 - 2.0 ** -24]], F)])
    want = ref_sample(img, uv)
    L = po.lib()
    f3 = lambda a: (C.c_float * len(a))(*a)
    wo, wi, uu = f3([0.0, 0.6, 0.8]), f3([0.6, 0.0, 0.8]), f3([0.3, 0.3])
    got = np.empty((len(uv), 3), F)
    with po._features(L, textures=[img]):
        for k, p in enumerate(uv):
            f, pdf = (C.c_float * 3)(), C.c_float()
            L.orc_material_F(C.byref(m), wo, wi, f3([float(p[0]), float(p[1])]), uu, f, C.byref(pdf))
            got[k] = f[:]
    lobe = F(0.8) / F(np.float32(np.pi))                                      # Lambert::F = wi.z / pi, times the colour
    f_lobe = np.empty(1, F)
    with po._features(L):                                                     # nothing uploaded: the albedo
        f, pdf = (C.c_float * 3)(), C.c_float()
        L.orc_material_F(C.byref(m), wo, wi, f3([0.5, 0.5]), uu, f, C.byref(pdf))
        f_lobe[0] = F(f[0]) / F(0.25)
    assert abs(float(f_lobe[0]) - float(lobe)) < 1e-6
    assert np.array_equal(got.view(np.uint32), (want * f_lobe[0]).astype(F).view(np.uint32))


def test_trace_rays_report_each_triangles_material():
    s = lc.cornell("lds")
    rays = camera_rays(s.cam, lc.W, lc.H)
    plain = po.trace_rays(s.view, rays)
    hits = po.trace_rays(s.view, rays, triangle_materials=s.tri)
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 20 and np.all(plain["material"][tri] == 19)
    assert np.array_equal(hits["material"][tri], s.tri[hits["pIndex"][tri]])
    assert np.array_equal(hits["material"][~tri], plain["material"][~tri])
    for f in ("t", "p", "uv", "pIndex"):
        assert np.array_equal(hits[f], plain[f])


# ---------------------------------------------------------------------------------------------------- 2. against float64 quadrature
def _region_z(resid, regions):
    """per region and channel: mean of the pixels' residuals over its standard error, estimated from those pixels (they are independent:
    every pixel has its own RNG stream)"""
    z = []
    for r in regions:
        px = resid[r]
        assert px.shape[0] >= 100
        se = px.std(axis=0, ddof=1) / np.sqrt(px.shape[0])
        assert np.all(se > 0)
        z.append(px.mean(axis=0) / se)
    return np.array(z)


def test_environment_only_floor_against_quadrature():
    """Two Lambert squares under a sun-and-sky map, one bounce (max_depth 2): every pixel's expectation is albedo * E, E the float64
    irradiance integral of tests/test_gpu_envlight.py.  Eight regions (two albedos x four bands of rows) x 3 channels within 5 standard
    errors.  256 samples per pixel: chosen on the CPU with room (largest |z| printed below; 2.27 when this was written)."""
    from test_gpu_envlight import irradiance_integral
    s = lc.floor()
    env = lc.el.sun_sky(256, 128, sun=(0.3, 0.7), sun_radius=0.05, sun_power=2000.0)
    E = irradiance_integral(env)
    W, H = lc.W, lc.H
    po.set_environment_map(env)
    try:
        acc, _ = po.render(s.view, s.cam, W, H, host.fill_rng(31, W, H), spp=256, max_depth=2, integrator=abi.INTEGRATOR_MIS, env_light=True)
    finally:
        po.set_environment_map(None)
    hits = po.trace_rays(s.view, camera_rays(s.cam, W, H))
    assert np.all(hits["hit"] != 0)
    mats = [s.view.materials[i] for i in range(s.view.n_material)]
    albedo = np.array([[mats[m].textureInfo.albedo.x, mats[m].textureInfo.albedo.y, mats[m].textureInfo.albedo.z] for m in hits["material"]], np.float64)
    assert sorted(set(np.round(albedo[:, 0], 3))) == [0.3, 0.7]
    resid = acc[..., :3].reshape(-1, 3).astype(np.float64) - albedo * E[None]
    rows = np.repeat(np.arange(H), W)
    regions = [(np.round(albedo[:, 0], 3) == a) & (rows * 4 // H == b) for a in (0.3, 0.7) for b in range(4)]
    z = _region_z(resid, regions)
    print(f"environment-only floor: largest |z| {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 5, z


@pytest.mark.parametrize("pick", [1, 0])
def test_triangle_lamp_over_a_floor_against_quadrature(pick):
    """The 1 x 1 lamp of four triangles over a Lambert mesh floor of tests/test_gpu_triangle_materials.py, one bounce (max_depth 2): every
    pixel's expectation is the Gauss-Legendre integral floor_radiance at its floor point.  TRC_FLAG_MESH_LIGHTS with the mesh's light
    sample (pick 1) and the BSDF-only arm (knob mesh_light_pick = 0) land on the same number: 12 regions x 3 channels within 5 standard
    errors each.  64 / 256 samples per pixel: chosen on the CPU with room (largest |z| printed; 2.03 and 2.17 when this was written)."""
    from test_gpu_triangle_materials import LIGHT_OVER_FLOOR, floor_radiance
    if "lamp" not in lc._SCENES:
        lc._SCENES["lamp"] = lc._from_pbrt("lamp", LIGHT_OVER_FLOOR, True)
    s = lc._SCENES["lamp"]
    W, H = lc.W, lc.H
    assert s.view.n_square == 0
    acc, _ = po.render(s.view, s.cam, W, H, host.fill_rng(41 + pick, W, H), spp=64 if pick else 256, max_depth=2, integrator=abi.INTEGRATOR_MIS,
                       mesh_lights=True, mesh_light_pick=pick, triangle_materials=s.tri)
    f = lambda a: np.array([a.x, a.y, a.z], np.float64)
    cam = s.cam
    eye, cll, hor, ver = f(cam.lookFrom), f(cam.cornerLowLeft), f(cam.horizontal), f(cam.vertical)
    ys, xs = np.mgrid[0:H, 0:W]
    d = cll[None, None] + hor[None, None] * (xs / np.float64(W))[..., None] + ver[None, None] * (ys / np.float64(H))[..., None] - eye
    pts = eye[None, None] + d * (-eye[1] / d[..., 1])[..., None]
    want = floor_radiance(pts[..., [0, 2]].reshape(-1, 2))
    assert want.max() > 0.05
    resid = acc[..., :3].reshape(-1, 3).astype(np.float64) - want[:, None]
    rows, cols = np.repeat(np.arange(H), W), np.tile(np.arange(W), H)
    regions = [(rows * 3 // H == a) & (cols * 4 // W == b) for a in range(3) for b in range(4)]
    z = _region_z(resid, regions)
    print(f"triangle lamp, mesh_light_pick = {pick}: largest |z| {np.abs(z).max():.2f}, frame mean / closed form {acc[..., :3].mean() / want.mean():.4f}")
    assert np.abs(z).max() < 5, z


# ---------------------------------------------------------------------------------------------------- 3. every branch is reached
REQUIRED = ["pick_light", "pick_light_p1", "pick_square5", "pick_square6", "support", "no_support", "lipdf_guard", "zero_pdf_no_shadow_ray",
            "no_sample_beckmann", "no_sample_metal", "no_sample_glass", "env_depth_cutoff", "escape_weighted", "escape_zero_pdf",
            "escape_other_lobe", "escape_camera", "tri_emitter_weighted", "tri_emitter_w1", "emitter_shared", "emitter_not_shared",
            "plastic_lambert_lobe", "plastic_beckmann_lobe", "no_squares_no_sample"]


def test_the_gpu_cases_reach_every_branch():
    """the cases of tests/test_gpu_light_oracle.py, through the oracle alone: every branch of traceMISLight at least once, for the light
    it belongs to; materials of all five kinds at path vertices"""
    lc._ORACLE.clear()
    per_light = {"env": {}, "mesh": {}}
    for case in lc.matrix() + lc.further():
        po.branch_counts(reset=True)
        acc, rng, st = lc.oracle_frame(case)
        assert np.isfinite(acc).all() and st.paths == lc.W * lc.H * (case.spp + case.second)
        for k, n in po.branch_counts(reset=True).items():
            per_light[case.light][k] = per_light[case.light].get(k, 0) + n
    assert sorted(REQUIRED) == sorted(po.BRANCHES)
    env_only = {"env_depth_cutoff", "escape_weighted", "escape_zero_pdf", "escape_other_lobe", "escape_camera", "emitter_not_shared"}
    mesh_only = {"lipdf_guard", "tri_emitter_weighted", "tri_emitter_w1", "no_squares_no_sample"}
    for light, counts in per_light.items():
        want = [b for b in REQUIRED if b not in (mesh_only if light == "env" else env_only)]
        zero = [b for b in want if counts.get(b, 0) == 0]
        print(light, {b: counts[b] for b in want})
        assert not zero, (light, zero)
