"""Image textures on the GPU (trc_upload_textures, tracer_abi.h): the lookup against a float32 numpy restatement bit for bit, uniform
images against the same scene with Constant albedo (every integrator, both tree residences, strips / one-wavefront workgroups /
persistent workgroups, small blocks, SPPM, a 1080p frame), the index rules, error codes, the G-buffer's albedo plane and the
fast-math build.  Every fixture is generated here from a seed."""
import numpy as np
import pytest

from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32


def ref_sample(img, uv):
    """the stated lookup in float32, one operation at a time (numpy does not contract): img (h, w, 3) rows bottom-up"""
    uv = np.asarray(uv, dtype=F).reshape(-1, 2)
    u, v = uv[:, 0].copy(), uv[:, 1].copy()
    u[~np.isfinite(u)] = 0
    v[~np.isfinite(v)] = 0
    u, v = np.clip(u, F(-1), F(2)), np.clip(v, F(-1), F(2))          # finite components clamped (u * w stays finite)
    h, w = img.shape[:2]
    x = u * F(w) - F(0.5)
    y = v * F(h) - F(0.5)
    fx0, fy0 = np.floor(x), np.floor(y)
    fx, fy = (x - fx0)[:, None], (y - fy0)[:, None]

    def clampi(f, n):
        return np.where(f < 0, 0, np.where(f > F(n - 1), n - 1, np.clip(f, 0, n - 1).astype(np.int64)))
    x0, x1 = clampi(fx0, w), clampi(fx0 + F(1), w)
    y0, y1 = clampi(fy0, h), clampi(fy0 + F(1), h)
    one = F(1)
    top = (one - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (one - fx) * img[y1, x0] + fx * img[y1, x1]
    return ((one - fy) * top + fy * bot).astype(F)


@pytest.fixture(scope="module")
def hooks_gpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def test_sampler_matches_restatement(hooks_gpu):
    rng = np.random.default_rng(1)
    sizes = [(1, 1), (5, 7), (64, 64), (17, 33), (1, 9), (128, 2)]
    imgs = [rng.random((h, w, 3), dtype=F) * F(4) for h, w in sizes]
    hooks_gpu.upload_textures(imgs)
    special = np.array([0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1], dtype=F)
    grid = np.stack(np.meshgrid(special, special), axis=-1).reshape(-1, 2)
    nonfinite = np.array([[np.nan, 0.3], [0.3, np.nan], [np.inf, 0.7], [-np.inf, 0.2], [0.4, np.inf], [np.nan, -np.inf],
                          [3e38, 0.5], [-3e38, 0.25], [0.5, 1e30], [7.0, -5.0], [2.0, -1.0], [1.9, -0.9]], dtype=F)
    for k, img in enumerate(imgs):
        h, w = img.shape[:2]
        centres = np.stack(np.meshgrid((np.arange(w) + F(0.5)) / F(w), (np.arange(h) + F(0.5)) / F(h)), axis=-1).reshape(-1, 2).astype(F)
        edges = np.stack(np.meshgrid(np.arange(w + 1) / F(w), np.arange(h + 1) / F(h)), axis=-1).reshape(-1, 2).astype(F)
        n = 10 ** 6 if k < 3 else 10 ** 5
        uv = np.concatenate([rng.uniform(-0.5, 1.5, size=(n, 2)).astype(F), grid, nonfinite, centres, edges])
        got = hooks_gpu.texture_sample(k, uv)
        exp = ref_sample(img, uv)
        assert np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f"image {k} {img.shape}"
        # texel centres reproduce the texels
        assert np.array_equal(hooks_gpu.texture_sample(k, centres), img.reshape(-1, 3))
    with pytest.raises(TracerError):
        hooks_gpu.texture_sample(len(imgs), np.zeros((1, 2), F))
    hooks_gpu.upload_textures([])


COLOURS = [0.0, 0.5, 0.25, 0.125]


def uniform_pair(kind, mesh=None, seed=0, light_too=False, sizes=((1, 1), (5, 7), (64, 64))):
    """(textured scene, constant scene, images): every non-emitter material is an Image of a uniform colour c != its albedo in the
    first, Constant with albedo c in the second"""
    rng = np.random.default_rng(seed)
    a, b = host.HostScene(kind, mesh), host.HostScene(kind, mesh)
    imgs = []
    for i in range(a.view.n_material):
        ma, mb = a.view.materials[i], b.view.materials[i]
        if ma.type == abi.MAT_DIFFUSE and not light_too:
            continue
        alb = (ma.textureInfo.albedo.x, ma.textureInfo.albedo.y, ma.textureInfo.albedo.z)
        while True:
            c = tuple(float(rng.choice(COLOURS)) for _ in range(3))
            if c != alb:
                break
        h, w = sizes[len(imgs) % len(sizes)]
        imgs.append(np.broadcast_to(np.array(c, F), (h, w, 3)).copy())
        ma.textureInfo.type = abi.TEX_IMAGE
        ma.textureInfo.textureIndex = len(imgs) - 1
        if ma.type != abi.MAT_DIFFUSE:
            mb.textureInfo.type = abi.TEX_CONSTANT
            mb.textureInfo.albedo.x, mb.textureInfo.albedo.y, mb.textureInfo.albedo.z = c
    return a, b, imgs


def frame(gpu, sc, W, H, spp, integrator, seed=9, small_blocks=None, textures=None, frame0=0):
    gpu.upload_scene(sc.view)
    if textures is not None:
        gpu.upload_textures(textures)
    gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(seed); gpu.clear_accum(); gpu.reset_stats()
    gpu.render(spp=spp, integrator=integrator, small_blocks=small_blocks, frame0=frame0)
    return gpu.download_accum(), gpu.download_rng(), gpu.stats()


def assert_same(x, y):
    assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))
    assert np.array_equal(x[1], y[1])
    assert x[2].rays == y[2].rays and x[2].paths == y[2].paths and x[2].shaded == y[2].shaded


@pytest.mark.parametrize("integrator", [abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS, abi.INTEGRATOR_VOLUME])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_uniform_images_render_exactly(gpu, integrator, residence):
    mesh = host.Mesh.ball(24, 24, 1.0) if residence == "mem" else None
    kind = abi.SCENE_CORNELL_MESH if residence == "mem" else abi.SCENE_CORNELL_SPHERES
    tex, const, imgs = uniform_pair(kind, mesh, seed=integrator * 7 + len(residence))
    W, H = 96, 64
    for spp, small in ((1, None), (4, None), (16, None), (16, True)):
        a = frame(gpu, tex, W, H, spp, integrator, small_blocks=small, textures=imgs)
        b = frame(gpu, const, W, H, spp, integrator, small_blocks=small, textures=[])
        assert_same(a, b)
        # the textured frame is not the frame of the materials' own albedos
        c = frame(gpu, tex, W, H, spp, integrator, small_blocks=small, textures=[])
        assert not np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32))


def test_uniform_images_full_frame(gpu):
    tex, const, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=3)
    a = frame(gpu, tex, 1920, 1080, 4, abi.INTEGRATOR_PATH, textures=imgs)
    b = frame(gpu, const, 1920, 1080, 4, abi.INTEGRATOR_PATH, textures=[])
    assert_same(a, b)


def sppm_run(gpu, sc, textures, W=64, H=48, frames=3):
    gpu.upload_scene(sc.view); gpu.upload_textures(textures)
    gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(5); gpu.sppm_init(77); gpu.sppm_frames(frames)
    cam, pho, mark, count, _ = gpu.sppm_download()
    return gpu.download_accum(), gpu.download_rng(), cam, pho


def test_uniform_images_sppm(gpu):
    tex, const, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=11)
    a = sppm_run(gpu, tex, imgs)
    b = sppm_run(gpu, const, [])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    gpu.upload_textures([])


def test_index_rules_and_order(gpu):
    W, H, spp = 64, 48, 8
    base = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    plain = frame(gpu, base, W, H, spp, abi.INTEGRATOR_MIS, textures=[])          # nothing uploaded
    rng = np.random.default_rng(4)
    imgs = [rng.random((8, 8, 3), dtype=F) for _ in range(2)]
    # Image materials whose index is not below n resolve to their albedo: the frame of the plain scene
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    for i in range(sc.view.n_material):
        if sc.view.materials[i].type != abi.MAT_DIFFUSE and sc.view.materials[i].textureInfo.type == abi.TEX_CONSTANT:
            sc.view.materials[i].textureInfo.type = abi.TEX_IMAGE
            sc.view.materials[i].textureInfo.textureIndex = 2 + i
    assert_same(frame(gpu, sc, W, H, spp, abi.INTEGRATOR_MIS, textures=imgs), plain)
    assert_same(frame(gpu, sc, W, H, spp, abi.INTEGRATOR_MIS, textures=[]), plain)
    # ... and without any upload on a fresh context
    with Tracer(0) as fresh:
        assert_same(frame(fresh, sc, W, H, spp, abi.INTEGRATOR_MIS), plain)
    # a texture on the light material changes nothing (Le = albedo)
    lit = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    for i in range(lit.view.n_material):
        if lit.view.materials[i].type == abi.MAT_DIFFUSE:
            lit.view.materials[i].textureInfo.type = abi.TEX_IMAGE
            lit.view.materials[i].textureInfo.textureIndex = 0
    assert_same(frame(gpu, lit, W, H, spp, abi.INTEGRATOR_MIS, textures=imgs), plain)
    # upload order: textures before or after the scene, and surviving a re-upload of the scene
    tex, _, timgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=8)
    first = frame(gpu, tex, W, H, spp, abi.INTEGRATOR_PATH, textures=timgs)
    gpu.upload_textures([]); gpu.upload_textures(timgs)
    second = frame(gpu, tex, W, H, spp, abi.INTEGRATOR_PATH)                     # scene uploaded after the textures
    assert_same(first, second)
    with Tracer(0) as t2:
        t2.upload_textures(timgs)
        assert_same(frame(t2, tex, W, H, spp, abi.INTEGRATOR_PATH), first)
    gpu.upload_textures([])


def test_error_codes(gpu):
    tex, _, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=2)
    gpu.upload_scene(tex.view); gpu.set_camera(host.prepare_camera(32, 32)); gpu.resize(32, 32); gpu.seed(1)
    bad = [np.zeros((0, 4, 3), F), np.full((2, 2, 3), np.nan, F), np.full((2, 2, 3), np.inf, F)]
    for b in bad:
        with pytest.raises(TracerError) as e:
            gpu.upload_textures([b])
        assert e.value.status == abi.ERR_INVALID_ARG
    gpu.upload_textures(imgs)
    for kw in (dict(sobol=True), dict(collect_stats=True)):
        with pytest.raises(TracerError) as e:
            gpu.render(spp=1, **kw)
        assert e.value.status == abi.ERR_UNSUPPORTED
    gpu.render(spp=1)                              # the production kernels run
    gpu.upload_textures([])
    gpu.render(spp=1, sobol=True)                  # no active image: Sobol' is back
    gpu.render(spp=1, collect_stats=True)


def gbuffer(gpu, sc, textures, W=80, H=60):
    gpu.upload_scene(sc.view); gpu.upload_textures(textures)
    gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.seed(3); gpu.clear_accum(); gpu.render(spp=2)
    gpu.denoise()
    return gpu.download_gbuffer()


@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_gbuffer_albedo(gpu, kind):
    mesh = host.Mesh.ball(16, 16, 1.0) if kind == "mesh" else None
    k = abi.SCENE_CORNELL_MESH if mesh else abi.SCENE_CORNELL_SPHERES
    tex, const, imgs = uniform_pair(k, mesh, seed=21)
    a = gbuffer(gpu, tex, imgs)
    b = gbuffer(gpu, const, [])
    assert a.tobytes() == b.tobytes()
    # other textures: the next trc_denoise rebuilds the albedo plane
    gpu.upload_scene(tex.view)
    gpu.upload_textures([im * F(0.5) for im in imgs])
    gpu.denoise()
    c = gpu.download_gbuffer()
    moved = (a["id"] != 0xFFFFFFFF) & ~np.all(a["albedo"] == 1, axis=-1)         # textured hits (misses and emitters hold 1)
    assert moved.any()
    assert np.array_equal(c["albedo"][moved], a["albedo"][moved] * F(0.5))
    gpu.upload_textures([])


def test_fast_math_build(gpu):
    """the fast-math build runs the texture kernels too; its arithmetic is not the exact build's (contraction, flushed denormals), so
    the comparison is statistical: frame means within 3 % of the exact build's, and of the fast-math constant-colour scene's"""
    tex, const, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=5)
    with Tracer(0, fast_math=True) as fm:
        a = frame(fm, tex, 96, 64, 64, abi.INTEGRATOR_MIS, textures=imgs)[0][..., :3]
        b = frame(fm, const, 96, 64, 64, abi.INTEGRATOR_MIS, textures=[])[0][..., :3]
    exact = frame(gpu, tex, 96, 64, 64, abi.INTEGRATOR_MIS, textures=imgs)[0][..., :3]
    assert np.isfinite(a).all()
    m = float(exact.mean())
    assert m > 0
    assert abs(float(a.mean()) - m) < 0.03 * m and abs(float(a.mean()) - float(b.mean())) < 0.03 * m
    gpu.upload_textures([])


def test_structured_texture_changes_the_frame(gpu):
    """a two-colour image on every non-emitter material: finite, and between the frames of its two uniform colours"""
    W, H, spp = 64, 48, 64
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    for i in range(sc.view.n_material):
        if sc.view.materials[i].type != abi.MAT_DIFFUSE:
            sc.view.materials[i].textureInfo.type = abi.TEX_IMAGE
            sc.view.materials[i].textureInfo.textureIndex = 0
    half = np.zeros((16, 16, 3), F); half[:, :8] = F(0.25); half[:, 8:] = F(0.75)
    mid = frame(gpu, sc, W, H, spp, abi.INTEGRATOR_PATH, textures=[half])[0][..., :3].mean()
    lo = frame(gpu, sc, W, H, spp, abi.INTEGRATOR_PATH, textures=[np.full((1, 1, 3), 0.25, F)])[0][..., :3].mean()
    hi = frame(gpu, sc, W, H, spp, abi.INTEGRATOR_PATH, textures=[np.full((1, 1, 3), 0.75, F)])[0][..., :3].mean()
    assert np.isfinite(mid) and lo < mid < hi
    gpu.upload_textures([])


def _rays(cam, W, H):
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import camera_rays
    return camera_rays(cam, W, H)


def random_textures(sc, rng, sizes=((13, 7), (64, 64), (1, 9), (32, 5))):
    """a random (non-uniform) image on every non-emitter material -> images"""
    imgs = []
    for i in range(sc.view.n_material):
        m = sc.view.materials[i]
        if m.type == abi.MAT_DIFFUSE:
            continue
        h, w = sizes[len(imgs) % len(sizes)]
        imgs.append(rng.random((h, w, 3), dtype=F))
        m.textureInfo.type = abi.TEX_IMAGE
        m.textureInfo.textureIndex = len(imgs) - 1
    return imgs


def test_gbuffer_albedo_at_hit_uv(gpu):
    """with random images on every non-emitter material, the G-buffer's albedo plane equals the stated lookup at the eager hit
    records' uv (trc_trace_rays: spheres' and squares' uv derived from the hit, cubes' and triangles' from the record), bit for bit"""
    W, H = 160, 120
    types = set()
    for kind, mesh in ((abi.SCENE_CORNELL_SPHERES, None), (abi.SCENE_CORNELL_MESH, host.Mesh.golden("coatball"))):
        sc = host.HostScene(kind, mesh)
        imgs = random_textures(sc, np.random.default_rng(kind))
        cam = host.prepare_camera(W, H)
        gpu.upload_scene(sc.view); gpu.upload_textures(imgs)
        gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H); gpu.seed(1)
        gpu.denoise()
        g = gpu.download_gbuffer().ravel()
        rays = _rays(cam, W, H)
        prod = gpu.trace_rays(rays, production=True)
        eager = gpu.trace_rays(rays)
        hit = prod["hit"] != 0
        assert np.array_equal(g["depth"][hit].view(np.uint32), prod["t"][hit].view(np.uint32))
        same = hit & (eager["hit"] != 0) & (eager["pType"] == prod["pType"]) & (eager["pIndex"] == prod["pIndex"])
        assert same.sum() > 0.99 * hit.sum()
        mats = [sc.view.materials[i] for i in range(sc.view.n_material)]
        textured = same & np.array([mats[int(m)].type != abi.MAT_DIFFUSE for m in eager["material"]])
        exp = np.empty((textured.sum(), 3), F)
        idx = np.nonzero(textured)[0]
        tex_of = np.array([mats[int(m)].textureInfo.textureIndex for m in eager["material"][idx]])
        for k, img in enumerate(imgs):
            sel = tex_of == k
            exp[sel] = ref_sample(img, eager["uv"][idx[sel]])
        got = g["albedo"][idx]
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
        types |= set(np.unique(eager["pType"][textured]).tolist())
        # emitters keep 1
        light = same & ~textured
        assert np.all(g["albedo"][light] == 1.0)
    assert len(types) == 4, types              # spheres, squares, cubes and triangles all sampled
    gpu.upload_textures([])


def test_quadrant_texture_lands_where_its_uv_says(gpu):
    """region by region: an image of four grey quadrants on the white walls' material renders, on the pixels whose primary hit
    lies in a quadrant (2 texels away from the seams), like the frame whose image is that quadrant's grey everywhere"""
    W, H, spp = 96, 72, 128
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    cam = host.prepare_camera(W, H)
    gpu.upload_scene(sc.view)
    rays = _rays(cam, W, H)
    eager = gpu.trace_rays(rays)
    sq = (eager["hit"] != 0) & (eager["pType"] == np.bincount(eager["pType"][eager["hit"] != 0]).argmax())
    counts = np.bincount(eager["material"][sq])
    wall = int(counts.argmax())                                    # the material most primary hits land on (the white walls)
    assert sc.view.materials[wall].type != abi.MAT_DIFFUSE
    sc.view.materials[wall].textureInfo.type = abi.TEX_IMAGE
    sc.view.materials[wall].textureInfo.textureIndex = 0
    greys = {(0, 0): 0.125, (1, 0): 0.375, (0, 1): 0.625, (1, 1): 0.875}     # (u half, v half)
    n = 16
    img = np.zeros((n, n, 3), F)
    for (qu, qv), c in greys.items():
        img[qv * 8:(qv + 1) * 8, qu * 8:(qu + 1) * 8] = c                   # row = v (bottom-up), column = u
    uv = eager["uv"]
    on = sq & (eager["material"] == wall)
    margin = 2.0 / n
    regions = {}
    for (qu, qv) in greys:
        ur = (uv[:, 0] < 0.5 - margin) if qu == 0 else (uv[:, 0] > 0.5 + margin)
        vr = (uv[:, 1] < 0.5 - margin) if qv == 0 else (uv[:, 1] > 0.5 + margin)
        regions[(qu, qv)] = on & ur & vr & (uv[:, 0] > margin) & (uv[:, 0] < 1 - margin) & (uv[:, 1] > margin) & (uv[:, 1] < 1 - margin)
    assert all(r.sum() >= 20 for r in regions.values()), {k: int(r.sum()) for k, r in regions.items()}

    def lum(textures, seed=9):
        acc = frame(gpu, sc, W, H, spp, abi.INTEGRATOR_PATH, seed=seed, textures=textures)[0][..., :3].reshape(-1, 3)
        return acc.mean(axis=1)
    textured = lum([img])
    uniform = {c: lum([np.full((1, 1, 3), c, F)]) for c in greys.values()}
    for q, r in regions.items():
        m = float(textured[r].mean())
        dist = {c: abs(m - float(u[r].mean())) for c, u in uniform.items()}
        best = min(dist, key=dist.get)
        assert best == greys[q], (q, m, {c: float(u[r].mean()) for c, u in uniform.items()})
        # and nearer to that frame than half the step to the next grey (the quadrants' indirect light mixes, so not closer)
        others = sorted(abs(float(uniform[greys[q]][r].mean()) - float(uniform[c][r].mean())) for c in greys.values() if c != greys[q])
        assert dist[best] < 0.5 * others[0]
    gpu.upload_textures([])


def test_inactive_image_material_inside_a_textured_launch(gpu):
    """an Image material whose index is not below n, in a launch where another material's image is active (the _tex kernels),
    keeps its albedo: the frame equals the scene with that material Constant and the active one Constant c"""
    W, H, spp = 64, 48, 8
    tex, const, imgs = uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=31)
    # the last textured material gets an index past the images: it must resolve to its own albedo
    last = max(i for i in range(tex.view.n_material) if tex.view.materials[i].textureInfo.type == abi.TEX_IMAGE
               and tex.view.materials[i].type != abi.MAT_DIFFUSE)
    tex.view.materials[last].textureInfo.textureIndex = 1000
    m = host.HostScene(abi.SCENE_CORNELL_SPHERES).view.materials[last]
    const.view.materials[last].textureInfo.type = abi.TEX_CONSTANT if m.textureInfo.type == abi.TEX_IMAGE else m.textureInfo.type
    const.view.materials[last].textureInfo.albedo.x = m.textureInfo.albedo.x
    const.view.materials[last].textureInfo.albedo.y = m.textureInfo.albedo.y
    const.view.materials[last].textureInfo.albedo.z = m.textureInfo.albedo.z
    for integ in (abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS):
        a = frame(gpu, tex, W, H, spp, integ, textures=imgs)
        b = frame(gpu, const, W, H, spp, integ, textures=[])
        assert_same(a, b)
    gpu.upload_textures([])


def _write_ball_obj(path, n=24):
    """a UV sphere with vt, for the example host"""
    lines = []
    for i in range(n + 1):
        th = np.pi * i / n
        for j in range(n + 1):
            ph = 2 * np.pi * j / n
            lines.append(f"v {np.sin(th) * np.cos(ph):.6f} {np.cos(th):.6f} {np.sin(th) * np.sin(ph):.6f}")
            lines.append(f"vt {j / n:.6f} {1 - i / n:.6f}")
    for i in range(n):
        for j in range(n):
            a, b = i * (n + 1) + j + 1, i * (n + 1) + j + 2
            c, d = a + n + 1, b + n + 1
            lines.append(f"f {a}/{a} {c}/{c} {b}/{b}")
            lines.append(f"f {b}/{b} {c}/{c} {d}/{d}")
    path.write_text("\n".join(lines) + "\n")


def test_example_host_albedo_map(tmp_path):
    """examples/trc_render --albedo-map: trc_host_load_png -> trc_upload_textures -> material 19 as Image 0, C ABI only"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "trc_render")
    obj, png = tmp_path / "ball.obj", tmp_path / "tex.png"
    _write_ball_obj(obj)
    rng = np.random.default_rng(12)
    tex = np.zeros((32, 32, 4), np.uint8)
    tex[..., :3] = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    tex[:, :16, 0] = 255; tex[:, 16:, 1] = 255; tex[..., 3] = 255
    host.write_png(str(png), tex)
    outs = {}
    for name, extra in (("plain", []), ("tex", ["--albedo-map", str(png)])):
        out = tmp_path / f"{name}.png"
        r = subprocess.run([exe, "--mesh", str(obj), "--size", "96", "64", "--spp", "8", "--out", str(out), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[name] = host.load_png(out)
    assert outs["plain"].shape == outs["tex"].shape
    assert not np.array_equal(outs["plain"], outs["tex"])
    # without a mesh there is no material 19 to texture
    r = subprocess.run([exe, "--albedo-map", str(png), "--size", "32", "32", "--spp", "1", "--out", str(tmp_path / "x.png")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
