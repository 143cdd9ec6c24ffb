"""TRC_FLAG_ENV_LIGHT on the GPU (tracer_abi.h): the sampling tables and the kernels' sampler / pdf bit for bit against the CPU
restatement (tests/envlight_ref), the sample distribution, the refused combinations, a black map with the flag = the flag-off
frame bit for bit, bit-exact invariances of the new kernels (fused samples, launch order, block sizes, tiles) and, with square
lights, the same expectation as without the flag.  The Tracer is shared by the session: every test clears the map it set."""
import os
import sys

import numpy as np
import pytest

from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envlight_ref"))
import envlight_loader as el  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ref():
    return el.build()


@pytest.fixture(scope="module")
def hooks_gpu():
    t = Tracer(0, hooks=True)
    yield t
    t.close()


def test_tables_and_sampler_match_restatement(hooks_gpu, ref):
    rng = np.random.default_rng(11)
    maps = [el.sun_sky(256, 128), rng.random((33, 70, 3), dtype=F) * F(2), np.full((1, 1, 3), 3.0, F), rng.random((1, 9, 3), dtype=F),
            rng.random((7, 1, 3), dtype=F)]
    maps[1][5:9] = 0
    maps[1][20, 30, 1] = np.nan
    try:
        for k, m in enumerate(maps):
            hooks_gpu.set_environment_map(m)
            g = hooks_gpu.env_tables()
            c = ref.tables(m)
            assert np.array_equal(g["weight"].view(np.uint32), c["weight"].view(np.uint32)), k
            assert np.array_equal(g["rows"], c["rows"]), k
            assert np.array_equal(g["marg"], c["marg"]), k
            assert g["total"] == c["total"], k
            n = 10 ** 6 if k == 0 else 10 ** 5
            d = rng.integers(0, 2 ** 32, size=(n, 6), dtype=np.uint64).astype(np.uint32)
            d[:, 4:] = rng.random((n, 2), dtype=F).view(np.uint32)
            edge_i = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint32)
            edge_f = np.array([0.0, 2.0 ** -32, 1 - 2.0 ** -24, 1.0], F).view(np.uint32)
            grid = np.array(np.meshgrid(edge_i, edge_i, edge_i, edge_i, edge_f, edge_f)).reshape(6, -1).T.astype(np.uint32)
            d = np.concatenate([d, grid])
            dirs = np.concatenate([rng.normal(size=(n, 3)).astype(F),
                                   np.array([[0, 1, 0], [0, -1, 0], [-1, 0, 0], [-1, 0, -0.0], [-1, 0, 0.0], [-2, 0, 1e-30], [-2, 0, -1e-30],
                                             [np.nan, 0, 1], [1, 0, 0], [0, 0, 0], [1e-30, 1, 0], [np.inf, 1, 0]], F)])
            got, gpdf = hooks_gpu.env_light_test(d, dirs)
            exp, epdf = ref.sample(c, d), ref.pdf(c, dirs)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), k
            assert np.array_equal(gpdf.view(np.uint32), epdf.view(np.uint32)), k
    finally:
        hooks_gpu.set_environment_map(None)


def test_sample_distribution(hooks_gpu):
    """chi-square of the cell histogram of sampled directions (cells recovered from the sampler's own (u, w)) against the table"""
    m = el.sun_sky(64, 32, sun_radius=0.15, sun_power=50.0)
    try:
        hooks_gpu.set_environment_map(m)
        t = hooks_gpu.env_tables()
        n = 4 * 10 ** 6
        rng = np.random.default_rng(2)
        d = rng.integers(0, 2 ** 32, size=(n, 6), dtype=np.uint64).astype(np.uint32)
        d[:, 4:] = np.full((n, 2), 0.5, F).view(np.uint32)                 # cell centres: the cell is unambiguous
        out, _ = hooks_gpu.env_light_test(d)
    finally:
        hooks_gpu.set_environment_map(None)
    H, W = t["weight"].shape
    v = out[:, :3].astype(np.float64)
    u = np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5
    w = np.arcsin(np.clip(v[:, 1], -1, 1)) / np.pi + 0.5
    i = np.clip(np.floor(u * W), 0, W - 1).astype(np.int64)
    j = np.clip(np.floor(w * H), 0, H - 1).astype(np.int64)
    hist = np.bincount(j * W + i, minlength=W * H).astype(np.float64)
    p = t["weight"].astype(np.float64).ravel() / t["weight"].astype(np.float64).sum()
    assert hist[p == 0].sum() == 0
    e = p * n
    keep = e > 5
    chi2 = ((hist[keep] - e[keep]) ** 2 / e[keep]).sum()
    dof = keep.sum() - 1
    # chi-square with dof ~ 2000: mean dof, sd sqrt(2 dof); 6 sd
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


def env_scene(gpu, sc, W, H, env, seed=9):
    gpu.upload_scene(sc.view)
    gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.set_environment_map(env)
    gpu.seed(seed); gpu.clear_accum(); gpu.reset_stats()


def run(gpu, spp, calls=1, **kw):
    for c in range(calls):
        gpu.render(spp=spp, integrator=abi.INTEGRATOR_MIS, frame0=c * spp, **kw)
    return gpu.download_accum(), gpu.download_rng(), gpu.stats()


def same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])


def test_refused_combinations(gpu):
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    env = el.sun_sky(32, 16)
    try:
        env_scene(gpu, sc, 32, 32, env)
        gpu.render(spp=8, integrator=abi.INTEGRATOR_MIS)
        before = gpu.download_accum(), gpu.download_rng()
        for kw in (dict(integrator=abi.INTEGRATOR_PATH), dict(integrator=abi.INTEGRATOR_VOLUME), dict(integrator=abi.INTEGRATOR_MIS, sobol=True),
                   dict(integrator=abi.INTEGRATOR_MIS, collect_stats=True)):
            with pytest.raises(TracerError) as e:
                gpu.render(spp=8, env_light=True, **kw)
            assert e.value.status == abi.ERR_UNSUPPORTED, kw
        gpu.set_environment_map(None)                              # the constant environment is not sampled
        with pytest.raises(TracerError) as e:
            gpu.render(spp=8, integrator=abi.INTEGRATOR_MIS, env_light=True)
        assert e.value.status == abi.ERR_UNSUPPORTED
        after = gpu.download_accum(), gpu.download_rng()
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    finally:
        gpu.set_environment_map(None)


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_black_map_equals_flag_off(gpu, residence):
    """p_env = 0: every draw and operation of the flag-off kernel (one-wavefront workgroups and on the mesh scene persistent
    workgroups; a 96 x 64 frame is too small for a strip launch at any spp: tests/test_gpu_light_oracle.py forces those)"""
    mesh = host.Mesh.ball(24, 24, 1.0) if residence == "mem" else None
    sc = host.HostScene(abi.SCENE_CORNELL_MESH if residence == "mem" else abi.SCENE_CORNELL_SPHERES, mesh)
    black = np.zeros((16, 32, 3), F)
    try:
        for spp in (1, 4, 16, 64):
            env_scene(gpu, sc, 96, 64, black)
            a = run(gpu, spp)
            env_scene(gpu, sc, 96, 64, black)
            b = run(gpu, spp, env_light=True)
            same(a, b)
            assert a[2].rays == b[2].rays and a[2].shaded == b[2].shaded
    finally:
        gpu.set_environment_map(None)


def test_black_map_with_uniform_texture(gpu):
    """... and with an active image texture (k_render*_env<.., TEX>) against the Constant material, as test_gpu_textures.py does"""
    tex, const = host.HostScene(abi.SCENE_CORNELL_SPHERES), host.HostScene(abi.SCENE_CORNELL_SPHERES)
    imgs = []
    for i in range(tex.view.n_material):
        ma, mb = tex.view.materials[i], const.view.materials[i]
        if ma.type == abi.MAT_DIFFUSE:
            continue
        c = (0.5, 0.25, 0.125)
        imgs.append(np.broadcast_to(np.array(c, F), (3, 5, 3)).copy())
        ma.textureInfo.type = abi.TEX_IMAGE
        ma.textureInfo.textureIndex = len(imgs) - 1
        mb.textureInfo.type = abi.TEX_CONSTANT
        mb.textureInfo.albedo.x, mb.textureInfo.albedo.y, mb.textureInfo.albedo.z = c
    black = np.zeros((8, 16, 3), F)
    try:
        for spp in (2, 16):
            env_scene(gpu, tex, 64, 64, black); gpu.upload_textures(imgs)
            a = run(gpu, spp, env_light=True)
            env_scene(gpu, const, 64, 64, black); gpu.upload_textures([])
            b = run(gpu, spp)
            same(a, b)
    finally:
        gpu.upload_textures([])
        gpu.set_environment_map(None)


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_invariances_with_a_map(gpu, residence):
    mesh = host.Mesh.ball(24, 24, 1.0) if residence == "mem" else None
    sc = host.HostScene(abi.SCENE_CORNELL_MESH if residence == "mem" else abi.SCENE_CORNELL_SPHERES, mesh)
    env = el.sun_sky(128, 64, sun_power=200.0)
    W, H = 96, 64
    try:
        env_scene(gpu, sc, W, H, env)
        fused = run(gpu, 16, env_light=True)
        env_scene(gpu, sc, W, H, env)
        calls = run(gpu, 1, calls=16, env_light=True)
        same(fused, calls)
        for kw in (dict(fixed_order=True), dict(small_blocks=True), dict(small_blocks=False)):
            env_scene(gpu, sc, W, H, env)
            same(fused, run(gpu, 16, env_light=True, **kw))
        # tiles of one context sum to the whole frame
        for n in (2, 3):
            env_scene(gpu, sc, W, H, env)
            for r in range(n):
                gpu.render(spp=16, integrator=abi.INTEGRATOR_MIS, tile_rank=r, tile_nranks=n, env_light=True)
            same(fused, (gpu.download_accum(), gpu.download_rng()))
        # the map lights the frame: not the flag-off frame
        env_scene(gpu, sc, W, H, env)
        off = run(gpu, 16)
        assert not np.array_equal(off[0].view(np.uint32), fused[0].view(np.uint32))
    finally:
        gpu.set_environment_map(None)


def test_unbiased_with_square_lights(gpu):
    """Cornell scene + a moderate map: per-region means of K seeds with and without the flag agree (two-sample z-test, |z| < 5
    in every one of 16 regions x 3 channels: a false alarm per run has probability ~3e-5)."""
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    env = el.sun_sky(64, 32, sun_radius=0.2, sun_power=20.0)
    W, H, K, spp = 64, 64, 12, 64
    means = {False: [], True: []}
    try:
        for flag in (False, True):
            for k in range(K):
                env_scene(gpu, sc, W, H, env, seed=100 + k)
                a = run(gpu, spp, env_light=flag)[0][..., :3].astype(np.float64)
                means[flag].append(a.reshape(4, H // 4, 4, W // 4, 3).mean(axis=(1, 3)))
    finally:
        gpu.set_environment_map(None)
    off, on = np.array(means[False]), np.array(means[True])
    se = np.sqrt(off.var(axis=0, ddof=1) / K + on.var(axis=0, ddof=1) / K)
    z = (on.mean(axis=0) - off.mean(axis=0)) / np.maximum(se, 1e-12)
    assert np.all(np.abs(z) < 5), z
    assert (off.mean() > 0) and (on.mean() > 0)


# ---------------------------------------------------------------- environment-only scene: the new capability
FLOOR_PBRT = '''LookAt 0 5 0  0 0 0  0 0 1
Camera "perspective" "float fov" [ 40 ]
Film "image" "integer xresolution" [ 64 ] "integer yresolution" [ 64 ]
WorldBegin
Material "matte" "rgb Kd" [ 0.3 0.3 0.3 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -4 0 -4  0 0 -4  0 0 4  -4 0 4 ]
Material "matte" "rgb Kd" [ 0.7 0.7 0.7 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 0 0 -4  4 0 -4  4 0 4  0 0 4 ]
WorldEnd
'''


def lookup64(img, d):
    """the kernels' env_radiance in float64: SampleSphericalMap's constants (Render.hh:42-48) + the bilinear, clamp-to-edge lookup"""
    h, w = img.shape[:2]
    u = np.arctan2(d[:, 2], d[:, 0]) * 0.1591 + 0.5
    v = np.arcsin(np.clip(d[:, 1], -1, 1)) * 0.3183 + 0.5
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xi = lambda a: np.clip(a, 0, w - 1).astype(np.int64)
    yi = lambda a: np.clip(a, 0, h - 1).astype(np.int64)
    im = img.astype(np.float64)
    top = (1 - fx) * im[yi(y0), xi(x0)] + fx * im[yi(y0), xi(x0 + 1)]
    bot = (1 - fx) * im[yi(y0 + 1), xi(x0)] + fx * im[yi(y0 + 1), xi(x0 + 1)]
    return (1 - fy) * top + fy * bot


def irradiance_integral(img, n_phi=4096, n_lat=1024):
    """E = integral over the upper hemisphere of L(w) cos(theta) / pi d(omega), midpoint rule in (phi, latitude), float64"""
    phi = 2 * np.pi * ((np.arange(n_phi) + 0.5) / n_phi - 0.5)
    lat = (np.pi / 2) * ((np.arange(n_lat) + 0.5) / n_lat)
    P, La = np.meshgrid(phi, lat)
    d = np.stack([np.cos(La) * np.cos(P), np.sin(La), np.cos(La) * np.sin(P)], -1).reshape(-1, 3)
    L = lookup64(img, d)
    wgt = (np.sin(La) * np.cos(La)).reshape(-1, 1) / np.pi * (2 * np.pi / n_phi) * (np.pi / 2 / n_lat)
    return (L * wgt).sum(axis=0)


def test_environment_only_scene(gpu, tmp_path):
    """Two Lambert squares (albedo 0.3 and 0.7, side by side on the floor, nothing else) under a sun-and-sky map, seen from above: every
    pixel of a square has the expectation albedo * E (E = the float64 integral above; one bounce, nothing occludes the sky).  traceMIS
    + the flag -- refused without it, the scene has no square light -- matches it and tracePath, at an equal-spp MSE far below tracePath's."""
    p = tmp_path / "floor.pbrt"
    p.write_text(FLOOR_PBRT)
    scene, cam, info, _ = host.HostScene.from_pbrt(str(p))
    assert scene.view.n_square < 7
    env = el.sun_sky(256, 128, sun=(0.3, 0.7), sun_radius=0.05, sun_power=2000.0)
    W, H, spp = info.xres, info.yres, 64
    E = irradiance_integral(env)
    frames = {}
    try:
        gpu.upload_scene(scene.view); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
        gpu.set_environment_map(env)
        with pytest.raises(TracerError) as e:
            gpu.render(spp=1, integrator=abi.INTEGRATOR_MIS)
        assert e.value.status == abi.ERR_INVALID_ARG
        for name, kw in (("mis", dict(integrator=abi.INTEGRATOR_MIS, env_light=True)), ("path", dict(integrator=abi.INTEGRATOR_PATH))):
            gpu.seed(21); gpu.clear_accum()
            gpu.render(spp=spp, **kw)
            frames[name] = gpu.download_accum()[..., :3].astype(np.float64)
    finally:
        gpu.set_environment_map(None)
    # the two halves of the frame (the squares meet in the middle column); 3 columns either side of it left out
    halves = [frames["mis"][:, : W // 2 - 3], frames["mis"][:, W // 2 + 3:]]
    order = np.argsort([h.mean() for h in halves])
    cols = [slice(0, W // 2 - 3), slice(W // 2 + 3, W)]
    mse = {}
    for name, f in frames.items():
        err2 = []
        for k, albedo in zip(order, (0.3, 0.7)):
            px = f[:, cols[k]].reshape(-1, 3)
            ref = albedo * E
            se = px.std(axis=0, ddof=1) / np.sqrt(px.shape[0])
            assert np.all(np.abs(px.mean(axis=0) - ref) < 5 * se + 2e-3 * ref), (name, albedo, px.mean(axis=0), ref, se)
            err2.append(((px - ref) ** 2).mean())
        mse[name] = float(np.mean(err2))
    print(f"equal-spp ({spp}) MSE: tracePath {mse['path']:.5g}, traceMIS + TRC_FLAG_ENV_LIGHT {mse['mis']:.5g}, "
          f"gain {mse['path'] / mse['mis']:.1f}x")
    assert mse["mis"] * 4 <= mse["path"], mse


def write_hdr(path, img):
    """flat (uncompressed) Radiance RGBE, rows top-down in the file (-Y): img rows are bottom-up like trc_host_load_hdr's result"""
    top_down = img[::-1]
    m = top_down.max(axis=2)
    mant, expo = np.frexp(m)
    ok = m > 1e-32
    scale = np.where(ok, mant * 256.0 / np.where(ok, m, 1), 0)
    rgbe = np.zeros(top_down.shape[:2] + (4,), np.uint8)
    rgbe[..., :3] = np.clip(top_down * scale[..., None], 0, 255).astype(np.uint8)
    rgbe[..., 3] = np.where(ok, expo + 128, 0).astype(np.uint8)
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + rgbe.tobytes())


def test_example_host_env_light(tmp_path):
    """examples/trc_render --pbrt (no area light) --hdr --env-light --integrator mis writes a lit frame; without --env-light it refuses"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "trc_render")
    scene, hdr, out = tmp_path / "floor.pbrt", tmp_path / "sky.hdr", tmp_path / "frame.png"
    scene.write_text(FLOOR_PBRT)
    write_hdr(str(hdr), el.sun_sky(64, 32, sun_radius=0.1, sun_power=50.0))
    r = subprocess.run([exe, "--pbrt", str(scene), "--hdr", str(hdr), "--env-light", "--integrator", "mis", "--spp", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = host.load_png(str(out))
    assert img.shape[0] == 64 and img.shape[1] == 64 and img[..., :3].max() > 0
    r = subprocess.run([exe, "--pbrt", str(scene), "--hdr", str(hdr), "--integrator", "mis", "--spp", "8", "--out", str(tmp_path / "x.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
