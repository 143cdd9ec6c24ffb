"""libtracer_amd_fast.so: the same sources under fast-math rules (approximate division / sqrt, FMA contraction,
denormals flushed), as the reference compiles its own shaders (MTL_FAST_MATH).  It is NOT the parity build: path tracing
is chaotic, so its frames are compared with the exact build's the way two exact renders with different seeds compare --
statistically -- and its first hits must be the exact build's (north_star: bit-exact hit indices, a float tolerance on
radiance)."""
import numpy as np
import pytest

import fast_ref as fr
from conftest import camera_rays
from tracer_amd import abi, device, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fast():
    t = device.Tracer(0, fast_math=True)
    yield t
    t.close()


def test_flavours(gpu, fast):
    assert device.lib().trc_build_flavor() == b"exact" and device.lib(fast_math=True).trc_build_flavor() == b"fast-math"


@pytest.mark.parametrize("scene_name", ["cornell_spheres", "coatball"])
def test_first_hits_are_the_exact_builds(gpu, fast, request, scene_name):
    scene = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("coatball")) if scene_name == "coatball" else request.getfixturevalue(scene_name)
    W, H = 960, 540
    rays = camera_rays(host.prepare_camera(W, H), W, H)
    gpu.upload_scene(scene.view); fast.upload_scene(scene.view)
    a, b = gpu.trace_rays(rays, production=True), fast.trace_rays(rays, production=True)
    same = (a["hit"] == b["hit"]) & (a["pType"] == b["pType"]) & (a["pIndex"] == b["pIndex"])
    assert same.mean() > 0.9999, f"{(~same).sum()} of {len(rays)} primary rays hit something else"
    h = same & (a["hit"] != 0)
    rel = np.abs(a["t"][h] - b["t"][h]) / a["t"][h]
    # stated tolerance: t within 1e-3 relative (median < 1e-6), the hit point within 3e-4 of the distance travelled
    assert rel.max() < 1e-3 and np.median(rel) < 1e-6
    assert (np.abs(a["p"][h] - b["p"][h]).max(axis=1) <= 3e-4 * np.maximum(a["t"][h], 100.0)).all()


def test_frames_agree_like_two_exact_renders(gpu, fast, cornell_spheres):
    """the criterion is fast_ref.frames_disagree: clipped-luminance RMSE below 1.15 x the seed noise, 8 x 8 block means (far less noisy:
    they must agree much more tightly than single pixels do) below 1.2 x, mean and ray count within 1 %"""
    W, H, spp = 480, 270, 64
    cam = host.prepare_camera(W, H)

    def render(t, seed):
        t.upload_scene(cornell_spheres.view); t.set_camera(cam); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
        t.seed(seed); t.clear_accum(); t.reset_stats(); t.render(spp=spp)
        return fr.luminance(t.download_accum()), t.stats().rays
    exact_a, rays_a = render(gpu, 11)
    exact_b, _ = render(gpu, 12)
    fast_a, rays_f = render(fast, 11)
    fig = fr.frame_figures(fast_a, exact_a, exact_b)
    assert not fr.frames_disagree(fig, (rays_f, rays_a)), fig              # indistinguishable from a re-seeded exact render
