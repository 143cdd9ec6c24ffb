"""Frames of libtracer_amd_fast.so beyond tracePath on Cornell + spheres: every render path that was compiled into the fast flavour after
tests/test_gpu_fast_math.py was written.  Path tracing is chaotic, so a fast frame is compared with the exact build's the way two exact
renders with different seeds compare (fast_ref.frames_disagree, the criterion and thresholds of test_frames_agree_like_two_exact_renders).

Frame size and spp are chosen, not guessed (SHAPES): per scene the first of 96 x 64, 160 x 96 and 240 x 136 at 64 spp -- then at 128, 256,
... spp: the spp is doubled before any threshold would widen -- at which three FURTHER exact-build seeds pass every threshold with half
its margin (1.075, 1.10, 0.5 %) while the exact frame scaled by 1.02 fails.  controls() computes those figures; the measured values behind SHAPES are in
profiles/r29/fast_flavour.txt.  Each test asserts the scaled control again, so a criterion that could not tell 2 % would show here.

TRC_FLAG_SOBOL does not read the RNG texture, so a "seed" of the Sobol' case is a range of sample indices: frame0 = 0 for SEED_A, then
spp, 2 spp, ...  The running mean takes its weights from frame0 + s, so a cleared accumulator filled from frame0 holds the mean of those
spp samples times spp / (frame0 + spp); render() undoes that factor on the luminance."""
import os
import sys

import numpy as np
import pytest

import fast_ref as fr
from test_gpu_mesh_lights import cornell_mesh, lamp_materials
from test_gpu_textures import uniform_pair
from test_gpu_update_vertices import DEVICE_TREE, scene
from tracer_amd import abi, device, host

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envlight_ref"))
import envlight_loader as el  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
PATH, MIS, VOLUME = abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS, abi.INTEGRATOR_VOLUME
SIZES = ((96, 64), (160, 96), (240, 136))
SEED_A, SEED_B, CONTROL_SEEDS = 11, 12, (13, 14, 15)
_KEEP = {}


@pytest.fixture(scope="module")
def fast():
    t = device.Tracer(0, fast_math=True)
    yield t
    t.close()


def once(key, make):
    if key not in _KEEP:
        _KEEP[key] = make()
    return _KEEP[key]


# every scene: prepare(t) uploads it and leaves the context ready to render; kw are render()'s; restore(t) undoes what a shared context keeps
def spheres(t):
    t.upload_scene(once("spheres", lambda: host.HostScene(abi.SCENE_CORNELL_SPHERES)).view)


def bigball_lamps(t):
    sc = cornell_mesh("bigball")
    n = sc.view.n_index // 3
    t.upload_scene(sc.view)
    t.upload_triangle_materials(lamp_materials(n, range(n // 3, n // 3 + 6)))


def spheres_env(t):
    spheres(t)
    t.set_environment_map(once("env", lambda: el.sun_sky(128, 64, sun_power=200.0)))


def mem_device_tree_materials(t):
    """'mem' through a device SAH tree, every third triangle the red Lambert (material 4), the rest material 19"""
    n = scene("mem").view.n_index // 3
    t.upload_scene_device(scene("mem", analytic_leaves_only=True).view, DEVICE_TREE)
    m = np.full(n, 19, np.uint32); m[::3] = 4
    t.upload_triangle_materials(m)


def textured(t):
    tex, _, imgs = once("textured", lambda: uniform_pair(abi.SCENE_CORNELL_SPHERES, seed=5))
    t.upload_scene(tex.view)
    t.upload_textures(imgs)


def volume(t):
    cloud = once("cloud", host.make_cloud)
    t.upload_scene(once("volume", lambda: host.HostScene(abi.SCENE_CORNELL_VOLUME)).view)
    t.upload_density(host.density_info(cloud), cloud)


def restore(t, prepare):
    if prepare in (bigball_lamps, mem_device_tree_materials):
        t.upload_triangle_materials(None)
    t.set_environment_map(None); t.upload_textures([]); t.upload_density(None, None)


SCENES = {
    "mis_spheres": (spheres, dict(integrator=MIS)),
    "mis_mesh_lights_bigball": (bigball_lamps, dict(integrator=MIS, mesh_lights=True)),
    "mis_env_light": (spheres_env, dict(integrator=MIS, env_light=True)),
    "path_mem_device_tree_triangle_materials": (mem_device_tree_materials, dict(integrator=PATH)),
    "mis_textured": (textured, dict(integrator=MIS)),
    "volume_cloud": (volume, dict(integrator=VOLUME)),
    "path_sobol": (spheres, dict(integrator=PATH, sobol=True)),
}
# (width, height, spp) per scene, from controls() on an MI355X: profiles/r29/fast_flavour.txt.  At 64 spp no size carries the criterion --
# the clipped mean of three further exact seeds moves by 1 - 3 %, far beyond the half margin of 0.5 % -- so the spp was doubled until one did.
# traceMIS + mesh lights and traceVolume met the controls only at shapes whose three renders take about ten seconds; no smaller shape may
# stand in (8 x 8 block means of further exact seeds reach 1.2 - 1.5 x the seed noise below them), so those two cases cost that much.
SHAPES = {
    "mis_spheres": (240, 136, 1024),
    "mis_mesh_lights_bigball": (240, 136, 8192),
    "mis_env_light": (160, 96, 1024),
    "path_mem_device_tree_triangle_materials": (160, 96, 1024),
    "mis_textured": (240, 136, 1024),
    "volume_cloud": (160, 96, 2048),
    "path_sobol": (160, 96, 256),
}
# the cases whose five control renders take under a second: their controls are asserted again by test_shape_still_meets_the_controls;
# those of the two slow cases are recorded in profiles/r29/fast_flavour.txt only
QUICK = ("mis_env_light", "mis_spheres", "mis_textured", "path_mem_device_tree_triangle_materials", "path_sobol")


def render(t, name, W, H, spp, seed):
    """-> (luminance frame, rays)"""
    prepare, kw = SCENES[name]
    try:
        prepare(t)
        t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
        t.seed(seed); t.clear_accum(); t.reset_stats()
        frame0 = (seed - SEED_A) * spp if kw.get("sobol") else 0
        t.render(spp=spp, frame0=frame0, **kw)
        return fr.luminance(t.download_accum()) * ((frame0 + spp) / spp), t.stats().rays
    finally:
        restore(t, prepare)


def controls(gpu, name, W, H, spp):
    """the figures that decide whether (W, H, spp) can carry the criterion for this scene -> (usable, dict)"""
    a, rays_a = render(gpu, name, W, H, spp, SEED_A)
    b, _ = render(gpu, name, W, H, spp, SEED_B)
    out = dict(noise=fr.frame_figures(a, a, b)["noise"], seeds=[], scaled=None)
    usable = True
    for s in CONTROL_SEEDS:
        c, rays_c = render(gpu, name, W, H, spp, s)
        fig = fr.frame_figures(c, a, b)
        missed = fr.frames_disagree(fig, (rays_c, rays_a), margin=0.5)
        out["seeds"].append((round(fig["rmse"], 4), round(fig["blocks"], 4), round(fig["mean"], 5), missed))
        usable = usable and not missed
    fig = fr.frame_figures(a * 1.02, a, b)
    out["scaled"] = (round(fig["rmse"], 4), round(fig["blocks"], 4), round(fig["mean"], 5), fr.frames_disagree(fig))
    return usable and bool(out["scaled"][3]), out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_fast_frame_is_a_re_seeded_exact_frame(gpu, fast, name):
    W, H, spp = SHAPES[name]
    exact_a, rays_a = render(gpu, name, W, H, spp, SEED_A)
    exact_b, _ = render(gpu, name, W, H, spp, SEED_B)
    fast_a, rays_f = render(fast, name, W, H, spp, SEED_A)
    assert exact_a.mean() > 0 and not np.array_equal(exact_a, exact_b)
    fig = fr.frame_figures(fast_a, exact_a, exact_b)
    print(name, (W, H, spp), {k: round(v, 5) if isinstance(v, float) else v for k, v in fig.items()}, rays_f, rays_a)
    assert not fr.frames_disagree(fig, (rays_f, rays_a)), fig
    assert fr.frames_disagree(fr.frame_figures(exact_a * 1.02, exact_a, exact_b))          # the criterion tells a 2 % brighter frame


@pytest.mark.parametrize("name", QUICK)
def test_shape_still_meets_the_controls(gpu, name):
    """the derivation of SHAPES, checkable: three further exact seeds within half of every margin, the exact frame x 1.02 outside"""
    usable, figures = controls(gpu, name, *SHAPES[name])
    assert usable, figures
