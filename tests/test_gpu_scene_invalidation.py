"""What a context forgets when its scene is replaced or edited (trc_ctx.hpp: trc_scene_changed).  Six ways lead from scene X to scene Y:
trc_upload_scene, trc_upload_scene_lbvh, trc_upload_scene_sah, trc_upload_scene_device with triangle leaves, trc_upload_triangle_materials
and trc_update_vertices.  Context A takes each of them with every cache derived from X live -- block costs and a sorted launch order, the
order of the view before a camera jump kept as the next cold pass's prior, the emissive triangles' tables, the denoiser's G-buffer and
history, per-triangle materials, the kept vertex arrays -- and context B is created fresh and goes straight to Y with the same calls.
RNG texture, accumulator and denoised frame must be the same bits: nothing of X may reach a pixel of Y.
(The launch order X leaves behind is a prior for the order of blocks only, and no pixel depends on launch order: DESIGN.md section 4.1.)

Scene: Cornell + the 1104-triangle ball of tests/test_gpu_mesh_lights.py (tree read from memory), some of its triangles the emitter.
Frame 32x32 = 16 pixel blocks, 8 samples per launch (the one-block kernels and the cold pass), depth 4, traceMIS with TRC_FLAG_MESH_LIGHTS."""
import numpy as np
import pytest

import refit_ref as rr
from test_gpu_mesh_lights import cornell_mesh, lamp_materials
from tracer_amd import abi, host
from tracer_amd.device import Tracer

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH, SEED = 32, 32, 8, 4, 9
MIS = abi.INTEGRATOR_MIS
DEVICE_TREE = abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES
PATHS = ["upload_scene", "upload_scene_lbvh", "upload_scene_sah", "upload_scene_device", "upload_triangle_materials", "update_vertices"]

_CACHE = {}


def scene_x():
    return cornell_mesh("bigball")


def n_triangles():
    return scene_x().view.n_index // 3


def lamp_x():
    return lamp_materials(n_triangles(), range(0, n_triangles(), 7))


def lamp_y():
    return lamp_materials(n_triangles(), range(3, n_triangles(), 11))


def moved_vertices():
    if "v" not in _CACHE:
        _CACHE["v"] = rr.twist(rr.vertices_of(scene_x().view), 0.7)
    return _CACHE["v"]


def scene_y(analytic_leaves_only=False):
    """X's mesh twisted and scaled (refit_ref.twist) and placed in the box afresh by the host scene: a scene of its own with a tree of its own"""
    key = ("y", analytic_leaves_only)
    if key not in _CACHE:
        mesh = host.Mesh.from_arrays(moved_vertices(), rr.indices_of(scene_x().view))
        _CACHE[key] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=analytic_leaves_only)
    return _CACHE[key]


def refitted_x():
    """X's host tree refitted to the moved vertices: what trc_update_vertices leaves of a trc_upload_scene"""
    if "refit" not in _CACHE:
        sc = scene_x()
        _CACHE["refit"] = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), moved_vertices(), rr.indices_of(sc.view)), moved_vertices())
    return _CACHE["refit"]


def arrive_at_y(t, path, fresh):
    """scene Y on context `t` by `path`; fresh: the context holds no scene yet, so the two edits start from the scene they edit"""
    if path == "upload_scene":
        t.upload_scene(scene_y().view)
    elif path == "upload_scene_lbvh":
        t.upload_scene_lbvh(scene_y().leaves_view())
    elif path == "upload_scene_sah":
        t.upload_scene_sah(scene_y().leaves_view())
    elif path == "upload_scene_device":
        t.upload_scene_device(scene_y(analytic_leaves_only=True).view, DEVICE_TREE)
    elif path == "upload_triangle_materials":
        if fresh:
            t.upload_scene(scene_x().view)
        t.upload_triangle_materials(lamp_y())
        return
    elif path == "update_vertices":
        if fresh:
            t.upload_scene(refitted_x().view); t.upload_triangle_materials(lamp_x())
        else:
            t.update_vertices(moved_vertices())                       # keeps the triangle materials
        return
    t.upload_triangle_materials(lamp_y())                             # an upload puts every triangle back to material 19


def far_camera():
    return host.make_camera((520.0, 360.0, -700.0), (278.0, 278.0, 278.0), (0.0, 1.0, 0.0), 0.0, W / H, float(np.deg2rad(45.0)), 10.0)


def render_y(t):
    """two launches (the second in the adaptive order) and the denoiser; the three planes that must not depend on the context's past"""
    t.seed(SEED); t.clear_accum(); t.reset_stats()
    for k in range(2):
        t.render(spp=SPP, max_depth=DEPTH, integrator=MIS, frame0=k * SPP, mesh_lights=True)
    t.denoise()
    return t.download_rng(), t.download_accum(), t.download_denoised()


@pytest.mark.parametrize("path", PATHS)
def test_scene_y_does_not_depend_on_scene_x_before_it(path):
    with Tracer(0) as a:
        a.upload_scene(scene_x().view); a.upload_triangle_materials(lamp_x())
        a.set_camera(far_camera()); a.set_environment((0.0, 0.0, 0.0)); a.resize(W, H)
        a.seed(SEED + 1); a.clear_accum()
        for k in range(3):                                            # cold, then ordered and planned by the launch before
            a.render(spp=SPP, max_depth=DEPTH, integrator=MIS, frame0=k * SPP, mesh_lights=True)
        a.denoise()
        x_frame = a.download_accum()
        a.set_camera(host.prepare_camera(W, H))                       # a jump: X's launch order stays as the next cold pass's prior
        arrive_at_y(a, path, fresh=False)
        got = render_y(a)
    with Tracer(0) as b:
        arrive_at_y(b, path, fresh=True)
        b.set_camera(host.prepare_camera(W, H)); b.set_environment((0.0, 0.0, 0.0)); b.resize(W, H)
        want = render_y(b)
    assert np.isfinite(want[1]).all() and (want[1][..., :3] > 0).any()
    assert not np.array_equal(x_frame.view(np.uint32), want[1].view(np.uint32))
    for name, g, w in zip(("rng", "accumulator", "denoised"), got, want):
        bad = int((g.view(np.uint32) != w.view(np.uint32)).any(axis=-1).sum())
        print(f"{path}: {name}: {bad} of {W * H} pixels differ")
        assert bad == 0, (path, name, bad)
