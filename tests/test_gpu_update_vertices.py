"""trc_update_vertices on the GPU (include/tracer_abi.h): the refitted tree and the frames rendered through it against the definition
(tests/refit_ref.py) and the CPU oracle, bit for bit; what the call keeps (triangle materials, block costs) and what it drops (mesh-light
tables, the G-buffer); refusals that change nothing.  The deformation is refit_ref.twist: a twist-and-scale about the mesh's box centre."""
import os
import sys

import numpy as np
import pytest

import refit_ref as rr
from conftest import random_rays
from oracle import pyoracle
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "meshlight_ref"))

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 48, 32
PATH, MIS = abi.INTEGRATOR_PATH, abi.INTEGRATOR_MIS
DEVICE_TREE = abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES

_SCENES = {}


def scene(residence, analytic_leaves_only=False):
    """'lds': Cornell + a 48-triangle ball (the whole tree is staged in LDS); 'mem': Cornell + a 5 000-triangle ball (read from memory)"""
    key = (residence, analytic_leaves_only)
    if key not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.ball(50, 50, 0.08)
        _SCENES[key] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=analytic_leaves_only)
    return _SCENES[key]


def moved(residence, angle, scale=0.9):
    """(new vertices, the scene view over refit() of the host tree and those vertices)"""
    sc = scene(residence)
    v = rr.twist(rr.vertices_of(sc.view), angle, scale)
    return v, rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)


def frame(t, spp, integrator, seed=9, **kw):
    t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H)
    t.seed(seed); t.clear_accum(); t.reset_stats()
    t.render(spp=spp, integrator=integrator, **kw)
    return t.download_accum(), t.download_rng(), t.stats().rays


def oracle_frame(view, spp, integrator, seed=9):
    rng = host.fill_rng(seed, W, H)
    acc, st = pyoracle.render(view, host.prepare_camera(W, H), W, H, rng, spp=spp, integrator=integrator)
    return acc, rng, st.rays


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} of {len(want)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}" if len(bad) else ""


# --------------------------------------------------------------------------------------------------- tree and hit records
@pytest.mark.parametrize("tree", ["sah_triangle_leaves", "lbvh"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_downloaded_tree_is_the_refit_of_the_tree_before(gpu, residence, tree):
    sc = scene(residence)
    if tree == "lbvh":
        gpu.upload_scene_lbvh(sc.leaves_view())
    else:
        gpu.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    before = rr.raw(gpu.download_bvh())
    idx = rr.indices_of(sc.view)
    for angle in (0.5, -1.2):
        v = rr.twist(rr.vertices_of(sc.view), angle)
        gpu.update_vertices(v)
        got = rr.raw(gpu.download_bvh())
        assert not first_difference(got, rr.refit(before, v, idx)), angle
    assert (got[:, :8] == before[:, :8]).all()                       # links, axis, pType, pIndex: the topology stays


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_host_tree_walk_counts_every_box(gpu, residence):
    """the instrumented walk's counters depend on every box of the tree: they pin a tree that cannot be downloaded"""
    v, m = moved(residence, 0.8)
    gpu.upload_scene(scene(residence).view)
    gpu.update_vertices(v)
    rays = random_rays(4000, 3, inside_only=True)
    got, ref = gpu.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
    for f in ref.dtype.names:
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    assert (ref["pType"][ref["hit"] != 0] == abi.PRIM_TRIANGLE).any() and ref["n_descend"].sum() > 0


# --------------------------------------------------------------------------------------------------- frames against the oracle
@pytest.mark.parametrize("integrator", [PATH, MIS])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_frame_after_update_is_the_oracle_s(gpu, residence, integrator):
    sc = scene(residence)
    v, m = moved(residence, 0.7)
    gpu.upload_scene(sc.view)
    original = frame(gpu, 4, integrator)
    gpu.update_vertices(v)
    got = frame(gpu, 4, integrator)
    assert same(got, oracle_frame(m.view, 4, integrator))
    assert not same(got, original)
    with Tracer(0) as fresh:                                            # ... and what uploading that tree gives
        fresh.upload_scene(m.view)
        assert same(frame(fresh, 4, integrator), got)
    # two updates in a row are one update to the final positions
    v2, m2 = moved(residence, -0.4, 0.8)
    gpu.update_vertices(v2)
    twice = frame(gpu, 4, integrator)
    with Tracer(0) as fresh:
        fresh.upload_scene(sc.view)
        fresh.update_vertices(v2)
        assert same(frame(fresh, 4, integrator), twice)
    assert same(twice, oracle_frame(m2.view, 4, integrator))
    # a partial range equals the whole array with the same final vertices
    n = len(v)
    a, b = n // 3, n // 3 + n // 2
    mixed = v2.copy(); mixed[a:b] = v[a:b]
    gpu.update_vertices(v[a:b], first=a)
    part = frame(gpu, 4, integrator)
    gpu.update_vertices(mixed)
    assert same(frame(gpu, 4, integrator), part)
    mm = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), mixed, rr.indices_of(sc.view)), mixed)
    assert same(part, oracle_frame(mm.view, 4, integrator))
    # back to the first vertices: the first frame
    gpu.update_vertices(rr.vertices_of(sc.view))
    assert same(frame(gpu, 4, integrator), original)


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_device_tree_frame_after_update(gpu, residence):
    """the refit of a device-built tree renders as the upload of the downloaded records does"""
    sc = scene(residence)
    gpu.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)
    v = rr.twist(rr.vertices_of(sc.view), 1.0)
    gpu.update_vertices(v)
    got = frame(gpu, 4, PATH)
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    assert same(got, oracle_frame(m.view, 4, PATH))


# --------------------------------------------------------------------------------------------------- state carried across
def test_triangle_materials_survive(gpu):
    """material 19 copied to a new slot k and an orange Lambert put at 19: with every triangle naming k the frame is the plain scene's"""
    from test_gpu_triangle_materials import Relabelled
    sc = scene("mem")
    rel = Relabelled(sc.view)
    n = sc.view.n_index // 3
    gpu.upload_scene(rel.view(sc.view))
    gpu.upload_triangle_materials(np.full(n, rel.k, np.uint32))
    v, m = moved("mem", 0.7)
    gpu.update_vertices(v)
    assert same(frame(gpu, 4, MIS), oracle_frame(m.view, 4, MIS))
    rays = random_rays(4000, 4, inside_only=True)
    hits = gpu.trace_rays(rays)
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.sum() > 50 and (hits["material"][tri] == rel.k).all()
    gpu.upload_triangle_materials(None)


def test_mesh_light_tables_follow_the_vertices():
    import meshlight_loader as ml
    ref = ml.build()
    sc = scene("lds")
    n = sc.view.n_index // 3
    tri_mat = np.full(n, 4, np.uint32); tri_mat[n // 2:n // 2 + 6] = 3   # Cornell's table: 3 = the lamp's emitter, 4 = the red Lambert
    with Tracer(0, hooks=True) as t:
        t.upload_scene(sc.view)
        t.upload_triangle_materials(tri_mat)
        before = t.mesh_light_tables(n)
        v = rr.twist(rr.vertices_of(sc.view), 0.3, 1.4)                 # the emissive triangles grow
        t.update_vertices(v)
        g = t.mesh_light_tables(n)
        m = rr.Moved(sc.view, sc.bvh_array().copy(), v)
        c = ref.tables(ml.view_triangles(m.view), tri_mat, *ml.view_materials(m.view))
        assert g["n_lights"] == c["n_lights"] == before["n_lights"] > 0      # (a triangle of no area is no light)
        assert np.array_equal(g["tri"], c["tri"]) and np.array_equal(g["alias"], c["alias"])
        assert np.array_equal(g["pdfA"].view(np.uint32), c["pdfA"].view(np.uint32)) and g["total"] == c["total"]
        assert g["total"] > before["total"]


# --------------------------------------------------------------------------------------------------- denoiser, scheduling, arguments
def test_gbuffer_shows_the_new_depth(gpu):
    v, m = moved("lds", 0.0, 0.5)                                        # the ball shrinks to half its size
    gpu.upload_scene(scene("lds").view)
    frame(gpu, 2, PATH)
    gpu.denoise()
    before = gpu.download_gbuffer()
    gpu.update_vertices(v)
    frame(gpu, 2, PATH)
    gpu.denoise()
    after = gpu.download_gbuffer()
    with Tracer(0) as fresh:
        fresh.upload_scene(m.view)
        frame(fresh, 2, PATH)
        fresh.denoise()
        want = fresh.download_gbuffer()
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()


def test_block_costs_are_kept_and_move_no_pixel(gpu):
    v, m = moved("mem", 0.2)
    gpu.upload_scene(scene("mem").view)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    gpu.update_vertices(v)
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)  # the costs were kept ...
    ordered = frame(gpu, 16, PATH)
    gpu.update_vertices(v)
    assert same(frame(gpu, 16, PATH, fixed_order=True), ordered)        # ... and order is scheduling only
    assert same(ordered, oracle_frame(m.view, 16, PATH))


def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        with pytest.raises(TracerError) as e:
            fresh.update_vertices(np.zeros((3, 8), F))
        assert e.value.status == abi.ERR_NO_SCENE
        spheres = host.HostScene(abi.SCENE_CORNELL_SPHERES)                      # a scene without triangles
        fresh.upload_scene(spheres.view)
        fresh.update_vertices(np.zeros((0, 8), F))
        with pytest.raises(TracerError) as e:
            fresh.update_vertices(np.zeros((1, 8), F))
        assert e.value.status == abi.ERR_INVALID_ARG
    sc = scene("lds")
    gpu.upload_scene(sc.view)
    v0 = rr.vertices_of(sc.view)
    n = len(v0)
    before = frame(gpu, 4, MIS)
    nan, inf, far = v0.copy(), v0.copy(), v0.copy()
    nan[n // 2, 1] = np.nan; inf[0, 0] = -np.inf; far[n - 1, 2] = 2e37
    for arr, first in ((v0, 1), (v0[:2], n - 1), (v0[:1], n), (v0[:1], 0xFFFFFFFF), (nan, 0), (inf, 0), (far, 0)):
        with pytest.raises(TracerError) as e:
            gpu.update_vertices(arr * F(0.5) if arr is v0 else arr, first=first)
        assert e.value.status == abi.ERR_INVALID_ARG
        assert same(frame(gpu, 4, MIS), before)
    assert gpu._L.trc_update_vertices(gpu._h, None, 0, 3) == abi.ERR_INVALID_ARG
    gpu.update_vertices(np.zeros((0, 8), F), first=n)                          # count == 0: TRC_OK, nothing happens
    assert gpu._L.trc_update_vertices(gpu._h, None, 0, 0) == abi.OK
    assert same(frame(gpu, 4, MIS), before)
