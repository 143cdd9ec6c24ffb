"""trc_rebuild_tree and trc_tree_cost on the GPU (include/tracer_abi.h).  The rebuilt tree against a fresh context's upload of the same
leaf records and vertices and against the host builder / the oracle's LBVH, record for record; the frames and the instrumented walk
through it against the CPU oracle; a caller's tree through the canonical leaf order (tests/rebuild_ref.py); what the call keeps
(triangle materials, rest copy, binding, block costs) and what it drops (G-buffer, mesh-light tables, refit maps); refusals that change
nothing; the cost against the definition summed exactly.  The mesh moves first, so that the leaf boxes are the last refit's: a twist by
trc_update_vertices (rebuild_ref.TWIST, chosen in tests/test_rebuild_cpu.py), then a skin over the ragged binding of the skinning tests."""
import ctypes as C
import math

import numpy as np
import pytest

import pose_ref as pr
import rebuild_ref as rb
import refit_ref as rr
import skin_ref as sr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_pose_vertices import bits
from test_gpu_skin_vertices import bind_and_skin, small_case
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, H, W, first_difference, frame, oracle_frame, same, scene
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
SAH = abi.TREE_SAH
FLAVOURS = pytest.mark.parametrize("sah", [True, False], ids=["sah", "lbvh"])
RESIDENCES = pytest.mark.parametrize("residence", ["lds", "mem"])


def flag(sah):
    return SAH if sah else 0


def rest_of(residence):
    return rr.vertices_of(scene(residence).view)


def analytic(residence):
    return scene(residence, analytic_leaves_only=True)


class WithVertices:
    """a copy of a scene view over other vertices (kept alive here); the leaf records stay"""

    def __init__(self, view, vertices):
        self.vertices = np.ascontiguousarray(vertices, dtype=F)
        self.view = abi.Scene.from_buffer_copy(view)
        self.view.triList = C.cast(self.vertices.ctypes.data, C.POINTER(abi.TriangleVertex))


def move(t, residence):
    """twist the mesh by an update, then skin the ragged binding -> the vertices the device holds"""
    v1 = rr.twist(rest_of(residence), *rb.TWIST)
    t.update_vertices(v1)
    first, b, w, palette = small_case(residence)
    bind_and_skin(t, first, b, w, palette)
    return sr.skin(v1, v1, first, b, w, palette)               # the update's vertices are the rest vertices of the first skin


def status_of(call):
    with pytest.raises(TracerError) as e:
        call()
    return e.value.status


# --------------------------------------------------------------------------------------------------- 1. the tree
@FLAVOURS
@pytest.mark.parametrize("upload", ["device", "lbvh"])
@RESIDENCES
def test_rebuilt_tree_is_the_definition_s(gpu, residence, upload, sah):
    sc = scene(residence)
    if upload == "lbvh":
        gpu.upload_scene_lbvh(sc.leaves_view())
    else:
        gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    v = move(gpu, residence)
    before = rr.raw(gpu.download_bvh())
    gpu.rebuild_tree(flag(sah))
    got = rr.raw(gpu.download_bvh())
    assert np.array_equal(bits(gpu.download_vertices()), bits(v))                       # no vertex moves
    leaves = rb.leaf_records(before)
    with Tracer(0) as fresh:
        if upload == "device":                                                           # the same analytic leaves and the current vertices
            m = WithVertices(analytic(residence).view, v)
            fresh.upload_scene_device(m.view, DEVICE_TREE if sah else abi.TREE_TRIANGLE_LEAVES)
        else:                                                                            # the leaf records as the refit left them
            m = rr.Moved(sc.view, leaves, v)
            (fresh.upload_scene_sah if sah else fresh.upload_scene_lbvh)(m.view)
        want = rr.raw(fresh.download_bvh())
        assert fresh.lbvh_info()[:2] == gpu.lbvh_info()[:2]
    assert not first_difference(got, want)
    assert not first_difference(got, rb.expected_tree(leaves, sah))                      # trc_host_build_tree / the oracle's LBVH
    assert (got[:, :8] != before[:, :8]).any()                                           # the topology did change


# --------------------------------------------------------------------------------------------------- 2. frames and walks
@FLAVOURS
@RESIDENCES
def test_frames_and_walks_through_the_rebuilt_tree(gpu, residence, sah):
    sc = scene(residence)
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    v = move(gpu, residence)
    rays = random_rays(4000, 3, inside_only=True)
    refitted_walk = gpu.trace_rays(rays)
    gpu.rebuild_tree(flag(sah))
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    for integrator in (PATH, MIS):
        assert same(frame(gpu, 4, integrator), oracle_frame(m.view, 4, integrator)), integrator
    got, ref = gpu.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
    for f in ref.dtype.names:                                                            # n_descend among them: it pins every box
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    assert (ref["pType"][ref["hit"] != 0] == abi.PRIM_TRIANGLE).any()
    assert got["n_descend"].sum() != refitted_walk["n_descend"].sum()
    for f in ("hit", "t"):                                                               # another tree, the same closest hits
        assert (got[f].view(np.uint32) == refitted_walk[f].view(np.uint32)).all(), f


# --------------------------------------------------------------------------------------------------- 3. a caller's tree
@FLAVOURS
@RESIDENCES
def test_a_caller_s_tree_is_rebuilt_over_its_canonical_leaves(gpu, residence, sah):
    sc = scene(residence)
    gpu.upload_scene(sc.view)
    assert status_of(gpu.download_bvh) == abi.ERR_NO_SCENE and status_of(gpu.lbvh_info) == abi.ERR_NO_SCENE
    v = move(gpu, residence)
    gpu.rebuild_tree(flag(sah))
    refitted = rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view))
    want = rb.expected_tree(rb.canonical_leaves(refitted), sah)
    got = rr.raw(gpu.download_bvh())
    assert not first_difference(got, want)
    n_nodes, height, _ = gpu.lbvh_info()
    assert n_nodes == len(want) and height == rb.tree_height(want)
    m = rr.Moved(sc.view, got, v)
    for integrator in (PATH, MIS):
        assert same(frame(gpu, 4, integrator), oracle_frame(m.view, 4, integrator)), integrator
    # ... and from here on it is a device-built tree: a refit keeps its records current, a second rebuild starts from them
    v2 = rr.twist(rest_of(residence), 0.5)
    gpu.update_vertices(v2)
    again = rr.refit(got, v2, rr.indices_of(sc.view))
    assert not first_difference(rr.raw(gpu.download_bvh()), again)
    gpu.rebuild_tree(flag(sah))
    assert not first_difference(rr.raw(gpu.download_bvh()), rb.expected_tree(rb.leaf_records(again), sah))


# --------------------------------------------------------------------------------------------------- 4. what survives
@RESIDENCES
def test_triangle_materials_survive(gpu, residence):
    sc = scene(residence)
    n = sc.view.n_index // 3
    tri_mat = np.where(np.arange(n) % 3 == 0, 4, 19).astype(np.uint32)                   # Cornell's table: 4 = the red Lambert
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    gpu.upload_triangle_materials(tri_mat)
    v = move(gpu, residence)
    gpu.rebuild_tree(SAH)
    got = frame(gpu, 4, MIS)
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.any() and (hits["material"][tri] == tri_mat[hits["pIndex"][tri]]).all()
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    with Tracer(0) as fresh:                                                             # the same tree, vertices and table, uploaded
        fresh.upload_scene(m.view)
        plain = frame(fresh, 4, MIS)
        fresh.upload_triangle_materials(tri_mat)
        assert same(frame(fresh, 4, MIS), got) and not same(plain, got)
    gpu.upload_triangle_materials(None)


@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


@RESIDENCES
def test_binding_and_rest_survive_and_the_refit_maps_are_made_anew(tracer, residence):
    """from a Morton tree to the SAH tree, so that the topology the maps were made for is certainly gone"""
    sc, v0 = scene(residence), rest_of(residence)
    idx = rr.indices_of(sc.view)
    first, b, w, pal_a = small_case(residence)
    pal_b = sr.palette(5, pr.box_centre(v0))[2:]
    tracer.upload_scene_lbvh(sc.leaves_view())
    bind_and_skin(tracer, first, b, w, pal_a)                                            # makes the maps and the rest copy
    before = rr.raw(tracer.download_bvh())
    tracer.rebuild_tree(SAH)
    rebuilt = rr.raw(tracer.download_bvh())
    assert (rebuilt[:, :8] != before[:, :8]).any()
    current = sr.skin(v0, v0, first, b, w, pal_a)
    assert np.array_equal(bits(tracer.download_vertices()), bits(current))
    for palette in (pal_b, pal_a):                                                       # twice: a counter the single launch did not put back shows
        tracer.skin_vertices(palette)
        current = sr.skin(v0, current, first, b, w, palette)                             # from the original rest, bit for bit
        assert np.array_equal(bits(tracer.download_vertices()), bits(current))
        assert not first_difference(rr.raw(tracer.download_bvh()), rr.refit(rebuilt, current, idx))
    assert not np.array_equal(bits(sr.skin(v0, v0, first, b, w, pal_b)), bits(sr.skin(v0, v0, first, b, w, pal_a)))
    m = rr.Moved(sc.view, rr.raw(tracer.download_bvh()), current)
    assert same(frame(tracer, 4, PATH), oracle_frame(m.view, 4, PATH))


def test_block_costs_are_kept_and_move_no_pixel(gpu):
    sc, v0 = scene("mem"), rest_of("mem")
    v = rr.twist(v0, *rb.TWIST)
    gpu.upload_scene_device(analytic("mem").view, DEVICE_TREE)
    gpu.update_vertices(v)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    gpu.rebuild_tree(SAH)
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)                  # the costs were kept ...
    ordered = frame(gpu, 16, PATH)
    gpu.rebuild_tree(SAH)
    assert same(frame(gpu, 16, PATH, fixed_order=True), ordered)                        # ... and order is scheduling only
    assert same(ordered, oracle_frame(rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v).view, 16, PATH))


# --------------------------------------------------------------------------------------------------- 5. what is dropped
def test_gbuffer_after_a_rebuild_is_a_fresh_context_s(gpu):
    sc = scene("lds")
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE)
    v = move(gpu, "lds")
    frame(gpu, 2, PATH)
    gpu.denoise()
    gpu.rebuild_tree(SAH)
    frame(gpu, 2, PATH)
    gpu.denoise()
    after = gpu.download_gbuffer()
    with Tracer(0) as fresh:
        fresh.upload_scene(rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v).view)
        frame(fresh, 2, PATH)
        fresh.denoise()
        want = fresh.download_gbuffer()
    assert after.tobytes() == want.tobytes()


@RESIDENCES
def test_mesh_light_frame_after_a_rebuild_is_the_oracle_s(gpu, residence):
    sc = scene(residence)
    n = sc.view.n_index // 3
    tri_mat = np.full(n, 4, np.uint32); tri_mat[n // 2:n // 2 + 6] = 3                   # Cornell's table: 3 = the lamp's emitter
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    gpu.upload_triangle_materials(tri_mat)
    v = move(gpu, residence)
    frame(gpu, 2, MIS, mesh_lights=True)                                                 # the tables exist when the rebuild comes
    gpu.rebuild_tree(SAH)
    got = frame(gpu, 4, MIS, mesh_lights=True)
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    rng = host.fill_rng(9, W, H)
    acc, st = pyoracle.render(m.view, host.prepare_camera(W, H), W, H, rng, spp=4, integrator=MIS, mesh_lights=True, triangle_materials=tri_mat)
    assert same(got, (acc, rng, st.rays))
    assert not same(got, frame(gpu, 4, MIS))                                             # the flag did sample the six triangles
    gpu.upload_triangle_materials(None)


# --------------------------------------------------------------------------------------------------- 6. another height
@FLAVOURS
def test_a_tree_of_another_height_gets_its_own_lds_plan(gpu, sah):
    """rebuild_ref.TWIST takes the 48-triangle ball's tree from height 9 to 11 (SAH) or 12 (LBVH): tests/test_rebuild_cpu.py.  The whole
    tree is staged in LDS beside a traversal stack of `height` rows: a plan kept from the old height walks off its stack"""
    sc = scene("lds")
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE)
    before = gpu.lbvh_info()[1]
    v = rr.twist(rest_of("lds"), *rb.TWIST)
    gpu.update_vertices(v)
    assert gpu.lbvh_info()[1] == before
    gpu.rebuild_tree(flag(sah))
    got = rr.raw(gpu.download_bvh())
    height = gpu.lbvh_info()[1]
    assert height == rb.tree_height(got) and height != before
    m = rr.Moved(sc.view, got, v)
    assert same(frame(gpu, 4, PATH), oracle_frame(m.view, 4, PATH))
    rays = random_rays(2000, 5, inside_only=True)
    walk, ref = gpu.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
    for f in ref.dtype.names:
        assert (walk[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f


# --------------------------------------------------------------------------------------------------- 7. the smallest trees
@pytest.mark.parametrize("n", [2, 3])
def test_smallest_trees(gpu, n):
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    v = sc.leaves_view()
    v.n_bvh = n
    with Tracer(0) as fresh:
        fresh.upload_scene_lbvh(v)
        want_lbvh = rr.raw(fresh.download_bvh())
    gpu.upload_scene_sah(v)
    want_sah = rr.raw(gpu.download_bvh())
    assert len(want_sah) == 2 * n - 1
    for sah, want in ((False, want_lbvh), (True, want_sah), (False, want_lbvh)):
        gpu.rebuild_tree(flag(sah))
        assert not first_difference(rr.raw(gpu.download_bvh()), want), (n, sah)
    c = gpu.tree_cost()
    assert (c.n_interior, c.n_leaves) == (n - 2, n)


# --------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        assert status_of(lambda: fresh.rebuild_tree(SAH)) == abi.ERR_NO_SCENE
        assert status_of(fresh.tree_cost) == abi.ERR_NO_SCENE
    sc, v0 = scene("lds"), rest_of("lds")
    first, b, w, palette = small_case("lds")
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE)
    gpu.update_vertices(rr.twist(v0, *rb.TWIST))
    tree, before = rr.raw(gpu.download_bvh()), frame(gpu, 4, MIS)
    for flags in (abi.TREE_TRIANGLE_LEAVES, 4, SAH | abi.TREE_TRIANGLE_LEAVES, 0x80000000):
        assert status_of(lambda: gpu.rebuild_tree(flags)) == abi.ERR_INVALID_ARG, flags
        assert same(frame(gpu, 4, MIS), before) and not first_difference(rr.raw(gpu.download_bvh()), tree)
    assert gpu._L.trc_tree_cost(gpu._h, None) == abi.ERR_INVALID_ARG
    # a caller's tree that names one triangle in two leaves (trc_upload_scene takes it: it checks every leaf's range, not the set)
    nodes = sc.bvh_array().copy()
    tri_leaves = np.nonzero(nodes[:, rr.PTYPE] == abi.PRIM_TRIANGLE)[0]
    nodes[tri_leaves[5], rr.PINDEX] = nodes[tri_leaves[9], rr.PINDEX]
    dup = rr.Moved(sc.view, nodes, v0)
    gpu.upload_scene(dup.view)
    before = frame(gpu, 4, MIS)
    for sah in (True, False):
        assert status_of(lambda: gpu.rebuild_tree(flag(sah))) == abi.ERR_UNSUPPORTED
        assert same(frame(gpu, 4, MIS), before)
        assert status_of(gpu.download_bvh) == abi.ERR_NO_SCENE                           # still the caller's tree
    bind_and_skin(gpu, first, b, w, palette)                                             # ... and a skin still works on it
    skinned = sr.skin(v0, v0, first, b, w, palette)
    assert np.array_equal(bits(gpu.download_vertices()), bits(skinned))
    m = rr.Moved(sc.view, rr.refit(nodes, skinned, rr.indices_of(sc.view)), skinned)
    assert same(frame(gpu, 4, MIS), oracle_frame(m.view, 4, MIS))


# --------------------------------------------------------------------------------------------------- 9. the cost
def check_cost(got, tree, what):
    """counts exact; each sum within n * 2^-52 of the exactly summed definition (math.fsum over the per-slot binary64 values): twice the
    worst case (n - 1) * 2^-53 of adding n non-negative doubles in any order"""
    want = rb.tree_cost(tree)
    n = rb.n_leaves_of(tree)
    print(f"{what}: root {got.root_half_area!r} / {want['root']!r}, interior {got.interior_half_area!r} / {want['interior']!r}, "
          f"leaf {got.leaf_half_area!r} / {want['leaf']!r}, ratio {rb.ratio(got):.4f}")
    assert (got.n_interior, got.n_leaves) == (want["n_interior"], want["n_leaves"]) == (n - 2, n), what
    for name, value, terms in (("root", got.root_half_area, 1), ("interior", got.interior_half_area, n - 2), ("leaf", got.leaf_half_area, n)):
        assert abs(value - want[name]) <= terms * 2.0 ** -52 * want[name], (what, name, value, want[name])
    assert math.isfinite(rb.ratio(got)) and want["root"] > 0


@RESIDENCES
def test_tree_cost_is_the_definition_s(gpu, residence):
    sc = scene(residence)
    gpu.upload_scene(sc.view)
    check_cost(gpu.tree_cost(), sc.bvh_array().copy(), "caller's tree")
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    fresh = gpu.tree_cost()
    check_cost(fresh, rr.raw(gpu.download_bvh()), "uploaded")
    gpu.update_vertices(rr.twist(rest_of(residence), *rb.TWIST))
    worn = gpu.tree_cost()
    check_cost(worn, rr.raw(gpu.download_bvh()), "refitted")
    for sah in (True, False):
        gpu.rebuild_tree(flag(sah))
        rebuilt = gpu.tree_cost()
        check_cost(rebuilt, rr.raw(gpu.download_bvh()), "rebuilt " + ("sah" if sah else "lbvh"))
        assert rb.ratio(worn) > rb.ratio(rebuilt), sah                                   # what tests/test_rebuild_cpu.py shows of the definition
    assert rebuilt.root_half_area == worn.root_half_area                                 # the same leaves under another tree


# --------------------------------------------------------------------------------------------------- the example host
def test_example_host_rebuild_ratio(tmp_path):
    """examples/trc_render --bend 3 --rebuild-ratio 1: trc_tree_cost after every trc_skin_vertices, trc_rebuild_tree whenever the cost
    has grown at all, through the C ABI only; the count it prints is the number of rebuilds it reported"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj, out = tmp_path / "tet.obj", tmp_path / "f.png"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 3 2\nf 1 2 4\nf 2 3 4\nf 1 4 3\n")
    r = subprocess.run([os.path.join(root, "examples", "trc_render"), "--mesh", str(obj), "--size", "48", "32", "--spp", "2", "--bend", "3",
                        "--rebuild-ratio", "1", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    m = re.search(r"rebuild-ratio 1\.00: (\d+) rebuilds after (\d+) animation calls", r.stdout)
    assert m and int(m.group(2)) == 3 and int(m.group(1)) == r.stdout.count("trc_rebuild_tree") >= 1
    bad = subprocess.run([os.path.join(root, "examples", "trc_render"), "--rebuild-ratio", "0.5"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--rebuild-ratio" in bad.stderr
