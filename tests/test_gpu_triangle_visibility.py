"""trc_set_triangle_visibility / trc_download_triangle_visibility on the GPU (include/tracer_abi.h).  The tree after a
call against the definition (tests/visibility_ref.py: the analytic leaves a rebuild would start from, then one canonical record per visible
triangle) built by the host builder / the oracle's LBVH and by a fresh context's upload of that leaf list, record for record; frames and
the instrumented walk through it against the CPU oracle; triangles that move while hidden; a scene that shrinks into LDS and grows out of
it again; what the call keeps (materials, binding, rest copy, block costs, with tracking on the denoiser history) and what it drops;
hidden triangles as mesh lights; the smallest trees; refusals that change nothing.  Shapes: tests/test_gpu_update_vertices.py's."""
import numpy as np
import pytest

import pose_ref as pr
import rebuild_ref as rb
import refit_ref as rr
import skin_ref as sr
import visibility_ref as vr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_pose_vertices import bits
from test_gpu_rebuild_tree import FLAVOURS, RESIDENCES, SAH, WithVertices, analytic, flag, rest_of, status_of
from test_gpu_skin_vertices import bind_and_skin, small_case
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, H, W, first_difference, frame, oracle_frame, same, scene
from tracer_amd import abi, host
from tracer_amd.device import Tracer

pytestmark = pytest.mark.gpu
F = np.float32
ANGLE = 0.5                     # refit_ref.twist: the boxes the call finds are not the upload's


def n_triangles(residence):
    return scene(residence).view.n_index // 3


def every_second(residence):
    """(mask, ranges): the odd triangles hidden, one range each"""
    n = n_triangles(residence)
    return (np.arange(n) % 2 == 0).astype(np.uint8), [(t, 1, 0) for t in range(1, n, 2)]


def upload(t, residence, how):
    """-> (device_built, the records a rebuild would start from once the mesh is twisted by ANGLE, the twisted vertices)"""
    sc = scene(residence)
    v = rr.twist(rest_of(residence), ANGLE)
    if how == "caller":
        t.upload_scene(sc.view)
        t.update_vertices(v)
        return False, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v
    if how == "lbvh":
        t.upload_scene_lbvh(sc.leaves_view())
    else:
        t.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    t.update_vertices(v)
    return True, rr.raw(t.download_bvh()), v


def fresh_upload(fresh, residence, leaves, v, flags):
    m = rr.Moved(scene(residence).view, leaves, v)
    if flags == 0:
        fresh.upload_scene_lbvh(m.view)
    elif flags == SAH:
        fresh.upload_scene_sah(m.view)
    else:
        fresh.upload_scene_device(m.view, flags)
    return m


def check_tree(gpu, residence, leaves, v, flags, mask):
    got = rr.raw(gpu.download_bvh())
    assert len(got) == 2 * len(leaves) - 1
    with Tracer(0) as fresh:
        fresh_upload(fresh, residence, leaves, v, flags)
        assert not first_difference(got, rr.raw(fresh.download_bvh()))
        assert fresh.lbvh_info()[:2] == gpu.lbvh_info()[:2]
    if flags in (0, SAH):
        assert not first_difference(got, rb.expected_tree(leaves, flags == SAH))           # trc_host_build_tree / the oracle's LBVH
    else:
        assert not first_difference(got, rr.raw(host.build_tree(list(rr.as_nodes(leaves)), flags)))
    assert np.array_equal(gpu.triangle_visibility(), mask)
    return got


# --------------------------------------------------------------------------------------------------- 1. the tree
CASES = [("lds", how, sah) for how in ("device", "lbvh", "caller") for sah in (True, False)] + [("mem", "device", True), ("mem", "lbvh", False), ("mem", "caller", True)]


@pytest.mark.parametrize("residence,how,sah", CASES, ids=[f"{r}-{h}-{'sah' if s else 'lbvh'}" for r, h, s in CASES])
def test_tree_is_the_definition_s(gpu, residence, how, sah):
    idx = rr.indices_of(scene(residence).view)
    device_built, before, v = upload(gpu, residence, how)
    assert gpu.triangle_visibility().all()                                                 # implicit until now: every triangle has a leaf
    mask, ranges = every_second(residence)
    gpu.set_triangle_visibility(ranges, flag(sah))
    leaves = vr.leaf_list(before, device_built, v, idx, mask)
    assert len(leaves) == len(rb.leaf_records(before) if device_built else rb.canonical_leaves(before)) - int((mask == 0).sum())
    check_tree(gpu, residence, leaves, v, flag(sah), mask)
    assert np.array_equal(bits(gpu.download_vertices()), bits(v))                          # no vertex moves


def test_tree_under_sah3(gpu):
    flags = SAH | abi.TREE_SAH3
    idx = rr.indices_of(scene("mem").view)
    device_built, before, v = upload(gpu, "mem", "device")
    mask, ranges = every_second("mem")
    gpu.set_triangle_visibility(ranges, flags)
    check_tree(gpu, "mem", vr.leaf_list(before, device_built, v, idx, mask), v, flags, mask)


def test_ranges_apply_in_order_and_none_rebuilds_from_the_mask(gpu):
    idx = rr.indices_of(scene("lds").view)
    device_built, before, v = upload(gpu, "lds", "device")
    ranges = [(0, 48, 0), (8, 30, 1), (10, 4, 0), (47, 1, 1), (20, 0, 0), (12, 1, 1)]
    mask = vr.apply_ranges(np.ones(48, np.uint8), ranges)
    assert mask.sum() == 30 - 4 + 1 + 1
    gpu.set_triangle_visibility(ranges, SAH)
    tree = check_tree(gpu, "lds", vr.leaf_list(before, device_built, v, idx, mask), v, SAH, mask)
    gpu.set_triangle_visibility([], 0)                                                     # the same leaves under the other build
    leaves = vr.leaf_list(tree, True, v, idx, mask)
    assert np.array_equal(leaves, rb.leaf_records(tree))
    check_tree(gpu, "lds", leaves, v, 0, mask)


# --------------------------------------------------------------------------------------------------- 2. frames and walks
@FLAVOURS
@RESIDENCES
def test_frames_and_walks_through_the_smaller_tree(gpu, residence, sah):
    sc = scene(residence)
    _, _, v = upload(gpu, residence, "device")
    all_visible = {i: frame(gpu, 4, i) for i in (PATH, MIS)}
    mask, ranges = every_second(residence)
    gpu.set_triangle_visibility(ranges, flag(sah))
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    for integrator in (PATH, MIS):
        got = frame(gpu, 4, integrator)
        assert same(got, oracle_frame(m.view, 4, integrator)), integrator
        assert not same(got, all_visible[integrator])
    rays = random_rays(4000, 3, inside_only=True)
    got, ref = gpu.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
    for f in ref.dtype.names:                                                              # n_descend among them: it pins every box
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    tri = (got["hit"] != 0) & (got["pType"] == abi.PRIM_TRIANGLE)
    assert tri.any() and mask[got["pIndex"][tri]].all()                                    # no hit names a hidden triangle
    production = gpu.trace_rays(rays, production=True)
    tri = (production["hit"] != 0) & (production["pType"] == abi.PRIM_TRIANGLE)
    assert tri.any() and mask[production["pIndex"][tri]].all()


# --------------------------------------------------------------------------------------------------- 3. moved while hidden
CASES3 = [("lds", True), ("lds", False), ("mem", True)]


@pytest.mark.parametrize("residence,sah", CASES3, ids=[f"{r}-{'sah' if s else 'lbvh'}" for r, s in CASES3])
def test_triangles_that_moved_while_hidden_come_back_where_they_are(gpu, residence, sah):
    n = n_triangles(residence)
    hidden = (n // 4, n // 2, 0)
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE)
    gpu.set_triangle_visibility([hidden], flag(sah))
    v = rr.twist(rest_of(residence), *rb.TWIST)
    if sah:
        gpu.update_vertices(v)
    else:                                                                                  # ... or a pose, whose vertices the device computes
        turn = pr.turn(pr.box_centre(rest_of(residence)), 0.7)
        gpu.pose_vertices([(0, len(v), *turn)])
        v = gpu.download_vertices()
    gpu.set_triangle_visibility([(hidden[0], hidden[1], 1)], flag(sah))
    assert gpu.triangle_visibility().all()
    with Tracer(0) as fresh:
        m = WithVertices(analytic(residence).view, v)
        fresh.upload_scene_device(m.view, DEVICE_TREE if sah else abi.TREE_TRIANGLE_LEAVES)
        assert not first_difference(rr.raw(gpu.download_bvh()), rr.raw(fresh.download_bvh()))
        assert fresh.lbvh_info()[:2] == gpu.lbvh_info()[:2]
        assert same(frame(gpu, 4, PATH), frame(fresh, 4, PATH))
    full = rr.Moved(scene(residence).view, rr.raw(gpu.download_bvh()), v)
    assert same(frame(gpu, 4, MIS), oracle_frame(full.view, 4, MIS))


# --------------------------------------------------------------------------------------------------- 4. across the LDS boundary
def kernel_of(t):
    k = t.last_kernel()
    return {name: k[name] for name in ("shape", "variant", "lds_resident", "triangle_materials", "strip")}


def shape_of(t):
    s = t.launch_shape()
    return s["entries"], s["wave_slots"]


def test_shrink_into_lds_and_grow_out_again():
    sc, v = scene("mem"), rest_of("mem")
    idx, n = rr.indices_of(sc.view), n_triangles("mem")
    mask = (np.arange(n) % 125 == 0).astype(np.uint8)
    assert mask.sum() == 40
    with Tracer(0, hooks=True) as t, Tracer(0, hooks=True) as fresh:
        t.upload_scene_device(analytic("mem").view, DEVICE_TREE)
        full_tree = rr.raw(t.download_bvh())
        frame(t, 4, PATH)
        assert not kernel_of(t)["lds_resident"]
        t.set_triangle_visibility(vr.ranges_of(np.ones(n, np.uint8), mask), SAH)
        leaves = vr.leaf_list(full_tree, True, v, idx, mask)
        fresh_upload(fresh, "mem", leaves, v, SAH)
        assert not first_difference(rr.raw(t.download_bvh()), rr.raw(fresh.download_bvh()))
        got, want = frame(t, 4, PATH), frame(fresh, 4, PATH)
        assert same(got, want)
        assert kernel_of(t) == kernel_of(fresh) and kernel_of(t)["lds_resident"]         # the whole tree is staged now
        assert shape_of(t) == shape_of(fresh)
        small = rr.Moved(sc.view, rr.raw(t.download_bvh()), v)
        assert same(got, oracle_frame(small.view, 4, PATH))
        # everything again: the node region and the record array still have the room
        t.set_triangle_visibility([(0, n, 1)], SAH)
        fresh.upload_scene_device(analytic("mem").view, DEVICE_TREE)
        fresh.rebuild_tree(SAH)
        assert not first_difference(rr.raw(t.download_bvh()), rr.raw(fresh.download_bvh()))
        assert t.lbvh_info()[:2] == fresh.lbvh_info()[:2]
        got = frame(t, 4, PATH)
        assert not kernel_of(t)["lds_resident"]
        assert same(got, oracle_frame(rr.Moved(sc.view, rr.raw(t.download_bvh()), v).view, 4, PATH))


# --------------------------------------------------------------------------------------------------- 5. what survives
@RESIDENCES
def test_triangle_materials_survive(gpu, residence):
    sc, n = scene(residence), n_triangles(residence)
    tri_mat = np.where(np.arange(n) % 3 == 0, 4, 19).astype(np.uint32)                     # Cornell's table: 4 = the red Lambert
    _, _, v = upload(gpu, residence, "device")
    gpu.upload_triangle_materials(tri_mat)
    mask, ranges = every_second(residence)
    gpu.set_triangle_visibility(ranges, SAH)
    got = frame(gpu, 4, MIS)
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.any() and (hits["material"][tri] == tri_mat[hits["pIndex"][tri]]).all()
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    with Tracer(0) as fresh:
        fresh.upload_scene(m.view)
        plain = frame(fresh, 4, MIS)
        fresh.upload_triangle_materials(tri_mat)
        assert same(frame(fresh, 4, MIS), got) and not same(plain, got)
    gpu.set_triangle_visibility([(0, n, 1)], SAH)                                          # hidden triangles kept theirs
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert (mask[hits["pIndex"][tri]] == 0).any() and (hits["material"][tri] == tri_mat[hits["pIndex"][tri]]).all()
    gpu.upload_triangle_materials(None)


@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


@RESIDENCES
def test_binding_and_rest_survive_and_the_smaller_tree_is_refitted(tracer, residence):
    sc, v0 = scene(residence), rest_of(residence)
    idx = rr.indices_of(sc.view)
    first, b, w, pal_a = small_case(residence)
    pal_b = sr.palette(5, pr.box_centre(v0))[2:]
    tracer.upload_scene_lbvh(sc.leaves_view())
    bind_and_skin(tracer, first, b, w, pal_a)                                              # makes the maps and the rest copy
    mask, ranges = every_second(residence)
    tracer.set_triangle_visibility(ranges, SAH)
    smaller = rr.raw(tracer.download_bvh())
    current = sr.skin(v0, v0, first, b, w, pal_a)
    assert np.array_equal(bits(tracer.download_vertices()), bits(current))
    for palette in (pal_b, pal_a):                                                         # twice: a counter the single launch did not put back shows
        tracer.skin_vertices(palette)
        current = sr.skin(v0, current, first, b, w, palette)                               # from the original rest, hidden vertices too
        assert np.array_equal(bits(tracer.download_vertices()), bits(current))
        assert not first_difference(rr.raw(tracer.download_bvh()), rr.refit(smaller, current, idx))
    v = rr.twist(v0, ANGLE)
    tracer.update_vertices(v)
    refitted = rr.refit(smaller, v, idx)
    assert not first_difference(rr.raw(tracer.download_bvh()), refitted)
    assert same(frame(tracer, 4, PATH), oracle_frame(rr.Moved(sc.view, refitted, v).view, 4, PATH))
    tracer.rebuild_tree(SAH)                                                               # a plain rebuild keeps n': the visible leaves only
    assert not first_difference(rr.raw(tracer.download_bvh()), rb.expected_tree(rb.leaf_records(refitted), True))
    assert np.array_equal(tracer.triangle_visibility(), mask)


def test_block_costs_are_kept_and_move_no_pixel(gpu):
    sc, v = scene("mem"), rest_of("mem")
    gpu.upload_scene_device(analytic("mem").view, DEVICE_TREE)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    mask, ranges = every_second("mem")
    gpu.set_triangle_visibility(ranges, SAH)
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)                     # the costs were kept ...
    ordered = frame(gpu, 16, PATH)
    gpu.set_triangle_visibility([], SAH)
    assert same(frame(gpu, 16, PATH, fixed_order=True), ordered)                           # ... and order is scheduling only
    assert same(ordered, oracle_frame(rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v).view, 16, PATH))


# --------------------------------------------------------------------------------------------------- 6. mesh lights
@RESIDENCES
def test_a_hidden_triangle_is_no_light(gpu, residence):
    sc, n = scene(residence), n_triangles(residence)
    lights = np.arange(n // 2, n // 2 + 6)
    tri_mat = np.full(n, 4, np.uint32); tri_mat[lights] = 3                                # Cornell's table: 3 = the lamp's emitter
    _, _, v = upload(gpu, residence, "device")
    gpu.upload_triangle_materials(tri_mat)
    before = frame(gpu, 4, MIS, mesh_lights=True)                                          # the tables exist when the call comes
    gpu.set_triangle_visibility([(int(t), 1, 0) for t in lights[::2]], SAH)
    got = frame(gpu, 4, MIS, mesh_lights=True)
    dark = tri_mat.copy(); dark[lights[::2]] = 4                                           # the same light set by the existing definition
    m = rr.Moved(sc.view, rr.raw(gpu.download_bvh()), v)
    rng = host.fill_rng(9, W, H)
    acc, st = pyoracle.render(m.view, host.prepare_camera(W, H), W, H, rng, spp=4, integrator=MIS, mesh_lights=True, triangle_materials=dark)
    assert same(got, (acc, rng, st.rays))
    assert not same(got, before) and not same(got, frame(gpu, 4, MIS))
    gpu.upload_triangle_materials(None)


# --------------------------------------------------------------------------------------------------- 7. the denoiser
def denoised_frame(t, k):
    t.clear_accum()
    t.render(spp=1, frame0=k, integrator=PATH)
    t.denoise()


@pytest.mark.parametrize("tracking", [False, True], ids=["untracked", "tracked"])
def test_history_across_the_call(tracking):
    with Tracer(0) as t:
        t.denoise_track_motion(tracking)
        t.upload_scene_device(analytic("lds").view, DEVICE_TREE)
        t.set_camera(host.prepare_camera(W, H)); t.set_environment((0.0, 0.0, 0.0)); t.resize(W, H); t.seed(11)
        for k in range(3):
            denoised_frame(t, k)
        gb_before, n_before = t.download_gbuffer().copy(), t.download_history_length().copy()
        ids_before = gb_before["id"]
        hit = (ids_before != abi.GBUFFER_MISS) & (n_before > 1)                             # the pixels that have a history to lose
        print(f"{int(hit.sum())} of {W * H} pixels with a history, lengths {np.unique(n_before[hit])}")
        assert hit.sum() > W * H // 2
        t.set_triangle_visibility(every_second("lds")[1], SAH)
        denoised_frame(t, 3)
        gb_after, n_after = t.download_gbuffer(), t.download_history_length()
        # the texel's id is the hit's MATERIAL (19 for every triangle): the primary hit is the same iff id, depth and normal are, bit for bit
        changed = np.zeros((H, W), bool)
        for name in ("id", "depth", "normal"):
            a, b = np.ascontiguousarray(gb_before[name]).view(np.uint32).reshape(H, W, -1), np.ascontiguousarray(gb_after[name]).view(np.uint32).reshape(H, W, -1)
            changed |= (a != b).any(-1)
        assert (gb_after["id"] != ids_before).any()                                          # ... the wall behind a triangle among them
        print(f"{int(changed.sum())} pixels show another surface; lengths after the call {np.unique(n_after)}")
        assert (hit & changed).any() and (hit & ~changed).any()
        if not tracking:
            assert (n_after == 1).all()
        else:
            assert (n_after[changed] == 1).all()                                           # a surface appeared or vanished
            keep = hit & ~changed                                                          # the same surface: its history goes on
            assert (n_after[keep] > 1).all() and (n_after[keep] >= n_before[keep]).all()


# --------------------------------------------------------------------------------------------------- 8. the smallest trees
def test_smallest_trees(gpu):
    sc = scene("lds")
    idx, v = rr.indices_of(sc.view), rest_of("lds")
    view = abi.Scene.from_buffer_copy(analytic("lds").view)
    view.n_bvh = 1                                                                         # one analytic leaf + the 48 triangles
    gpu.upload_scene_device(view, DEVICE_TREE)
    before = rr.raw(gpu.download_bvh())
    assert len(before) == 2 * 49 - 1
    for sah in (True, False):
        mask = np.zeros(48, np.uint8); mask[17] = 1
        gpu.set_triangle_visibility([(0, 48, 0), (17, 1, 1)], flag(sah))
        leaves = vr.leaf_list(before, True, v, idx, mask)
        assert len(leaves) == 2
        got = check_tree(gpu, "lds", leaves, v, flag(sah), mask)
        assert len(got) == 3
        assert same(frame(gpu, 2, PATH), oracle_frame(rr.Moved(sc.view, got, v).view, 2, PATH))
        assert status_of(lambda: gpu.set_triangle_visibility([(0, 48, 0)], flag(sah))) == abi.ERR_INVALID_ARG      # one leaf left
        assert not first_difference(rr.raw(gpu.download_bvh()), got) and np.array_equal(gpu.triangle_visibility(), mask)
        gpu.set_triangle_visibility([(0, 48, 1)], flag(sah))
        assert gpu.lbvh_info()[0] == 2 * 49 - 1


def test_a_scene_without_triangles_is_rebuilt_over_its_leaves(gpu):
    sc = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    gpu.upload_scene_sah(sc.leaves_view())
    leaves = rb.leaf_records(rr.raw(gpu.download_bvh()))
    assert len(gpu.triangle_visibility()) == 0
    for sah in (False, True):
        gpu.set_triangle_visibility([], flag(sah))
        assert not first_difference(rr.raw(gpu.download_bvh()), rb.expected_tree(leaves, sah))
    assert status_of(lambda: gpu.set_triangle_visibility([(0, 1, 0)], SAH)) == abi.ERR_INVALID_ARG
    assert same(frame(gpu, 2, PATH), oracle_frame(sc.view, 2, PATH))


# --------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_change_nothing(gpu):
    with Tracer(0) as fresh:
        assert status_of(lambda: fresh.set_triangle_visibility([(0, 1, 0)], SAH)) == abi.ERR_NO_SCENE
        assert status_of(fresh.triangle_visibility) == abi.ERR_NO_SCENE
        assert status_of(fresh.download_bvh) == abi.ERR_NO_SCENE
    sc, v0 = scene("lds"), rest_of("lds")
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE)
    gpu.update_vertices(rr.twist(v0, ANGLE))
    gpu.set_triangle_visibility([(3, 7, 0)], SAH)
    tree, before, mask = rr.raw(gpu.download_bvh()), frame(gpu, 4, MIS), gpu.triangle_visibility()
    assert mask.sum() == 41

    def unchanged():
        return same(frame(gpu, 4, MIS), before) and not first_difference(rr.raw(gpu.download_bvh()), tree) and np.array_equal(gpu.triangle_visibility(), mask)

    for flags in (abi.TREE_TRIANGLE_LEAVES, abi.TREE_SAH3, SAH | abi.TREE_TRIANGLE_LEAVES, 0x80000000):
        assert status_of(lambda: gpu.set_triangle_visibility([(0, 48, 1)], flags)) == abi.ERR_INVALID_ARG, flags
        assert unchanged()
    for ranges in ([(0, 48, 1), (40, 9, 0)], [(49, 0, 0)], [(0xFFFFFFFF, 2, 0)], [(0, 48, 1), (5, 1, 2)]):
        assert status_of(lambda: gpu.set_triangle_visibility(ranges, SAH)) == abi.ERR_INVALID_ARG, ranges
        assert unchanged()
    assert gpu._L.trc_set_triangle_visibility(gpu._h, None, 1, SAH) == abi.ERR_INVALID_ARG and unchanged()
    assert gpu._L.trc_download_triangle_visibility(gpu._h, None) == abi.ERR_INVALID_ARG
    gpu.set_triangle_visibility(None, SAH)                                                 # NULL with n_ranges == 0 is legal
    assert unchanged()
    # a caller's tree that names one triangle in two leaves has no mask
    nodes = sc.bvh_array().copy()
    tri_leaves = np.nonzero(nodes[:, rr.PTYPE] == abi.PRIM_TRIANGLE)[0]
    nodes[tri_leaves[5], rr.PINDEX] = nodes[tri_leaves[9], rr.PINDEX]
    dup = rr.Moved(sc.view, nodes, v0)
    gpu.upload_scene(dup.view)
    before = frame(gpu, 4, MIS)
    for call in (lambda: gpu.set_triangle_visibility([(0, 4, 0)], SAH), lambda: gpu.set_triangle_visibility([], 0), gpu.triangle_visibility):
        assert status_of(call) == abi.ERR_UNSUPPORTED
        assert same(frame(gpu, 4, MIS), before)
        assert status_of(gpu.download_bvh) == abi.ERR_NO_SCENE                             # still the caller's tree
    # an upload drops the mask: the next tree defines it again
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE)
    gpu.set_triangle_visibility([(0, 10, 0)], SAH)
    gpu.upload_scene(sc.view)
    assert gpu.triangle_visibility().all()
