"""trc_update_primitives on the GPU (include/tracer_abi.h): the refitted tree and the frames rendered through it against the definition
(tests/primitives_ref.py) and the CPU oracle, bit for bit; the call beside the other moving calls and trc_rebuild_tree; what it keeps
(triangle materials, a skin binding, block costs); refusals that change nothing.  The motion is primitives_ref.motion: sphere 0 and
three others, the light square 5, cube 0 and the container cube, all at once."""
import ctypes as C

import numpy as np
import pytest

import pose_ref as por
import primitives_ref as pr
import rebuild_ref as rb
import refit_ref as rr
import skin_ref as sr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_rebuild_tree import check_cost
from test_gpu_skin_vertices import bind_and_skin, small_case
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, H, W, first_difference, frame, oracle_frame, same, scene
from tracer_amd import abi, host
from tracer_amd.device import Tracer, TracerError

pytestmark = pytest.mark.gpu
F = np.float32
_SPHERES = {}


def scn(name, analytic_leaves_only=False):
    """'spheres': SCENE_CORNELL_SPHERES (21 leaves, the whole tree in LDS); 'lds' / 'mem': Cornell + the 48- / 5 000-triangle ball"""
    if name != "spheres":
        return scene(name, analytic_leaves_only)
    if "s" not in _SPHERES:
        _SPHERES["s"] = host.HostScene(abi.SCENE_CORNELL_SPHERES)
    return _SPHERES["s"]


def mesh_of(view):
    return (rr.vertices_of(view), rr.indices_of(view)) if view.n_vertex else (None, None)


def moved(name, phase=1.0, nodes=None, vertices=None):
    """(lists, the scene over those lists and over refit() of `nodes` -- the host tree unless given)"""
    sc = scn(name)
    lists = pr.motion(sc.view, phase)
    v, idx = mesh_of(sc.view)
    if vertices is not None:
        v = vertices
    records = pr.refit(sc.bvh_array().copy() if nodes is None else nodes, *lists, v, idx)
    return lists, pr.Moved(sc.view, records, *lists, vertices=vertices)


def update(t, lists):
    t.update_primitives(spheres=lists[0], squares=lists[1], cubes=lists[2])


def status_of(call):
    with pytest.raises(TracerError) as e:
        call()
    return e.value.status


@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


# --------------------------------------------------------------------------------------------------- 1. device trees
@pytest.mark.parametrize("name,tree", [("spheres", "lbvh"), ("spheres", "sah"), ("lds", "lbvh"), ("lds", "sah_triangle_leaves"), ("mem", "sah"),
                                       ("mem", "sah_triangle_leaves")])
def test_downloaded_tree_is_the_refit_of_the_tree_before(tracer, name, tree):
    sc = scn(name)
    if tree == "lbvh":
        tracer.upload_scene_lbvh(sc.leaves_view())
    elif tree == "sah":
        tracer.upload_scene_sah(sc.leaves_view())
    else:
        tracer.upload_scene_device(scn(name, analytic_leaves_only=True).view, DEVICE_TREE)
    before = rr.raw(tracer.download_bvh())
    v, idx = mesh_of(sc.view)
    got = before
    for phase in (1.0, 0.35, 1.0):                                     # the third: counters the single launch did not put back would show
        lists = pr.motion(sc.view, phase)
        update(tracer, lists)
        got = rr.raw(tracer.download_bvh())
        want = pr.refit(before, *lists, v, idx)
        assert not first_difference(got, want), phase
    assert (got[:, :8] == before[:, :8]).all()                         # links, axis, pType, pIndex: the topology stays
    assert (got[:, 8:] != before[:, 8:]).any()                         # ... and boxes moved
    assert tracer.refit_ms() > 0.0


# --------------------------------------------------------------------------------------------------- 2. a host tree
@pytest.mark.parametrize("name", ["spheres", "lds", "mem"])
def test_host_tree_walk_counts_every_box(tracer, name):
    """the instrumented walk's counters depend on every box of the tree: they pin a tree that cannot be downloaded"""
    lists, m = moved(name)
    tracer.upload_scene(scn(name).view)
    update(tracer, lists)
    rays = random_rays(4000, 3, inside_only=True)
    got, ref = tracer.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
    for f in ref.dtype.names:
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    old = pyoracle.trace_rays(scn(name).view, rays)
    assert (ref["t"].view(np.uint32) != old["t"].view(np.uint32)).sum() > 100 and ref["n_descend"].sum() != old["n_descend"].sum()
    for t in (abi.PRIM_SQUARE, abi.PRIM_CUBE) + ((abi.PRIM_SPHERE,) if name == "spheres" else (abi.PRIM_TRIANGLE,)):
        assert (ref["pType"][ref["hit"] != 0] == t).any(), t


# --------------------------------------------------------------------------------------------------- 3. frames against the oracle
@pytest.mark.parametrize("integrator", [PATH, MIS])
@pytest.mark.parametrize("name", ["spheres", "mem"])
def test_frame_after_update_is_the_oracle_s(gpu, name, integrator):
    sc = scn(name)
    lists, m = moved(name)
    gpu.upload_scene(sc.view)
    original = frame(gpu, 4, integrator)
    update(gpu, lists)
    got = frame(gpu, 4, integrator)
    assert same(got, oracle_frame(m.view, 4, integrator))
    assert not same(got, original)
    with Tracer(0) as fresh:                                            # ... and what uploading the moved scene gives
        fresh.upload_scene(m.view)
        assert same(frame(fresh, 4, integrator), got)
    # two calls in a row are one call to the final state; a call with one kind leaves the others
    lists2, m2 = moved(name, 0.4)
    gpu.update_primitives(spheres=lists2[0])
    gpu.update_primitives(cubes=lists2[2], squares=lists2[1][5:6], first_square=5)
    twice = frame(gpu, 4, integrator)
    assert same(twice, oracle_frame(m2.view, 4, integrator))
    with Tracer(0) as fresh:
        fresh.upload_scene(sc.view)
        update(fresh, lists2)
        assert same(frame(fresh, 4, integrator), twice)
    # back to the scene's own records: the first frame
    update(gpu, pr.motion(sc.view, 0.0))
    assert same(frame(gpu, 4, integrator), original)


def test_device_tree_frame_after_update(gpu):
    """the refit of a device-built tree renders as the upload of the downloaded records does"""
    sc = scn("mem")
    gpu.upload_scene_device(scn("mem", analytic_leaves_only=True).view, DEVICE_TREE)
    lists = pr.motion(sc.view)
    update(gpu, lists)
    got = frame(gpu, 4, PATH)
    m = pr.Moved(sc.view, rr.raw(gpu.download_bvh()), *lists)
    assert same(got, oracle_frame(m.view, 4, PATH))


# --------------------------------------------------------------------------------------------------- 4. the container cube as a leaf
def test_volume_scene_with_the_container_moved(gpu):
    sc = host.HostScene(abi.SCENE_CORNELL_VOLUME)
    cloud = host.make_cloud()
    info = host.density_info(cloud)
    lists = pr.motion(sc.view)
    m = pr.Moved(sc.view, pr.refit(sc.bvh_array().copy(), *lists), *lists)
    assert (rr.raw(m.nodes) != sc.bvh_array()).any()
    cam = host.prepare_camera(W, H)
    gpu.upload_scene(sc.view); gpu.set_camera(cam); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
    gpu.upload_density(info, cloud)
    pyoracle.set_density(info, cloud)
    try:
        gpu.update_primitives(cubes=lists[2][2:3], first_cube=2)                 # the container alone ...
        gpu.update_primitives(spheres=lists[0], squares=lists[1], cubes=lists[2][:2])      # ... then the rest
        rng = host.fill_rng(21, W, H)
        gpu.upload_rng(rng); gpu.clear_accum(); gpu.reset_stats()
        gpu.render(spp=4, integrator=abi.INTEGRATOR_VOLUME)
        got, got_rng, rays = gpu.download_accum(), gpu.download_rng(), gpu.stats().rays
        ref, ref_st = pyoracle.render(m.view, cam, W, H, rng, spp=4, integrator=abi.INTEGRATOR_VOLUME)
        assert (got.view(np.uint32) == ref.view(np.uint32)).all() and (got_rng == rng).all() and rays == ref_st.rays
        rng0 = host.fill_rng(21, W, H)
        ref0, _ = pyoracle.render(sc.view, cam, W, H, rng0, spp=4, integrator=abi.INTEGRATOR_VOLUME)
        assert (ref0.view(np.uint32) != ref.view(np.uint32)).any()
    finally:
        pyoracle.set_density(None, None)
        gpu.upload_density(None, None)


# --------------------------------------------------------------------------------------------------- 5. a primitive without a leaf
def test_a_primitive_without_a_leaf_leaves_the_tree_alone(gpu):
    """Cornell + ball: no leaf names a sphere or the container cube"""
    sc = scn("lds")
    assert not (sc.bvh_array()[:, rr.PTYPE] == abi.PRIM_SPHERE).any()
    lists = pr.motion(sc.view)
    gpu.upload_scene_lbvh(sc.leaves_view())
    before = rr.raw(gpu.download_bvh())
    original = frame(gpu, 4, PATH)
    gpu.update_primitives(spheres=lists[0], cubes=lists[2][2:3], first_cube=2)
    got = rr.raw(gpu.download_bvh())
    assert (got[:, :11] == before[:, :11]).all() and (got[:, 12:15] == before[:, 12:15]).all()      # every link and every box
    own = pr.motion(sc.view, 0.0)
    m = pr.Moved(sc.view, got, lists[0], own[1], (abi.Cube * 3)(own[2][0], own[2][1], lists[2][2]))
    after = frame(gpu, 4, PATH)
    assert same(after, oracle_frame(m.view, 4, PATH)) and same(after, original)                      # nothing that is walked changed
    with Tracer(0) as fresh:
        fresh.upload_scene(m.view)
        assert same(frame(fresh, 4, PATH), after)


# --------------------------------------------------------------------------------------------------- 6. beside a pose
@pytest.mark.parametrize("order", ["primitives_first", "pose_first"])
def test_update_primitives_and_pose_vertices_commute(tracer, order):
    sc = scn("mem")
    v0, idx = mesh_of(sc.view)
    n = len(v0)
    model, normal = por.turn(por.box_centre(v0), 0.6, (1.1, 0.8, 1.0), (25.0, -10.0, 15.0))
    posed = por.pose(v0, v0, [(0, n, model, normal)])
    lists, m = moved("mem", vertices=posed)
    tracer.upload_scene(sc.view)
    if order == "primitives_first":
        update(tracer, lists); tracer.pose_vertices([(0, n, model, normal)])
    else:
        tracer.pose_vertices([(0, n, model, normal)]); update(tracer, lists)
    assert np.array_equal(tracer.download_vertices().view(np.uint32), posed.view(np.uint32))
    assert same(frame(tracer, 4, MIS), oracle_frame(m.view, 4, MIS))


# --------------------------------------------------------------------------------------------------- 7. a rebuild behind it
@pytest.mark.parametrize("sah", [True, False], ids=["sah", "lbvh"])
def test_rebuild_after_an_update_builds_from_the_new_leaves(gpu, sah):
    sc = scn("spheres")
    lists = pr.motion(sc.view)
    gpu.upload_scene_lbvh(sc.leaves_view())
    before = rr.raw(gpu.download_bvh())
    update(gpu, lists)
    refitted = pr.refit(before, *lists)
    cost = gpu.tree_cost()
    check_cost(cost, refitted, "after trc_update_primitives")                            # the definition over the restated refit
    assert cost.leaf_half_area != rb.tree_cost(before)["leaf"]
    gpu.rebuild_tree(abi.TREE_SAH if sah else 0)
    got = rr.raw(gpu.download_bvh())
    leaves = rb.leaf_records(refitted)
    assert not first_difference(got, rb.expected_tree(leaves, sah))
    with Tracer(0) as fresh:                                                             # a fresh device upload of the moved leaves
        m = pr.Moved(sc.view, leaves, *lists)
        (fresh.upload_scene_sah if sah else fresh.upload_scene_lbvh)(m.view)
        assert not first_difference(got, rr.raw(fresh.download_bvh()))
    m = pr.Moved(sc.view, got, *lists)
    assert same(frame(gpu, 4, PATH), oracle_frame(m.view, 4, PATH))


# --------------------------------------------------------------------------------------------------- 8. what survives
def test_triangle_materials_a_skin_binding_and_block_costs_survive(gpu):
    sc = scn("mem")
    v0, idx = mesh_of(sc.view)
    n_tri = sc.view.n_index // 3
    tri_mat = np.where(np.arange(n_tri) % 3 == 0, 4, 19).astype(np.uint32)               # Cornell's table: 4 = the red Lambert
    first, b, w, palette = small_case("mem")
    gpu.upload_scene(sc.view)
    gpu.upload_triangle_materials(tri_mat)
    bind_and_skin(gpu, first, b, w, palette)
    skinned = sr.skin(v0, v0, first, b, w, palette)
    for _ in range(3):
        frame(gpu, 16, PATH)
    tiles, costs, _ = gpu.block_costs()
    assert len(tiles) > 0 and costs.any()
    lists, m = moved("mem", vertices=skinned)
    update(gpu, lists)
    tiles2, costs2, _ = gpu.block_costs()
    assert len(tiles2) == len(tiles) and np.array_equal(costs2, costs)                   # the costs were kept
    assert np.array_equal(gpu.download_vertices().view(np.uint32), skinned.view(np.uint32))
    got = frame(gpu, 4, MIS)
    rng = host.fill_rng(9, W, H)
    ref, st = pyoracle.render(m.view, host.prepare_camera(W, H), W, H, rng, spp=4, integrator=MIS, triangle_materials=tri_mat)
    assert same(got, (ref, rng, st.rays))
    gpu.skin_vertices(palette)                                                           # the binding and the rest copy are still there
    assert np.array_equal(gpu.download_vertices().view(np.uint32), skinned.view(np.uint32))
    assert same(frame(gpu, 4, MIS), got)
    gpu.upload_triangle_materials(None)


# --------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_change_nothing(gpu):
    r = abi.PrimitiveRanges()
    with Tracer(0) as fresh:
        assert fresh._L.trc_update_primitives(fresh._h, C.byref(r)) == abi.ERR_NO_SCENE
        assert fresh._L.trc_update_primitives(fresh._h, None) == abi.ERR_NO_SCENE
    sc = scn("spheres")
    gpu.upload_scene_lbvh(sc.leaves_view())
    tree = rr.raw(gpu.download_bvh())
    before = frame(gpu, 4, MIS)
    sp, sq, cb = pr.motion(sc.view)
    big = 0xFFFFFFFF

    def edited(rec, fn):
        c = type(rec).from_buffer_copy(bytes(rec)); fn(c); return c
    bad_calls = [
        dict(spheres=sp, first_sphere=1), dict(spheres=sp[:2], first_sphere=11), dict(spheres=sp[:1], first_sphere=12), dict(spheres=sp[:2], first_sphere=big),
        dict(squares=sq, first_square=1), dict(squares=sq[:1], first_square=big), dict(cubes=cb, first_cube=1), dict(cubes=cb[:2], first_cube=big - 1),
        dict(spheres=sp, cubes=cb, squares=[edited(sq[5], lambda s: setattr(s, "material", 20))], first_square=5),      # the last list checked is bad
        dict(spheres=[edited(sp[0], lambda s: setattr(s, "material", big))]), dict(cubes=[edited(cb[0], lambda s: setattr(s, "material", 20))]),
        dict(squares=[edited(sq[5], lambda s: setattr(s, "axis_k", 3))], first_square=5), dict(squares=[edited(sq[5], lambda s: setattr(s, "axis_i", 255))]),
        dict(spheres=[edited(sp[0], lambda s: setattr(s, "radius", float("nan")))]), dict(spheres=[edited(sp[0], lambda s: setattr(s.center, "x", float("inf")))]),
        dict(spheres=[edited(sp[0], lambda s: setattr(s.boundingBOX.maxi, "y", 2e37))]), dict(spheres=[edited(sp[0], lambda s: setattr(s.model_matrix.columns[3], "z", -2e37))]),
        dict(squares=[edited(sq[5], lambda s: setattr(s, "value_k", float("nan")))]), dict(squares=[edited(sq[5], lambda s: setattr(s.range_j, "y", -float("inf")))]),
        dict(cubes=[edited(cb[0], lambda s: setattr(s.inverse_matrix.columns[1], "y", float("nan")))]), dict(cubes=[edited(cb[0], lambda s: setattr(s.normal_matrix.columns[2], "z", 3e37))]),
        dict(spheres=sp, cubes=[edited(cb[0], lambda s: setattr(s.box.mini, "x", float("nan")))]),
    ]
    for kw in bad_calls:
        assert status_of(lambda: gpu.update_primitives(**kw)) == abi.ERR_INVALID_ARG, kw.keys()
    assert gpu._L.trc_update_primitives(gpu._h, None) == abi.ERR_INVALID_ARG
    for name in ("sphere", "square", "cube"):                                    # a NULL list with a count
        r = abi.PrimitiveRanges(); setattr(r, "n_" + name, 1)
        assert gpu._L.trc_update_primitives(gpu._h, C.byref(r)) == abi.ERR_INVALID_ARG
    assert same(frame(gpu, 4, MIS), before) and np.array_equal(rr.raw(gpu.download_bvh()), tree)


# --------------------------------------------------------------------------------------------------- 10. the empty call
def test_an_empty_call_changes_nothing(gpu):
    sc = scn("spheres")
    gpu.upload_scene(sc.view)
    frame(gpu, 2, PATH)
    for _ in range(3):
        gpu.denoise()
    n = gpu.download_history_length()
    assert n.max() >= 3
    gpu.update_primitives()
    r = abi.PrimitiveRanges(); r.first_sphere = r.first_square = r.first_cube = 0xFFFFFFFF
    assert gpu._L.trc_update_primitives(gpu._h, C.byref(r)) == abi.OK
    gpu.denoise()
    n2 = gpu.download_history_length()
    assert (n2 >= n).all() and (n2 > n).any()                                     # the history went on growing
    update(gpu, pr.motion(sc.view))                                              # a call that moves something drops it
    frame(gpu, 2, PATH)
    gpu.denoise()
    assert (gpu.download_history_length() == 1).all()
