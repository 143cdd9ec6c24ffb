"""TRC_TREE_SAH3 on the GPU (include/tracer_abi.h): the device-built tree against trc_host_build_tree_flags record for record (which
tests/test_sah3_cpu.py holds to the header's text), frames through it against the CPU oracle, trc_rebuild_tree with the flag, refusals
that change nothing -- and TRC_TREE_SAH alone and the LBVH still what the oracle builds."""
import ctypes as C

import numpy as np
import pytest

import rebuild_ref as rb
import refit_ref as rr
import sah3_ref as s3
import skin_ref as sr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_pose_vertices import bits
from test_gpu_rebuild_tree import WithVertices, analytic, check_cost, move, rest_of, status_of
from test_gpu_skin_vertices import small_case
from test_gpu_update_vertices import DEVICE_TREE, MIS, PATH, first_difference, frame, oracle_frame, same, scene
from tracer_amd import abi, host
from tracer_amd.device import Tracer

pytestmark = pytest.mark.gpu
SAH, SAH3 = abi.TREE_SAH, abi.TREE_SAH | abi.TREE_SAH3
_SPHERES = []


def spheres():
    if not _SPHERES:
        _SPHERES.append(host.HostScene(abi.SCENE_CORNELL_SPHERES))
    return _SPHERES[0]


class Leaves:
    """the sphere scene's view over other leaf records (kept alive here); every record names one of the scene's spheres"""

    def __init__(self, records):
        sc = spheres()
        self.records = records.copy()
        self.records[:, rr.PTYPE] = abi.PRIM_SPHERE
        self.records[:, rr.PINDEX] = np.arange(len(records)) % sc.view.n_sphere
        self.nodes = rr.as_nodes(self.records)
        self.view = abi.Scene.from_buffer_copy(sc.leaves_view())
        self.view.bvhList = C.cast(self.nodes, C.POINTER(abi.BVH)); self.view.n_bvh = len(records)


def host_tree(records, flags=SAH3):
    return rr.raw(host.build_tree(list(rr.as_nodes(records)), flags))


def check_upload(gpu, records):
    l = Leaves(records)
    gpu.upload_scene_device(l.view, SAH3)
    got, want = rr.raw(gpu.download_bvh()), host_tree(l.records)
    assert not first_difference(got, want)
    n_nodes, height, ms = gpu.lbvh_info()
    assert n_nodes == 2 * len(records) - 1 and height == rb.tree_height(want) and ms > 0
    return got


# --------------------------------------------------------------------------------------------------- 1. the tree
@pytest.mark.parametrize("n", [2, 3, 64, 65, 66, 129, 2048, 2049, 4097, 70000])
def test_device_tree_is_the_host_builder_s_on_random_boxes(gpu, n):
    """<= 64: the finish kernel alone; 65, 66: one level, then finishes; 2048 / 2049: one and two tasks in the root; 70 000: levels of more
    than 64 rows (several wavefronts of the split kernel, several workgroups of the pricing) and nodes of many tasks"""
    check_upload(gpu, s3.families["random"](n, 3 * n + 1))


@pytest.mark.parametrize("n", [200, 3000])
@pytest.mark.parametrize("family", [f for f in s3.families if f not in ("random", "ball48")])
def test_device_tree_is_the_host_builder_s_on_awkward_leaf_sets(gpu, family, n):
    check_upload(gpu, s3.families[family](n, 7 * n))


def test_device_tree_of_the_ball_of_the_animation_tests(gpu):
    sc = scene("lds")
    gpu.upload_scene_device(sc.leaves_view(), SAH3)
    assert not first_difference(rr.raw(gpu.download_bvh()), host_tree(rb.leaf_records(sc.bvh_array().copy())))


@pytest.mark.parametrize("mesh", ["teapot", "coatball"])
def test_triangle_leaves_of_the_committed_meshes(gpu, mesh):
    m = host.Mesh.golden(mesh)
    full = host.HostScene(abi.SCENE_CORNELL_MESH, m)
    lean = host.HostScene(abi.SCENE_CORNELL_MESH, m, analytic_leaves_only=True)
    gpu.upload_scene_device(lean.view, SAH3 | abi.TREE_TRIANGLE_LEAVES)
    got, want = rr.raw(gpu.download_bvh()), host_tree(rb.leaf_records(full.bvh_array().copy()))
    assert not first_difference(got, want)
    assert rb.tree_cost(got)["interior"] < rb.tree_cost(full.bvh_array().copy())["interior"]


def test_without_the_flag_the_trees_are_the_oracle_s(gpu):
    """in one session, after a flagged build: TRC_TREE_SAH alone and the LBVH"""
    sc = scene("mem")
    n = sc.n_leaves
    gpu.upload_scene_device(sc.leaves_view(), SAH3)
    flagged = rr.raw(gpu.download_bvh())
    gpu.upload_scene_device(sc.leaves_view(), SAH)
    plain = rr.raw(gpu.download_bvh())
    assert not first_difference(plain, rr.raw(pyoracle.sah_build(sc.leaves(), n)))
    assert (flagged[:, :8] != plain[:, :8]).any()
    gpu.upload_scene_device(sc.leaves_view(), 0)
    nodes, _ = pyoracle.lbvh_build(sc.leaves(), n)
    assert not first_difference(rr.raw(gpu.download_bvh()), rr.raw(nodes))


# --------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("integrator", [PATH, MIS], ids=["path", "mis"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_frames_through_the_flagged_tree_are_the_oracle_s(gpu, residence, integrator):
    sc = scene(residence)
    gpu.upload_scene_device(analytic(residence).view, SAH3 | abi.TREE_TRIANGLE_LEAVES)
    tree = rr.raw(gpu.download_bvh())
    assert not first_difference(tree, host_tree(rb.leaf_records(sc.bvh_array().copy())))
    m = rr.Moved(sc.view, tree, rr.vertices_of(sc.view))
    assert same(frame(gpu, 4, integrator), oracle_frame(m.view, 4, integrator))
    if residence == "mem":
        assert (tree[:, :8] != sc.bvh_array()[:, :8]).any()                              # not the reference's tree


# --------------------------------------------------------------------------------------------------- 3. rebuild
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_flagged_rebuild_is_a_fresh_flagged_upload_and_keeps_what_a_rebuild_keeps(gpu, residence):
    sc = scene(residence)
    n = sc.view.n_index // 3
    tri_mat = np.where(np.arange(n) % 3 == 0, 4, 19).astype(np.uint32)
    gpu.upload_scene_device(analytic(residence).view, DEVICE_TREE | abi.TREE_SAH3)
    gpu.upload_triangle_materials(tri_mat)
    v = move(gpu, residence)                                                             # an update, then a skin over the ragged binding
    before = rr.raw(gpu.download_bvh())
    gpu.rebuild_tree(SAH3)
    got = rr.raw(gpu.download_bvh())
    assert np.array_equal(bits(gpu.download_vertices()), bits(v))
    with Tracer(0) as fresh:
        m = WithVertices(analytic(residence).view, v)
        fresh.upload_scene_device(m.view, DEVICE_TREE | abi.TREE_SAH3)
        assert not first_difference(got, rr.raw(fresh.download_bvh()))
        assert fresh.lbvh_info()[:2] == gpu.lbvh_info()[:2]
    assert not first_difference(got, host_tree(rb.leaf_records(before)))
    assert (got[:, :8] != before[:, :8]).any()
    check_cost(gpu.tree_cost(), got, "rebuilt sah3")
    # the triangle materials
    hits = gpu.trace_rays(random_rays(4000, 4, inside_only=True))
    tri = (hits["hit"] != 0) & (hits["pType"] == abi.PRIM_TRIANGLE)
    assert tri.any() and (hits["material"][tri] == tri_mat[hits["pIndex"][tri]]).all()
    mv = rr.Moved(sc.view, got, v)
    with Tracer(0) as fresh:
        fresh.upload_scene(mv.view); fresh.upload_triangle_materials(tri_mat)
        assert same(frame(fresh, 4, MIS), frame(gpu, 4, MIS))
    # the binding and the rest copy: another palette skins from the same rest
    first, b, w, palette = small_case(residence)
    v1 = rr.twist(rest_of(residence), *rb.TWIST)
    other = palette[::-1].copy()
    gpu.skin_vertices(other)
    want_v = sr.skin(v1, v, first, b, w, other)
    assert np.array_equal(bits(gpu.download_vertices()), bits(want_v))
    assert not first_difference(rr.raw(gpu.download_bvh()), rr.refit(got, want_v, rr.indices_of(sc.view)))
    gpu.upload_triangle_materials(None)


# --------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_change_nothing(gpu):
    gpu.upload_scene_device(analytic("lds").view, DEVICE_TREE | abi.TREE_SAH3)
    tree, before = rr.raw(gpu.download_bvh()), frame(gpu, 4, MIS)
    for flags in (abi.TREE_SAH3, abi.TREE_SAH3 | abi.TREE_TRIANGLE_LEAVES):
        assert status_of(lambda: gpu.rebuild_tree(flags)) == abi.ERR_INVALID_ARG, flags
        assert same(frame(gpu, 4, MIS), before) and not first_difference(rr.raw(gpu.download_bvh()), tree)
        assert status_of(lambda: gpu.upload_scene_device(analytic("lds").view, flags)) == abi.ERR_INVALID_ARG, flags
        assert same(frame(gpu, 4, MIS), before) and not first_difference(rr.raw(gpu.download_bvh()), tree)
    # a leaf box that is not finite: found by the build's intake, before any tree is written.  An upload has let the context's old scene
    # go by then (as documented for every device build), so it runs in a context of its own; this one renders what it rendered
    for bad in (np.inf, np.nan, 2e37):
        records = s3.families["random"](300, 1)
        records.view(np.float32)[123, 13] = bad
        with Tracer(0) as other:
            assert status_of(lambda: other.upload_scene_device(Leaves(records).view, SAH3)) == abi.ERR_BVH_INVALID, bad
    assert same(frame(gpu, 4, MIS), before) and not first_difference(rr.raw(gpu.download_bvh()), tree)
