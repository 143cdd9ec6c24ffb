"""trc_update_vertices, the refit variants side by side: one launch per depth of the tree (the default) and one launch with an arrival
counter per node (knob refit_single) give the bits of the definition (tests/refit_ref.py).  Every case updates twice and more, so a
counter that the single launch did not put back to zero shows in the second result.  And the angle nobody moves by: unchanged vertices
leave a device-built tree as the upload made it, which ties the refit's leaf box (dev_trileaf.hpp) to the upload kernel's."""
import numpy as np
import pytest

import refit_ref as rr
from conftest import random_rays
from oracle import pyoracle
from test_gpu_update_vertices import DEVICE_TREE, PATH, first_difference, frame, moved, oracle_frame, same, scene
from tracer_amd.device import Tracer

pytestmark = pytest.mark.gpu
ANGLES = (0.5, -1.2, 0.3)


@pytest.fixture(params=[0, 1], ids=["per_depth", "single_launch"])
def tracer(request):
    with Tracer(0) as t:
        t.debug_set("refit_single", request.param)
        yield t


def upload_device_tree(t, residence, tree):
    if tree == "lbvh":
        t.upload_scene_lbvh(scene(residence).leaves_view())
    else:
        t.upload_scene_device(scene(residence, analytic_leaves_only=True).view, DEVICE_TREE)


@pytest.mark.parametrize("tree", ["sah_triangle_leaves", "lbvh"])
@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_downloaded_tree_after_successive_updates(tracer, residence, tree):
    sc = scene(residence)
    upload_device_tree(tracer, residence, tree)
    before = rr.raw(tracer.download_bvh())
    idx = rr.indices_of(sc.view)
    for angle in ANGLES:
        v = rr.twist(rr.vertices_of(sc.view), angle)
        tracer.update_vertices(v)
        got = rr.raw(tracer.download_bvh())
        assert not first_difference(got, rr.refit(before, v, idx)), angle
    assert (got[:, :8] == before[:, :8]).all()


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_unchanged_vertices_leave_a_device_tree_as_it_was(tracer, residence):
    """TRC_TREE_TRIANGLE_LEAVES: the upload wrote every triangle leaf's box and the unions above; the refit writes the same bits"""
    sc = scene(residence)
    upload_device_tree(tracer, residence, "sah_triangle_leaves")
    before = rr.raw(tracer.download_bvh())
    v0 = rr.vertices_of(sc.view)
    tracer.update_vertices(v0)
    got = rr.raw(tracer.download_bvh())
    box = np.r_[8:11, 12:15]                                          # the padding lanes are the upload's own
    assert not first_difference(got[:, box], before[:, box])
    assert (got[:, :8] == before[:, :8]).all()
    assert not first_difference(got, rr.refit(before, v0, rr.indices_of(sc.view)))


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_host_tree_walk_after_successive_updates(tracer, residence):
    """the instrumented walk's counters depend on every box of a tree that cannot be downloaded"""
    tracer.upload_scene(scene(residence).view)
    rays = random_rays(4000, 5, inside_only=True)
    for angle in ANGLES:
        v, m = moved(residence, angle)
        tracer.update_vertices(v)
        got, ref = tracer.trace_rays(rays), pyoracle.trace_rays(m.view, rays)
        for f in ref.dtype.names:
            assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), (angle, f)
    assert ref["n_descend"].sum() > 0


def test_single_launch_frame_is_the_oracle_s(tracer):
    v, m = moved("mem", 0.7)
    tracer.upload_scene(scene("mem").view)
    tracer.update_vertices(rr.twist(v, 0.2))                         # one update before the one that is looked at
    tracer.update_vertices(v)
    assert same(frame(tracer, 4, PATH), oracle_frame(m.view, 4, PATH))
