"""trc_update_vertices on the CPU: the ABI names it, and its definition (tests/refit_ref.py) is well defined -- a tree of the host
builder refitted with UNCHANGED vertices is that tree again, bit for bit, so the oracle can render through a refitted tree as through
any other."""
import numpy as np
import pytest

import refit_ref as rr
from oracle import pyoracle
from conftest import random_rays
from tracer_amd import abi, host


def test_abi_names_update_vertices():
    assert abi.TRC_ABI_VERSION == 13
    assert "trc_update_vertices" in abi.DEVICE_SYMBOLS


def scenes():
    return {"ball": lambda: host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(50, 50, 0.08)),
            "small_ball": lambda: host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1)),
            "teapot": lambda: host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden("teapot"))}


@pytest.mark.parametrize("name", sorted(scenes()))
def test_refit_of_unchanged_vertices_is_the_host_tree(name):
    sc = scenes()[name]()
    nodes = sc.bvh_array().copy()
    got = rr.refit(nodes, rr.vertices_of(sc.view), rr.indices_of(sc.view))
    bad = np.nonzero((got != nodes).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(nodes)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {nodes[bad[0]]}"


def test_refitted_tree_bounds_the_moved_mesh():
    """after a twist the oracle finds through the refitted tree what it finds without any tree"""
    sc = scenes()["small_ball"]()
    v = rr.twist(rr.vertices_of(sc.view), 0.6)
    moved = rr.Moved(sc.view, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view)), v)
    rays = random_rays(3000, 5, inside_only=True)
    a, b = pyoracle.trace_rays(moved.view, rays), pyoracle.trace_rays(moved.view, rays, brute=True)
    for f in ("hit", "pType", "pIndex", "t"):
        assert (a[f].view(np.uint32) == b[f].view(np.uint32)).all(), f
    assert (a["pType"][a["hit"] != 0] == abi.PRIM_TRIANGLE).any()
