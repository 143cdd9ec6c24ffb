"""tests/visibility_ref.py against the host builder and the oracle: the inputs the GPU tests of trc_set_triangle_visibility
(tests/test_gpu_triangle_visibility.py) rely on are sound -- all of it on the CPU.  With every second triangle hidden and with all of them
hidden the host's SAH build and the oracle's LBVH take the subset leaf list, the oracle renders a view whose tree omits triangles, the
frames of "all", "half" and "none" differ pairwise, and the trees have other heights (so the LDS plan has to follow)."""
import numpy as np
import pytest

import rebuild_ref as rb
import refit_ref as rr
import visibility_ref as vr
from oracle import pyoracle
from tracer_amd import abi, host

W, H = 48, 32
_SCENES = {}
# tracePath at 2 spp, seed 9: the oracle's ray counts, and for 'lds' the accumulator sums (binary64 sum of the RGBA32F plane)
RAYS = {("lds", "all"): 5640, ("lds", "half"): 5511, ("lds", "none"): 5318, ("mem", "all"): 5698, ("mem", "half"): 5517, ("mem", "none"): 5318}
SUMS = {"all": 1690.11, "half": 1693.69, "none": 1700.08}
HEIGHTS = {"all": (9, 12), "half": (8, 9), "none": (4, 4)}      # 'lds': (SAH, LBVH)


def scene(residence):
    """the two residences of tests/test_gpu_update_vertices.py (not imported from there: that module is marked gpu as a whole)"""
    if residence not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.ball(50, 50, 0.08)
        _SCENES[residence] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
    return _SCENES[residence]


def masks(n_tri):
    return {"all": np.ones(n_tri, np.uint8), "half": (np.arange(n_tri) % 2 == 0).astype(np.uint8), "none": np.zeros(n_tri, np.uint8)}


def trees(residence, sah):
    sc = scene(residence)
    tree, v, idx = sc.bvh_array().copy(), rr.vertices_of(sc.view), rr.indices_of(sc.view)
    out = {}
    for name, mask in masks(len(idx) // 3).items():
        leaves = vr.leaf_list(tree, False, v, idx, mask)
        out[name] = (leaves, rb.expected_tree(leaves, sah))
    return out


def oracle_frame(view):
    rng = host.fill_rng(9, W, H)
    acc, st = pyoracle.render(view, host.prepare_camera(W, H), W, H, rng, spp=2, integrator=abi.INTEGRATOR_PATH)
    return acc, st.rays


def test_ranges_and_masks():
    m = vr.apply_ranges(np.ones(10, np.uint8), [(2, 5, 0), (4, 2, 1), (9, 1, 0), (0, 0, 0)])
    assert m.tolist() == [1, 1, 0, 0, 1, 1, 0, 1, 1, 0]                                   # the later range wins
    assert np.array_equal(vr.apply_ranges(np.ones(10, np.uint8), vr.ranges_of(np.ones(10, np.uint8), m)), m)
    sc = scene("lds")
    n_tri = sc.view.n_index // 3
    assert vr.implicit_mask(sc.bvh_array().copy(), n_tri).all()                           # the host tree names every triangle once


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_the_full_list_of_a_host_tree_is_its_canonical_list(residence):
    """the box rule: trc_host_build_node of a triangle's vertices is what the scene builder put into the tree"""
    sc = scene(residence)
    tree = sc.bvh_array().copy()
    n_tri = sc.view.n_index // 3
    full = vr.leaf_list(tree, False, rr.vertices_of(sc.view), rr.indices_of(sc.view), np.ones(n_tri, np.uint8))
    assert np.array_equal(full, rb.canonical_leaves(tree))


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_subset_trees_build_render_and_differ(residence):
    sc = scene(residence)
    n_tri = sc.view.n_index // 3
    v = rr.vertices_of(sc.view)
    frames = {}
    by_flavour = {sah: trees(residence, sah) for sah in (True, False)}
    for name in ("all", "half", "none"):
        per_flavour = []
        for sah in (True, False):
            leaves, tree = by_flavour[sah][name]
            n = len(leaves)
            assert n == (n_tri, (n_tri + 1) // 2, 0)[("all", "half", "none").index(name)] + (leaves[:, rr.PTYPE] != abi.PRIM_TRIANGLE).sum()
            assert len(tree) == 2 * n - 1 and np.array_equal(rb.canonical_leaves(tree), leaves)      # a tree over exactly those leaves
            acc, rays = oracle_frame(rr.Moved(sc.view, tree, v).view)
            per_flavour.append((acc, rays))
            print(f"{residence} {name} {'sah' if sah else 'lbvh'}: {n} leaves, height {rb.tree_height(tree)}, {rays} rays, sum {acc.astype(np.float64).sum():.2f}")
        assert per_flavour[0][1] == per_flavour[1][1] and np.array_equal(per_flavour[0][0].view(np.uint32), per_flavour[1][0].view(np.uint32))
        frames[name] = per_flavour[0]
        assert frames[name][1] == RAYS[(residence, name)]
        if residence == "lds":
            assert abs(float(frames[name][0].astype(np.float64).sum()) - SUMS[name]) < 0.006
    for a, b in (("all", "half"), ("all", "none"), ("half", "none")):
        assert not np.array_equal(frames[a][0].view(np.uint32), frames[b][0].view(np.uint32)), (a, b)


def test_subset_trees_have_other_heights():
    for k, sah in enumerate((True, False)):
        got = {name: rb.tree_height(tree) for name, (_, tree) in trees("lds", sah).items()}
        assert got == {name: h[k] for name, h in HEIGHTS.items()}, (sah, got)
