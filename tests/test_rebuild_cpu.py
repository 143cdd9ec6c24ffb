"""tests/rebuild_ref.py against the host builder and the oracle: the canonical leaf order, the counts of the cost, and the inputs the GPU
tests of trc_rebuild_tree / trc_tree_cost (tests/test_gpu_rebuild_tree.py) rely on -- all of it on the CPU."""
import numpy as np
import pytest

import rebuild_ref as rb
import refit_ref as rr
from tracer_amd import abi, host

F = np.float32
_SCENES = {}


def scene(residence):
    """the two residences of tests/test_gpu_update_vertices.py (not imported from there: that module is marked gpu as a whole)"""
    if residence not in _SCENES:
        mesh = host.Mesh.ball(4, 6, 0.1) if residence == "lds" else host.Mesh.ball(50, 50, 0.08)
        _SCENES[residence] = host.HostScene(abi.SCENE_CORNELL_MESH, mesh)
    return _SCENES[residence]


def twisted(residence):
    """(vertices under rebuild_ref.TWIST, the host tree refitted to them)"""
    sc = scene(residence)
    v = rr.twist(rr.vertices_of(sc.view), *rb.TWIST)
    return v, rr.refit(sc.bvh_array().copy(), v, rr.indices_of(sc.view))


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_canonical_leaves_are_a_permutation_of_the_leaf_records(residence):
    sc = scene(residence)
    tree = sc.bvh_array().copy()
    n = sc.n_leaves
    leaves, canon = tree[1:n + 1], rb.canonical_leaves(tree)
    assert len(canon) == n == rb.n_leaves_of(tree)
    key = lambda a: a[:, rr.PTYPE].astype(np.int64) << 32 | a[:, rr.PINDEX]
    assert len(np.unique(key(leaves))) == n and (np.diff(key(canon)) > 0).all()          # every primitive once; sorted by type, then index
    by_key = {int(k): row for k, row in zip(key(leaves), leaves)}
    for k, row in zip(key(canon), canon):
        src = by_key[int(k)]
        assert np.array_equal(row[rr.MINI], src[rr.MINI]) and np.array_equal(row[rr.MAXI], src[rr.MAXI])      # bit-equal boxes
        assert not row[[0, 1, 2, 3, 6, 7, 11, 15]].any()                                  # links, axis and every padding lane are 0
    counts = [sc.view.n_sphere, sc.view.n_square, sc.view.n_cube, sc.view.n_index // 3]
    first = np.concatenate([[0], np.cumsum(counts)])
    slot = first[canon[:, rr.PTYPE]] + canon[:, rr.PINDEX]                                 # the device's sort key: first[pType] + pIndex
    assert (np.diff(slot) > 0).all() and slot[-1] < first[-1]
    # the tree over them is a tree over the same primitives
    built = rb.expected_tree(canon, True)
    assert np.array_equal(rb.canonical_leaves(built), canon)


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_cost_counts_and_terms(residence):
    tree = scene(residence).bvh_array().copy()
    n = rb.n_leaves_of(tree)
    c = rb.tree_cost(tree)
    assert (c["n_interior"], c["n_leaves"]) == (n - 2, n) and n - 2 == (len(tree) - n) - 1       # nodes - 1 interior slots
    assert len(c["interior_terms"]) == n - 2 and len(c["leaf_terms"]) == n
    assert (c["interior_terms"] >= 0).all() and (c["leaf_terms"] >= 0).all() and c["root"] > 0
    assert c["interior_terms"].max() <= c["root"]                                          # a child's box lies in the root's
    # a box that is flat or inverted along an axis counts that extent as 0
    flat = tree[:3].copy()
    b = flat.view(F)
    b[1, rr.MINI] = (0, 0, 0); b[1, rr.MAXI] = (2, 3, 0)
    b[2, rr.MINI] = (0, 0, 5); b[2, rr.MAXI] = (2, 3, 1)
    assert list(rb.half_areas(flat, np.array([1, 2]))) == [6.0, 6.0]


@pytest.mark.parametrize("residence", ["lds", "mem"])
def test_the_twist_of_the_cost_tests_degrades_a_refitted_tree(residence):
    """what tests/test_gpu_rebuild_tree.py asserts of the GPU's numbers holds for the definition's: after rebuild_ref.TWIST the refitted
    tree costs more than either rebuilt one, and both rebuilds change the topology"""
    v, refitted = twisted(residence)
    worn = rb.ratio(rb.tree_cost(refitted))
    assert worn > rb.ratio(rb.tree_cost(scene(residence).bvh_array().copy()))
    for sah in (True, False):
        rebuilt = rb.expected_tree(rb.leaf_records(refitted), sah)
        assert np.array_equal(rebuilt[1:rb.n_leaves_of(rebuilt) + 1, 4:], refitted[1:rb.n_leaves_of(refitted) + 1, 4:])      # the leaves stay
        assert worn > rb.ratio(rb.tree_cost(rebuilt)), sah
        assert (rebuilt[:, :8] != refitted[:, :8]).any()


def test_the_twist_changes_the_height_of_the_lds_tree():
    """the input of the GPU test that pins the LDS plan being made again"""
    _, refitted = twisted("lds")
    before = rb.tree_height(refitted)
    assert before == scene("lds").tree_depth()
    for sah in (True, False):
        assert rb.tree_height(rb.expected_tree(rb.leaf_records(refitted), sah)) != before, sah
