"""trc_host_build_tree_flags (include/tracer_abi.h) on the CPU: TRC_TREE_SAH is trc_host_build_tree, TRC_TREE_SAH | TRC_TREE_SAH3 is the
definition of the header as tests/sah3_ref.py restates it, record for record; the flagged tree of the committed meshes costs less."""
import ctypes as C

import numpy as np
import pytest

import rebuild_ref as rb
import refit_ref as rr
import sah3_ref as s3
from tracer_amd import abi, host

SAH, SAH3 = abi.TREE_SAH, abi.TREE_SAH | abi.TREE_SAH3
SIZES = (2, 3, 4, 5, 64, 65, 200, 3000)
FAMILY_SIZES = (200, 3000)
BVH = np.uint32(abi.PRIM_BVH)


def built(leaves, flags):
    return rr.raw(host.build_tree(list(rr.as_nodes(leaves)), flags))


def depth_of(tree):
    d = C.c_uint32()
    status = host.lib().trc_host_tree_depth(rr.as_nodes(tree), len(tree), C.byref(d))
    assert status == 0
    return d.value


def check(leaves):
    got, want = built(leaves, SAH3), s3.expected_tree(leaves)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f"{len(bad)} of {len(want)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    assert depth_of(got) <= abi.TRC_MAX_BVH_DEPTH
    return got


@pytest.mark.parametrize("n", SIZES)
def test_sah_flag_alone_is_trc_host_build_tree(n):
    leaves = s3.families["random"](n, 100 + n)
    assert np.array_equal(built(leaves, SAH), built(leaves, None))


@pytest.mark.parametrize("n", SIZES)
def test_flagged_tree_is_the_definition_s_on_random_boxes(n):
    tree = check(s3.families["random"](n, n))
    if n >= 64:
        assert (tree[tree[:, rr.PTYPE] == BVH][:, rr.AXIS] == 0).any() and (tree[tree[:, rr.PTYPE] == BVH][:, rr.AXIS] == 1).any()      # not one axis only


@pytest.mark.parametrize("n", FAMILY_SIZES)
@pytest.mark.parametrize("family", [f for f in s3.families if f not in ("random", "ball48")])
def test_flagged_tree_is_the_definition_s_on_awkward_leaf_sets(family, n):
    leaves = s3.families[family](n, 7 * n)
    tree = check(leaves)
    interior_axes = tree[tree[:, rr.PTYPE] == BVH][:, rr.AXIS]
    wide = np.array([i for i in np.nonzero(tree[:, rr.PTYPE] == BVH)[0] if _n_leaves_below(tree, i) >= 3])
    if family == "lattice":
        assert tree[0, rr.AXIS] == 0                                                 # the three axes tie at the root: the lowest wins
        assert set(interior_axes) == {0, 1, 2}
    if family.startswith("line_"):
        assert (tree[wide, rr.AXIS] == "xyz".index(family[-1])).all()                # the two other axes have no extent: skipped
    if family == "coplanar":
        assert (tree[wide, rr.AXIS] != 1).all()
    if family == "identical":
        assert (tree[wide, rr.AXIS] == 2).all()                                       # the fallback: axis 2, median, order kept
        assert tree[0, rr.LEFT] != tree[0, rr.RIGHT]
    if family == "huge":
        assert np.isfinite(tree.view(np.float32)[:, 8:15]).all() and np.abs(tree.view(np.float32)[0, 8:15]).max() == np.float32(1e37)
        assert _n_leaves_below(tree, int(tree[0, rr.LEFT])) == 1 and tree[0, rr.AXIS] == 0      # infinite costs: the first candidate, bin 0 of x


def _n_leaves_below(tree, i):
    if tree[i, rr.PTYPE] != BVH:
        return 1
    return _n_leaves_below(tree, int(tree[i, rr.LEFT])) + _n_leaves_below(tree, int(tree[i, rr.RIGHT]))


def test_identical_centroids_keep_the_input_order():
    tree = built(s3.families["identical"](8, 1), SAH3)

    def order(i):
        return [i] if tree[i, rr.PTYPE] != BVH else order(int(tree[i, rr.LEFT])) + order(int(tree[i, rr.RIGHT]))
    # spans 8 -> 4 + 4 -> 2 + 2: the pairs are ordered by the two-leaf rule (equal centroids: the second goes left)
    assert order(0) == [2, 1, 4, 3, 6, 5, 8, 7]


def test_flagged_tree_is_the_definition_s_on_the_ball_of_the_animation_tests():
    leaves = s3.families["ball48"](0, 0)
    assert (leaves[:, rr.PTYPE] == abi.PRIM_TRIANGLE).sum() == 48
    check(leaves)


@pytest.mark.parametrize("mesh", ["teapot", "coatball"])
def test_flagged_tree_of_the_committed_meshes_costs_less(mesh):
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.golden(mesh))
    leaves = rb.leaf_records(sc.bvh_array().copy())
    plain, flagged = built(leaves, SAH), built(leaves, SAH3)
    assert np.array_equal(plain, sc.bvh_array())
    assert depth_of(flagged) <= abi.TRC_MAX_BVH_DEPTH
    a, b = rb.tree_cost(plain), rb.tree_cost(flagged)
    print(f"{mesh}: interior / root {a['interior'] / a['root']:.3f} -> {b['interior'] / b['root']:.3f}, depth {depth_of(plain)} -> {depth_of(flagged)}")
    assert b["interior"] < a["interior"]
    assert np.array_equal(flagged[1:len(leaves) + 1, 4:], plain[1:len(leaves) + 1, 4:])          # the same leaves in the same slots


@pytest.mark.parametrize("flags", [0, abi.TREE_SAH3, 4, 8, abi.TREE_TRIANGLE_LEAVES, SAH3 | abi.TREE_TRIANGLE_LEAVES])
def test_other_flags_are_refused_and_touch_nothing(flags):
    leaves = s3.families["random"](5, 5)
    nodes = (abi.BVH * 9)()
    for i, leaf in enumerate(rr.as_nodes(leaves)):
        nodes[i] = leaf
    before = bytes(memoryview(nodes))
    count = C.c_uint32(77)
    assert host.lib().trc_host_build_tree_flags(nodes, 5, flags, C.byref(count)) == abi.ERR_INVALID_ARG
    assert bytes(memoryview(nodes)) == before and count.value == 77
