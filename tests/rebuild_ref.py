"""The definitions of trc_rebuild_tree and trc_tree_cost (include/tracer_abi.h) restated in numpy, for tests/test_rebuild_cpu.py and
tests/test_gpu_rebuild_tree.py.  A tree is an (n, 16) uint32 array of trc_BVH records (refit_ref.raw), root at 0, leaves at 1..n_leaves.

leaf_records(tree)       the leaf records a rebuild of a device-built tree starts from: slots 1..n as they stand, links cleared
canonical_leaves(tree)   ... and of a caller's tree: by pType, then by pIndex; box from the record, padding lanes 0, everything else 0
tree_cost(tree)          the surface-area measure: per child slot h = ((double)dx*dy + (double)dy*dz) + (double)dz*dx of its box, d = max - min
                         in binary32 with a d that is not > 0 counted as 0; summed exactly (math.fsum) over interior and over leaf slots
expected_tree(leaves, sah)  the tree the definition names: host.build_tree (the SAH build) or the oracle's LBVH over those leaf records

TWIST is the deformation of the cost tests, chosen on the CPU (tests/test_rebuild_cpu.py asserts what makes it a sound input): a twist of
the ball by more than a full turn, which no refit undoes."""
import math

import numpy as np

import refit_ref as rr
from oracle import pyoracle
from tracer_amd import abi

F = np.float32
PARENT, LEFT, RIGHT, AXIS, PTYPE, PINDEX = rr.PARENT, rr.LEFT, rr.RIGHT, rr.AXIS, rr.PTYPE, rr.PINDEX
TWIST = (7.0, 1.1)          # (angle, scale) of refit_ref.twist


def n_leaves_of(tree):
    return (len(tree) + 1) // 2


def leaf_records(tree):
    """(n_leaves, 16) uint32: slots 1..n of the tree with parent / left / right cleared (what an upload clears too)"""
    out = tree[1:n_leaves_of(tree) + 1].copy()
    out[:, [PARENT, LEFT, RIGHT]] = 0
    return out


def canonical_leaves(tree):
    """(n_leaves, 16) uint32: the leaves of any tree (wherever they are in the array) ordered by pType, then by pIndex"""
    leaves = tree[tree[:, PTYPE] != np.uint32(abi.PRIM_BVH & 0xFFFFFFFF)]
    order = np.lexsort((leaves[:, PINDEX], leaves[:, PTYPE]))
    out = np.zeros((len(leaves), 16), np.uint32)
    out[:, PTYPE] = leaves[order, PTYPE]; out[:, PINDEX] = leaves[order, PINDEX]
    out[:, rr.MINI] = leaves[order, rr.MINI]; out[:, rr.MAXI] = leaves[order, rr.MAXI]
    return out


def expected_tree(leaves, sah):
    """(2n-1, 16) uint32 records of the tree over (n, 16) leaf records: trc_host_build_tree, or the oracle's LBVH"""
    from tracer_amd import host
    arr = rr.as_nodes(leaves)
    if sah:
        return rr.raw(host.build_tree(list(arr)))
    nodes, _ = pyoracle.lbvh_build(arr, len(leaves))
    return rr.raw(nodes)


def tree_height(tree):
    """depth of the deepest leaf"""
    depth, deepest, stack = {0: 0}, 0, [0]
    while stack:
        i = stack.pop()
        for c in (int(tree[i, LEFT]), int(tree[i, RIGHT])):
            depth[c] = depth[i] + 1
            if tree[c, PTYPE] == np.uint32(abi.PRIM_BVH & 0xFFFFFFFF):
                stack.append(c)
            else:
                deepest = max(deepest, depth[c])
    return deepest


def half_areas(tree, rows):
    """binary64 half areas of the boxes of records `rows`"""
    box = tree.view(F)
    d = box[rows][:, rr.MAXI] - box[rows][:, rr.MINI]              # binary32
    d = np.where(d > 0, d, F(0)).astype(np.float64)
    return (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]


def tree_cost(tree):
    """dict: root, interior, leaf (exact sums, rounded once), n_interior, n_leaves, and the per-slot terms behind the two sums"""
    is_interior = tree[:, PTYPE] == np.uint32(abi.PRIM_BVH & 0xFFFFFFFF)
    parents = np.nonzero(is_interior)[0]
    slots = np.concatenate([tree[parents, LEFT], tree[parents, RIGHT]]).astype(np.int64)
    h = half_areas(tree, slots)
    inner = is_interior[slots]
    return dict(root=float(half_areas(tree, np.array([0]))[0]), interior=math.fsum(h[inner]), leaf=math.fsum(h[~inner]),
                n_interior=int(inner.sum()), n_leaves=int((~inner).sum()), interior_terms=h[inner], leaf_terms=h[~inner])


def ratio(cost):
    """(interior + leaf) / root of a tree_cost dict or an abi.TreeCost"""
    if isinstance(cost, dict):
        return (cost["interior"] + cost["leaf"]) / cost["root"]
    return (cost.interior_half_area + cost.leaf_half_area) / cost.root_half_area
