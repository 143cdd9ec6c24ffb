"""The definition of trc_set_triangle_visibility (include/tracer_abi.h) restated in numpy, for tests/test_visibility_cpu.py and
tests/test_gpu_triangle_visibility.py.  A tree is an (n, 16) uint32 array of trc_BVH records (refit_ref.raw).

apply_ranges(mask, ranges)   the ranges in the order given, a later one wins
implicit_mask(tree, n_tri)   the mask before the first call: a triangle is visible iff a leaf of the tree names it
leaf_list(tree_before, device_built, vertices, indices, mask)
                             the analytic leaves a rebuild would start from (rebuild_ref.leaf_records of a device-built tree,
                             rebuild_ref.canonical_leaves of a caller's), filtered to pType != triangle, in that order, with the boxes they
                             hold; then one record per visible triangle, ascending: pType triangle, pIndex t, the box
                             refit_ref.triangle_leaf_box of its three current vertices, everything else 0
The tree over that list is rebuild_ref.expected_tree's."""
import numpy as np

import rebuild_ref as rb
import refit_ref as rr
from tracer_amd import abi

F = np.float32


def apply_ranges(mask, ranges):
    out = np.asarray(mask, dtype=np.uint8).copy()
    for first, count, visible in ranges:
        assert visible in (0, 1) and first + count <= len(out)
        out[first:first + count] = visible
    return out


def implicit_mask(tree, n_tri):
    mask = np.zeros(n_tri, np.uint8)
    named = tree[tree[:, rr.PTYPE] == abi.PRIM_TRIANGLE][:, rr.PINDEX]
    assert len(np.unique(named)) == len(named), "a triangle named by two leaves has no mask"
    mask[named] = 1
    return mask


def ranges_of(mask_before, mask_after):
    """maximal runs of triangles whose bit changes, as (first, count, visible) triples"""
    out, t, n = [], 0, len(mask_after)
    changed = np.asarray(mask_before) != np.asarray(mask_after)
    while t < n:
        if not changed[t]:
            t += 1
            continue
        e = t
        while e < n and changed[e] and mask_after[e] == mask_after[t]:
            e += 1
        out.append((t, e - t, int(mask_after[t])))
        t = e
    return out


def leaf_list(tree_before, device_built, vertices, indices, mask):
    src = rb.leaf_records(tree_before) if device_built else rb.canonical_leaves(tree_before)
    analytic = src[src[:, rr.PTYPE] != abi.PRIM_TRIANGLE]
    visible = np.nonzero(np.asarray(mask))[0]
    tri = np.zeros((len(visible), 16), np.uint32)
    pos = np.ascontiguousarray(vertices, dtype=F)[:, :3]
    corners = np.asarray(indices, dtype=np.uint32).reshape(-1, 3)
    box = tri.view(F)
    for k, t in enumerate(visible):
        lo, hi = rr.triangle_leaf_box(pos[corners[t]])
        box[k, rr.MINI] = lo; box[k, rr.MAXI] = hi
    tri[:, rr.PTYPE] = abi.PRIM_TRIANGLE; tri[:, rr.PINDEX] = visible
    return np.concatenate([analytic, tri])
