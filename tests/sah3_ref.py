"""The definition of TRC_TREE_SAH3 (include/tracer_abi.h, at trc_upload_scene_device) restated in numpy from the header's text, for
tests/test_sah3_cpu.py: explicit binary32 operations in the order the header writes them, the two-ended swap loop for the partition,
serial post-order numbering.  A tree is an (2n-1, 16) uint32 array of trc_BVH records like rebuild_ref.expected_tree's.

expected_tree(leaves)   the tree over (n, 16) uint32 leaf records
families                the leaf sets of the CPU and GPU tests: name -> function(n, seed) -> (m, 16) uint32 leaf records, m near n

Slow (Python per node): meant for a few thousand leaves.  min / max and counts are order-free, so the unions of the 31 splits of an axis
come from per-bin boxes and running min / max; every cost is priced by the expression of the header, one float32 operation at a time."""
import sys

import numpy as np

import refit_ref as rr
from tracer_amd import abi

F = np.float32
PARENT, LEFT, RIGHT, AXIS, PTYPE, PINDEX = rr.PARENT, rr.LEFT, rr.RIGHT, rr.AXIS, rr.PTYPE, rr.PINDEX
BINS = 32


def centroids(mn, mx):
    return (mn + (mx - mn) / F(2)).astype(F)


def area(mn, mx):
    """A(B) = 2 * ((dx * dy + dx * dz) + dy * dz), d = max - min; mn, mx: (..., 3) float32"""
    d = (mx - mn).astype(F)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return F(2) * ((dx * dy + dx * dz) + dy * dz)


def bins_of(c, lo, e):
    rel = ((c - lo) / e).astype(F)
    fb = (F(BINS) * rel).astype(F)
    b = np.where(fb >= 0, fb, F(0)).astype(np.uint32)
    return np.minimum(b, np.uint32(BINS - 1))


def partition(order, below):
    """the two-ended swap loop (BVH.hh:154-168) over the list `order` with the predicate below[k] of its k-th entry; returns the split"""
    order = list(order); below = list(below)
    first, last = 0, len(order)
    while True:
        while True:
            if first == last:
                return order, first
            if below[first]:
                first += 1
            else:
                break
        last -= 1
        while True:
            if first == last:
                return order, first
            if not below[last]:
                last -= 1
            else:
                break
        order[first], order[last] = order[last], order[first]
        below[first], below[last] = below[last], below[first]
        first += 1


def split(c, mn, mx):
    """records (k >= 3) by centroid c and box mn, mx (each (k, 3) float32) -> (axis, below mask) of the winning candidate, or None when no
    axis has a positive extent"""
    best = None
    cb_lo, cb_hi = c.min(axis=0), c.max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            lo = cb_lo[a]; e = F(cb_hi[a] - lo)
            if not e > 0:
                continue
            b = bins_of(c[:, a], lo, e)
            count = np.bincount(b, minlength=BINS)
            bmn = np.full((BINS, 3), np.inf, F); bmx = np.full((BINS, 3), -np.inf, F)
            np.minimum.at(bmn, b, mn); np.maximum.at(bmx, b, mx)
            n0 = np.cumsum(count)[:-1]; n1 = len(c) - n0                                          # i = 0..30: bins <= i | the rest
            mn0 = np.minimum.accumulate(bmn, axis=0)[:-1]; mx0 = np.maximum.accumulate(bmx, axis=0)[:-1]
            mn1 = np.minimum.accumulate(bmn[::-1], axis=0)[::-1][1:]; mx1 = np.maximum.accumulate(bmx[::-1], axis=0)[::-1][1:]
            cost = n0.astype(F) * area(mn0, mx0) + n1.astype(F) * area(mn1, mx1)
            for i in range(BINS - 1):
                if n0[i] == 0 or n1[i] == 0:
                    continue
                if best is None or cost[i] < best[0]:
                    best = (cost[i], a, b <= i)
    return None if best is None else (best[1], best[2])


def expected_tree(leaves):
    n = len(leaves)
    assert n >= 2
    out = np.zeros((2 * n - 1, 16), np.uint32)
    out[1:n + 1] = leaves
    out[1:n + 1, [PARENT, LEFT, RIGHT]] = 0
    box = out.view(F)
    cen = centroids(box[:, rr.MINI], box[:, rr.MAXI])
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 100))

    def build(slots, base, is_root):
        span = len(slots)
        if span == 1:
            return slots[0]
        if span == 2:
            a, b = slots
            d = np.maximum(cen[a], cen[b]) - np.minimum(cen[a], cen[b])
            axis = 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)
            left, right = (a, b) if cen[a, axis] < cen[b, axis] else (b, a)
        else:
            s = np.array(slots)
            won = split(cen[s], box[s][:, rr.MINI], box[s][:, rr.MAXI])
            if won is None:
                axis, mid = 2, span // 2
            else:
                axis, below = won
                slots, mid = partition(slots, below)
            left = build(slots[:mid], base, False)
            right = build(slots[mid:], base + mid - 1, False)
        me = 0 if is_root else base + span - 2
        out[me, [PARENT, LEFT, RIGHT, AXIS, PTYPE, PINDEX]] = (0, left, right, axis, abi.PRIM_BVH, 0)
        l, r = box[left], box[right]                                                              # where two bounds compare equal the right child's is kept
        box[me, rr.MINI] = np.where(l[rr.MINI] < r[rr.MINI], l[rr.MINI], r[rr.MINI])
        box[me, rr.MAXI] = np.where(l[rr.MAXI] > r[rr.MAXI], l[rr.MAXI], r[rr.MAXI])
        out[left, PARENT] = me; out[right, PARENT] = me
        return me

    try:
        build(list(range(1, n + 1)), n + 1, True)
    finally:
        sys.setrecursionlimit(limit)
    return out


# ---------------------------------------------------------------------------------------------------------------- leaf sets
def records(mn, mx):
    """(n, 3) corners -> (n, 16) uint32 leaf records: triangles 0..n-1 (the type only has to be a leaf's)"""
    n = len(mn)
    out = np.zeros((n, 16), np.uint32)
    out[:, PTYPE] = abi.PRIM_TRIANGLE; out[:, PINDEX] = np.arange(n)
    out.view(F)[:, rr.MINI] = np.asarray(mn, F); out.view(F)[:, rr.MAXI] = np.asarray(mx, F)
    return out


def _random(n, seed):
    r = np.random.default_rng(seed)
    c = r.uniform(-100, 100, (n, 3)); h = r.uniform(0.01, 4, (n, 3))
    return records(c - h, c + h)


def _lattice(n, seed):
    k = max(2, round(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F)
    return records(g, g + F(0.5))


def _line(axis):
    def make(n, seed):
        r = np.random.default_rng(seed)
        c = np.zeros((n, 3)); c[:, axis] = r.uniform(-50, 50, n); c[:, (axis + 1) % 3] = 3.0
        h = r.integers(2, 9, (n, 1)) / 4.0 * np.ones(3)                                           # cubes of quarter sizes: mn + (mx - mn) / 2 is exact off the axis
        return records(c - h, c + h)
    return make


def _coplanar(n, seed):
    r = np.random.default_rng(seed)
    c = r.uniform(-50, 50, (n, 3)); c[:, 1] = 7.0
    h = r.integers(2, 9, (n, 1)) / 4.0 * np.ones(3)
    return records(c - h, c + h)


def _identical(n, seed):
    r = np.random.default_rng(seed)
    h = r.integers(1, 9, (n, 3)).astype(np.float64)                                               # integers: mn + (mx - mn) / 2 is exact
    c = np.array([3.0, -2.0, 5.0])
    return records(c - h, c + h)


def _half_identical(n, seed):
    out = _random(n, seed)
    out[n // 4: n // 4 + n // 2, 8:16] = out[0, 8:16]
    return out


def _huge(n, seed):
    """random boxes, four of them slabs with corners out to +-1e37 whose centroids lie far out on x: every cost of a node that holds
    one is infinite (dx * dy overflows), so the first candidate wins there -- three such nodes, then the tree is an ordinary one.  (A
    set with ALL coordinates that large prices every node at infinity and peels bin 0 off level after level: a valid tree of the
    definition, but deeper than TRC_MAX_BVH_DEPTH, which the device build refuses.)"""
    out = _random(n, seed)
    box = out.view(F)
    for slot, (x0, x1) in zip((n // 2, 0, n - 1, 1), ((-1e37, -0.8e37), (-0.6e37, -0.4e37), (0.4e37, 0.6e37), (0.8e37, 1e37))):
        box[slot, rr.MINI] = (x0, -1e37, -1.0); box[slot, rr.MAXI] = (x1, 1e37, 1.0)
    return out


def _signed_zeros(n, seed):
    r = np.random.default_rng(seed)
    mn = r.choice([-1.0, -0.0, 0.0], (n, 3)); mx = r.choice([-0.0, 0.0, 1.0], (n, 3))
    return records(mn, mx)


def _ball(n, seed):
    """the 48-triangle ball of the animation tests (tests/test_gpu_update_vertices.py): the leaf records of its scene"""
    from tracer_amd import host
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(4, 6, 0.1))
    tree = sc.bvh_array().copy()
    leaves = tree[1:sc.n_leaves + 1].copy()
    leaves[:, [PARENT, LEFT, RIGHT]] = 0
    return leaves


families = {"random": _random, "ball48": _ball, "lattice": _lattice, "line_x": _line(0), "line_y": _line(1), "line_z": _line(2),
            "coplanar": _coplanar, "identical": _identical, "half_identical": _half_identical, "huge": _huge, "signed_zeros": _signed_zeros}
