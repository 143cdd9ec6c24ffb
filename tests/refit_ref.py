"""The definition of trc_update_vertices (include/tracer_abi.h) restated in numpy, for tests/test_refit_cpu.py and
tests/test_gpu_update_vertices.py: the same topology, a triangle leaf's box from trc_host_build_node under the identity matrix for the
box of its three current vertices, an interior box the min / max of its two children's (the right child's bound on a tie), the boxes
of the analytic primitives kept."""
import ctypes as C

import numpy as np

from tracer_amd import abi, host

F = np.float32
PARENT, LEFT, RIGHT, AXIS, PTYPE, PINDEX = range(6)
MINI, MAXI = slice(8, 11), slice(12, 15)


def raw(nodes):
    """(n, 16) uint32 copy of a ctypes array of abi.BVH"""
    return np.frombuffer(bytes(memoryview(nodes)), dtype=np.uint32).reshape(-1, 16).copy()


def vertices_of(view):
    a = (C.c_float * (8 * view.n_vertex)).from_address(C.addressof(view.triList.contents))
    return np.frombuffer(a, dtype=np.float32).reshape(-1, 8).copy()


def indices_of(view):
    a = (C.c_uint32 * view.n_index).from_address(C.addressof(view.idxList.contents))
    return np.frombuffer(a, dtype=np.uint32).copy()


def triangle_leaf_box(tri_vertices):
    """(3, 3) float32 positions -> (mini, maxi) through trc_host_build_node under the identity matrix"""
    lo, hi = tri_vertices[0].copy(), tri_vertices[0].copy()
    for v in tri_vertices[1:]:                       # std::min / std::max of an initializer list: the first of equals stays
        lo = np.where(v < lo, v, lo); hi = np.where(hi < v, v, hi)
    r = host.build_node(tuple(float(x) for x in lo), tuple(float(x) for x in hi), abi.PRIM_TRIANGLE, 0)
    return (np.array([r.bBOX.mini.x, r.bBOX.mini.y, r.bBOX.mini.z], F), np.array([r.bBOX.maxi.x, r.bBOX.maxi.y, r.bBOX.maxi.z], F))


def refit(nodes, vertices, indices):
    """nodes: (n, 16) uint32 records, root at 0; vertices: (n_vertex, 8) float32; indices: uint32, 3 per triangle -> the refitted records"""
    out = nodes.copy()
    box = out.view(F)
    pos = np.ascontiguousarray(vertices, dtype=F)[:, :3]
    tri = np.asarray(indices, dtype=np.uint32).reshape(-1, 3)
    order, head = [0], 0                             # parents before children
    while head < len(order):
        i = order[head]; head += 1
        if out[i, PTYPE] == abi.PRIM_BVH:
            order += [int(out[i, LEFT]), int(out[i, RIGHT])]
    assert len(order) == len(out)
    for i in reversed(order):
        if out[i, PTYPE] == abi.PRIM_TRIANGLE:
            lo, hi = triangle_leaf_box(pos[tri[out[i, PINDEX]]])
        elif out[i, PTYPE] == abi.PRIM_BVH:
            l, r = int(out[i, LEFT]), int(out[i, RIGHT])
            lo = np.where(box[l, MINI] < box[r, MINI], box[l, MINI], box[r, MINI])
            hi = np.where(box[l, MAXI] > box[r, MAXI], box[l, MAXI], box[r, MAXI])
        else:
            continue
        box[i, MINI] = lo; box[i, MAXI] = hi
        out[i, 11] = 0; out[i, 15] = 0               # the padding lane of a rewritten corner
    return out


def as_nodes(records):
    """(n, 16) uint32 -> ctypes array of abi.BVH"""
    return (abi.BVH * len(records)).from_buffer_copy(np.ascontiguousarray(records).tobytes())


class Moved:
    """a copy of a scene view over another node array and other vertices (kept alive here)"""

    def __init__(self, view, records, vertices):
        self.nodes = as_nodes(records)
        self.vertices = np.ascontiguousarray(vertices, dtype=F)
        self.view = abi.Scene.from_buffer_copy(view)
        self.view.bvhList = C.cast(self.nodes, C.POINTER(abi.BVH)); self.view.n_bvh = len(records)
        self.view.triList = C.cast(self.vertices.ctypes.data, C.POINTER(abi.TriangleVertex))


def twist(vertices, angle, scale=0.9):
    """deterministic twist-and-scale of (n, 8) vertices about the centre of their box: a rotation about the vertical axis that grows
    with height, from -angle / 2 at the bottom to +angle / 2 at the top, and a uniform scale; normals are rotated alike"""
    v = np.asarray(vertices, dtype=np.float64).copy()
    lo, hi = v[:, :3].min(0), v[:, :3].max(0)
    c = 0.5 * (lo + hi)
    q = v[:, :3] - c
    a = angle * q[:, 1] / max(hi[1] - lo[1], 1e-9)
    ca, sa = np.cos(a), np.sin(a)
    v[:, 0] = c[0] + scale * (ca * q[:, 0] + sa * q[:, 2]); v[:, 1] = c[1] + scale * q[:, 1]; v[:, 2] = c[2] + scale * (-sa * q[:, 0] + ca * q[:, 2])
    n = v[:, 3:6].copy()
    v[:, 3] = ca * n[:, 0] + sa * n[:, 2]; v[:, 5] = -sa * n[:, 0] + ca * n[:, 2]
    return v.astype(F)
