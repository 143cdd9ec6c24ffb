"""The definition of trc_pose_vertices (include/tracer_abi.h) restated in numpy, for tests/test_pose_cpu.py and
tests/test_gpu_pose_vertices.py.  Everything is a float32 array and every line is ONE operation, so nothing is fused and the order
of the sum is the header's:  x' = ((c0.x*x + c1.x*y) + c2.x*z) + c3.x.

A pose here is (first, count, model, normal): two (4, 4) matrices in the mathematical layout, m[r, c] = row r of column c (the ABI
stores them column-major).  Vertices are (n, 8) float32 rows: position, normal, uv."""
import numpy as np

F = np.float32


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def transform(m, x, y, z, translate):
    """rows 0..2 of m applied to (x, y, z): ((m[r,0]*x + m[r,1]*y) + m[r,2]*z) [+ m[r,3]] -> three float32 arrays"""
    m = _f(m)
    out = []
    for r in range(3):
        t0 = m[r, 0] * x
        t1 = m[r, 1] * y
        t2 = m[r, 2] * z
        s = t0 + t1
        s = s + t2
        if translate:
            s = s + m[r, 3]
        assert s.dtype == F
        out.append(s)
    return out


def pose(rest, current, poses):
    """rest, current: (n, 8) float32; -> the vertices after trc_pose_vertices(poses): every range from REST, the others as in current"""
    rest, out = _f(rest), _f(current).copy()
    for first, count, model, normal in poses:
        r = rest[first:first + count]
        x, y, z = transform(model, r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), True)
        nx, ny, nz = transform(normal, r[:, 3].copy(), r[:, 4].copy(), r[:, 5].copy(), False)
        out[first:first + count] = np.stack([x, y, z, nx, ny, nz, r[:, 6], r[:, 7]], axis=1)
    return out


def valid(poses, n_vertex):
    """what trc_pose_vertices accepts (TRC_OK) on a scene with n_vertex > 0 vertices; a refusal is TRC_ERR_INVALID_ARG"""
    ranges = []
    for first, count, model, normal in poses:
        if count == 0 or first + count > n_vertex:
            return False
        if not np.isfinite(_f(model)[:3, :4]).all() or not np.isfinite(_f(normal)[:3, :3]).all():
            return False
        ranges.append((first, first + count))
    ranges.sort()
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


# ---------------------------------------------------------------------------------------------------- matrices for the tests
def identity():
    return np.eye(4, dtype=F)


def turn(centre, angle, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """(model, normal): T(centre + shift) * R_y(angle) * S(scale) * T(-centre), composed in float64 and rounded once, and its inverse
    transpose.  With an angle whose cosine and sine are inexact in float32 and a non-uniform scale no product of the pose is exact."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=np.float64)
    sc = np.diag([scale[0], scale[1], scale[2], 1.0])
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3] = -np.asarray(centre, dtype=np.float64)
    t1[:3, 3] = np.asarray(centre, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    model = t1 @ rot @ sc @ t0
    normal = np.eye(4)
    normal[:3, :3] = np.linalg.inv(model[:3, :3]).T
    return model.astype(F), normal.astype(F)


def box_centre(vertices):
    p = np.asarray(vertices, dtype=np.float64)[:, :3]
    return 0.5 * (p.min(0) + p.max(0))
