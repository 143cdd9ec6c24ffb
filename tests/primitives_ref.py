"""The definition of trc_update_primitives (include/tracer_abi.h) restated in numpy, for tests/test_primitives_cpu.py and
tests/test_gpu_update_primitives.py: the device's record of a sphere, a square and a cube, the leaf box of an analytic primitive
(trc_host_build_node), and the refit of a tree whose analytic leaves moved (tests/refit_ref.py does the rest).  Every value is a
float32 and every line is ONE operation, so nothing is fused and the order of every sum is the header's.

Records are the ctypes PODs of tracer_amd/abi.py; a node array is (n, 16) uint32 as refit_ref.raw gives it."""
import ctypes as C

import numpy as np

import refit_ref as rr
from tracer_amd import abi, host

F = np.float32
U = np.uint32
SPHERE_DWORDS, SQUARE_DWORDS, CUBE_DWORDS = 8, 8, 40


def _bits(x):
    return np.asarray(x, dtype=F).reshape(1).view(U)[0]


def _cols(m, n=4):
    """the xyz rows of the first n columns of an abi.float4x4: [column][row]"""
    return [[F(m.columns[c].x), F(m.columns[c].y), F(m.columns[c].z)] for c in range(n)]


# ------------------------------------------------------------------------------------------------- the scene's lists
def spheres_of(view):
    return (abi.Sphere * view.n_sphere).from_buffer_copy(C.string_at(view.sphereList, C.sizeof(abi.Sphere) * view.n_sphere)) if view.n_sphere else (abi.Sphere * 0)()


def squares_of(view):
    return (abi.Square * view.n_square).from_buffer_copy(C.string_at(view.squareList, C.sizeof(abi.Square) * view.n_square)) if view.n_square else (abi.Square * 0)()


def cubes_of(view):
    return (abi.Cube * view.n_cube).from_buffer_copy(C.string_at(view.cubeList, C.sizeof(abi.Cube) * view.n_cube)) if view.n_cube else (abi.Cube * 0)()


# ------------------------------------------------------------------------------------------------- record packing
def pack_sphere(s):
    q = np.zeros(SPHERE_DWORDS, U)
    q[0], q[1], q[2], q[3] = _bits(s.center.x), _bits(s.center.y), _bits(s.center.z), _bits(s.radius)
    q[4] = s.material
    return q


def pack_square(s):
    q = np.zeros(SQUARE_DWORDS, U)
    i0, i1, j0, j1 = F(s.range_i.x), F(s.range_i.y), F(s.range_j.x), F(s.range_j.y)
    di = i1 - i0
    dj = j1 - j0
    area = F(2) * di
    area = area * dj
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = F(1) / area
    assert pdf.dtype == F
    q[0], q[1], q[2], q[3] = _bits(i0), _bits(i1), _bits(j0), _bits(j1)
    q[4], q[5] = _bits(s.value_k), _bits(pdf)
    q[6] = s.axis_i | (s.axis_j << 2) | (s.axis_k << 4)
    q[7] = s.material
    return q


def pack_cube(c):
    q = np.zeros(CUBE_DWORDS, U)
    for base, m, n in ((0, c.inverse_matrix, 4), (12, c.model_matrix, 4), (24, c.normal_matrix, 3)):
        for k, col in enumerate(_cols(m, n)):
            for r in range(3):
                q[base + 3 * k + r] = _bits(col[r])
    for k, v in enumerate((c.box.mini.x, c.box.mini.y, c.box.mini.z, c.box.maxi.x, c.box.maxi.y, c.box.maxi.z)):
        q[33 + k] = _bits(v)
    q[39] = c.material
    return q


# ------------------------------------------------------------------------------------------------- the leaf box
def leaf_box(mini, maxi, cols):
    """mini, maxi: three float32 each; cols: [column][row] of the model matrix's xyz rows, four columns -> (lo, hi), (3,) float32 each.
    The eight corners in the order i, j, k; each row ((m0 * x + m1 * y) + m2 * z) + m3 * 1; fmin / fmax from +-FLT_MAX, the second
    operand kept on a tie."""
    ele = ([F(v) for v in mini], [F(v) for v in maxi])
    big = np.finfo(F).max
    lo, hi = [big, big, big], [-big, -big, -big]
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    x, y, z = ele[i][0], ele[j][1], ele[k][2]
                    for q in range(3):
                        t0 = F(cols[0][q]) * x
                        t1 = F(cols[1][q]) * y
                        s = t0 + t1
                        t2 = F(cols[2][q]) * z
                        s = s + t2
                        t3 = F(cols[3][q]) * F(1)
                        w = s + t3
                        assert w.dtype == F
                        lo[q] = lo[q] if lo[q] < w else w
                        hi[q] = hi[q] if hi[q] > w else w
    return np.array(lo, F), np.array(hi, F)


def _box3(b):
    return (b.mini.x, b.mini.y, b.mini.z), (b.maxi.x, b.maxi.y, b.maxi.z)


def primitive_leaf_box(ptype, rec):
    box = rec.box if ptype == abi.PRIM_CUBE else rec.boundingBOX
    return leaf_box(*_box3(box), _cols(rec.model_matrix))


# ------------------------------------------------------------------------------------------------- the refit
def refit(nodes, spheres, squares, cubes, vertices=None, indices=None):
    """the records after trc_update_primitives left the scene with these lists (and trc_update_vertices with these vertices): every
    analytic leaf's box from its record, padding lane 0, then refit_ref.refit for the triangle leaves and every interior box"""
    out = nodes.copy()
    box = out.view(F)
    lists = {abi.PRIM_SPHERE: spheres, abi.PRIM_SQUARE: squares, abi.PRIM_CUBE: cubes}
    for i in range(len(out)):
        t = int(out[i, rr.PTYPE])
        if t in lists:
            lo, hi = primitive_leaf_box(t, lists[t][int(out[i, rr.PINDEX])])
            box[i, rr.MINI] = lo; box[i, rr.MAXI] = hi
            out[i, 11] = 0; out[i, 15] = 0
    if vertices is None:
        vertices, indices = np.zeros((0, 8), F), np.zeros(0, U)
    return rr.refit(out, vertices, indices)


def leaves(nodes, spheres, squares, cubes):
    """trc_host_build_node leaf records, in the order the leaves appear in `nodes`, of the analytic leaves under the new lists; the
    triangle leaves as they are"""
    lists = {abi.PRIM_SPHERE: spheres, abi.PRIM_SQUARE: squares, abi.PRIM_CUBE: cubes}
    out = []
    for rec in nodes:
        t, k = int(rec[rr.PTYPE]), int(rec[rr.PINDEX])
        if t in lists:
            r = lists[t][k]
            lo, hi = _box3(r.box if t == abi.PRIM_CUBE else r.boundingBOX)
            m = [[getattr(r.model_matrix.columns[c], "xyzw"[row]) for c in range(4)] for row in range(4)]
            out.append(host.build_node(lo, hi, t, k, m))
        elif t == abi.PRIM_TRIANGLE:
            out.append(abi.BVH.from_buffer_copy(rec.tobytes()))
    return out


class Moved:
    """a copy of a scene view over other primitive lists and another node array (kept alive here)"""

    def __init__(self, view, records, spheres, squares, cubes, vertices=None):
        self.nodes = rr.as_nodes(records)
        self.spheres, self.squares, self.cubes = spheres, squares, cubes
        self.view = abi.Scene.from_buffer_copy(view)
        self.view.bvhList = C.cast(self.nodes, C.POINTER(abi.BVH)); self.view.n_bvh = len(records)
        self.view.sphereList = C.cast(spheres, C.POINTER(abi.Sphere))
        self.view.squareList = C.cast(squares, C.POINTER(abi.Square))
        self.view.cubeList = C.cast(cubes, C.POINTER(abi.Cube))
        if vertices is not None:
            self.vertices = np.ascontiguousarray(vertices, dtype=F)
            self.view.triList = C.cast(self.vertices.ctypes.data, C.POINTER(abi.TriangleVertex))


# ------------------------------------------------------------------------------------------------- the tests' motion
def rotation_y(angle, translate, scale):
    """T * Ry * S as a (4, 4) float32 array m[r][c]"""
    c, s = np.cos(angle), np.sin(angle)
    m = np.array([[c * scale[0], 0, s * scale[2], translate[0]], [0, scale[1], 0, translate[1]],
                  [-s * scale[0], 0, c * scale[2], translate[2]], [0, 0, 0, 1]], np.float64)
    return m.astype(F)


def motion(view, phase=1.0):
    """(spheres, squares, cubes): the scene's lists with, at once, sphere 0 and three others translated and resized, the light square 5
    shifted and shrunk, cube 0 under a new rotation and translation, and the container cube (the last) moved.  phase 0 is the scene's
    own lists, bit for bit."""
    sp, sq, cb = spheres_of(view), squares_of(view), cubes_of(view)
    if phase == 0.0:
        return sp, sq, cb
    p = float(phase)
    for k, (r, c) in {0: (50.0, (230.0, 230.0, 260.0)), 3: (30.0, (310.0, 70.0, 90.0)), 7: (44.0, (20.0, 470.0, 380.0)),
                      11: (25.0, (560.0, 440.0, 300.0))}.items():
        if k < len(sp):
            o = sp[k].center
            sp[k] = host.make_sphere(F(r), (F(o.x + p * (c[0] - o.x)), F(o.y + p * (c[1] - o.y)), F(o.z + p * (c[2] - o.z))), sp[k].material)
    if len(sq) > 5:
        s = sq[5]
        sq[5] = host.make_square(s.axis_i, F(s.range_i.x - 60 * p), F(s.range_i.y - 90 * p), s.axis_j, F(s.range_j.x + 25 * p), F(s.range_j.y + 5 * p),
                                 s.axis_k, F(s.value_k - 12 * p), s.material)
    if len(cb) > 0:
        cb[0] = host.make_cube(cb[0].material, rotation_y(0.26 + 0.9 * p, (300 - 40 * p, 1 + 20 * p, 330), (165, 330 - 60 * p, 165)))
        last = len(cb) - 1
        if last > 0:
            cb[last] = host.make_cube(cb[last].material, rotation_y(0.4 * p, (60 * p, 200 - 30 * p, 65 + 50 * p), (200, 200, 80)))
    return sp, sq, cb


# ------------------------------------------------------------------------------------------------- the motion texels
def motion_texels(hits, current, snapshot):
    """The motion texels of analytic winners (include/tracer_abi.h, "Motion tracking"): `hits` are the production walk's records of the
    G-buffer rays (hit, pType, pIndex, p), current / snapshot the (spheres, squares, cubes) lists now and when the last trc_denoise ran.
    -> (n,) motion_ref.MOTION, zero wherever the winner is no analytic primitive or its record did not change"""
    from motion_ref import MOTION
    out = np.zeros(len(hits), MOTION)
    for i in np.nonzero((hits["hit"] != 0) & (hits["pType"] <= abi.PRIM_CUBE))[0]:
        t, k = int(hits["pType"][i]), int(hits["pIndex"][i])
        p = [F(v) for v in hits["p"][i]]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if t == abi.PRIM_SPHERE:
                c, s = pack_sphere(current[0][k])[:4].view(F), pack_sphere(snapshot[0][k])[:4].view(F)
                moved = bool((c != s).any())
                prev = []
                for a in range(3):
                    d = p[a] - c[a]
                    n = d / c[3]
                    m = n * s[3]
                    prev.append(s[a] + m)
            elif t == abi.PRIM_SQUARE:
                c, s = pack_square(current[1][k]), pack_square(snapshot[1][k])
                cf, sf = c.view(F), s.view(F)
                moved = bool((cf[:5] != sf[:5]).any() or c[6] != s[6])
                ai, aj = int(c[6]) & 3, (int(c[6]) >> 2) & 3
                si, sj, sk = int(s[6]) & 3, (int(s[6]) >> 2) & 3, (int(s[6]) >> 4) & 3
                a, b = p[ai], p[aj]
                di = cf[1] - cf[0]
                fu = a - cf[0]
                fu = fu / di
                dj = cf[3] - cf[2]
                fv = b - cf[2]
                fv = fv / dj
                prev = [F(0), F(0), F(0)]
                prev[sk] = sf[4]
                e = sf[1] - sf[0]
                e = fu * e
                prev[si] = sf[0] + e
                e = sf[3] - sf[2]
                e = fv * e
                prev[sj] = sf[2] + e
            else:
                c, s = pack_cube(current[2][k]).view(F), pack_cube(snapshot[2][k]).view(F)
                moved = bool((c[:24] != s[:24]).any())
                q = []
                for r in range(3):                                   # ((I0 * p.x + I1 * p.y) + I2 * p.z) + I3, row r
                    t0 = c[r] * p[0]
                    t1 = c[3 + r] * p[1]
                    acc = t0 + t1
                    t2 = c[6 + r] * p[2]
                    acc = acc + t2
                    q.append(acc + c[9 + r])
                prev = []
                for r in range(3):                                   # ((M0' * q.x + M1' * q.y) + M2' * q.z) + M3', row r
                    t0 = s[12 + r] * q[0]
                    t1 = s[15 + r] * q[1]
                    acc = t0 + t1
                    t2 = s[18 + r] * q[2]
                    acc = acc + t2
                    prev.append(acc + s[21 + r])
        if moved:
            assert all(np.asarray(v).dtype == F for v in prev)
            out["prev"][i] = prev
            out["moved"][i] = 1
    return out
