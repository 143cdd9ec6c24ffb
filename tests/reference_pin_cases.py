"""Inputs of the reference pin (tests/test_reference_pin.py, tests/golden/make_reference_pin.py, tests/test_gpu_reference_pin.py).

CASES maps a name to a Case: how many hand-made edge inputs it has and a function pin -> {field: array}, where pin is
oracle.pyoracle.Pin, either family.  Every case feeds its edge inputs first, then N_SEEDED inputs from a fixed seed; nothing
is stored but what the reference's own code answered (tests/golden/reference_pin.npz).  No input is made from an output of the
code under test: where an input must sit exactly on a computed value (t == range_t.y ...), the value is computed here, in
numpy binary32, one correctly rounded operation at a time, in the order the reference writes it.

Edge classes per area: the table in the docstring of tests/test_reference_pin.py.
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np

from oracle import pyoracle as po
from tracer_amd import abi

F32 = np.float32
N_SEEDED = 200_000
N_STORED = 512                       # of the seeded inputs, how many have their whole output recorded (1 024 did not fit in 512 KB)
N_SCENE_RAYS = 8192
FLT_MAX, FLT_MIN, FLT_EPS = np.finfo(F32).max, np.finfo(F32).tiny, np.finfo(F32).eps
DENORM = F32(1e-42)
ONE_BELOW = F32(1 - 2.0 ** -24)
REC_FIELDS = ["accepted", "range_y", "t", "p", "gn", "sn", "uv", "material", "PDF", "f"]


class Case:
    """n_edge: the inputs before the seeded ones; run: pin -> {field: array}; excluded: fields not compared (the table of the test);
    stored: the rows whose whole output the golden file keeps (default: the edges and the first N_STORED seeded)"""

    def __init__(self, n_edge, run, excluded=(), stored=None):
        self.n_edge, self.run, self.excluded = n_edge, run, frozenset(excluded)
        self.stored = np.arange(n_edge + N_STORED) if stored is None else np.asarray(stored)


def ulps(x, k):
    """x moved by k units in the last place (k may be an array), away from or towards zero by the sign of k * sign(x)"""
    x = np.asarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, np.int64(-0x80000000) - i, i) + k         # to a monotone integer line and back
    i = np.where(i < 0, np.int64(-0x80000000) - i, i)
    return i.astype(np.int32).view(F32)


def pow10(rs, lo, hi, size=None):
    """log-uniform over [10^lo, 10^hi), roughly, made of exact operations only (ldexp of a uniform mantissa): the inputs must come
    out bit for bit the same on every machine, and a vectorised float64 pow / exp / cos need not"""
    e = rs.randint(int(np.floor(lo * 3.3219281)), int(np.ceil(hi * 3.3219281)), size)
    return np.ldexp(rs.uniform(1.0, 2.0, size), e)


def mat3_vec(M, v):
    """(n, 3, 3) times (n, 3), one product and one sum at a time (no BLAS, no einsum: their summation order and fusing are the machine's)"""
    return (M[:, :, 0] * v[:, 0:1] + M[:, :, 1] * v[:, 1:2]) + M[:, :, 2] * v[:, 2:3]


def unit(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):                              # a null vector stays an input: NaN
        return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def dot3(a, b):
    """dot as the reference's convention has it: ((a.x*b.x) + (a.y*b.y)) + (a.z*b.z), every step rounded to binary32"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def carray(T, arr):
    """numpy structured array with T's layout -> ctypes array of T"""
    assert arr.dtype.itemsize == C.sizeof(T)
    return (T * len(arr)).from_buffer_copy(arr.tobytes())


def rec_fields(rec):
    return {f: rec[f] for f in REC_FIELDS}


def cat_rays(*parts):
    return np.ascontiguousarray(np.concatenate(parts))


# ---------------------------------------------------------------------------------------------------------------- sphere
def _spheres():
    rs = np.random.RandomState(101)
    s = np.zeros(64, dtype=np.dtype(abi.Sphere))
    s["radius"][0], s["material"][0] = 1.0, 3                      # sphere 0: unit sphere at the origin, exact arithmetic
    r = rs.uniform(0.05, 90, 63).astype(F32)
    s["radius"][1:] = r + F32(0.0001)                              # MakeSphere inflates the radius by 1e-4
    c = rs.uniform(-300, 300, (63, 3)).astype(F32)
    s["center"]["x"][1:], s["center"]["y"][1:], s["center"]["z"][1:] = c[:, 0], c[:, 1], c[:, 2]
    s["material"][1:] = rs.randint(0, 24, 63)
    return s


def _sphere_near_root(s, k, o, d):
    """(-half_b - root) / a and (-half_b + root) / a of Sphere.hh:35-63 in numpy binary32 (NaN where discriminant <= 0)"""
    c = np.stack([s["center"]["x"][k], s["center"]["y"][k], s["center"]["z"][k]], -1)
    oc = o - c
    a, half_b = dot3(d, d), dot3(oc, d)
    cc = dot3(oc, oc) - s["radius"][k] * s["radius"][k]
    disc = half_b * half_b - a * cc
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.where(disc > 0, disc, np.nan).astype(F32))
    return (-half_b - root) / a, (-half_b + root) / a


def _sphere_inputs():
    s = _spheres()
    rs = np.random.RandomState(102)
    # --- edges, all on sphere 0 unless said: item i uses primitive i % 64, so an edge ray sits at an index that is 0 mod 64
    E = []

    def edge(o, d, lo=FLT_MIN, hi=FLT_MAX, k=0):
        E.append((k, o, d, lo, hi))
    for z in (-0.5, -0.25, 0.0, 0.125, 3.0):                        # discriminant exactly 0, and 1..3 ulp either side of it
        for kk in range(-3, 4):
            edge((ulps(F32(1.0), kk), 0.0, z), (0, 0, 1))
            edge((0.0, ulps(F32(-1.0), kk), z), (0, 0, -1))
    for hi in (ulps(F32(2.0), -1), F32(2.0), ulps(F32(2.0), 1), F32(4.0), ulps(F32(4.0), 1), ulps(F32(4.0), -1)):
        edge((0, 0, -3), (0, 0, 1), FLT_MIN, hi)                    # near root 2 (far root 4) exactly t_max, 1 ulp around
    for lo in (ulps(F32(2.0), -1), F32(2.0), ulps(F32(2.0), 1), F32(4.0), ulps(F32(4.0), -1)):
        edge((0, 0, -3), (0, 0, 1), lo, FLT_MAX)                    # ... exactly t_min
        edge((0, 0, -3), (0, 0, 1), lo, F32(4.0))
    for o in ((0, 0, 0), (0.5, 0.25, -0.125), (0, 0.999, 0), (1, 0, 0), (0, 0, -1)):    # inside / on the surface: second root
        for d in ((0, 0, 1), (0, 1, 0), (-1, 0, 0), (0.6, 0, 0.8)):
            edge(o, d)
    for sc in (1e-20, 1e-19, 3e-23, 1e19, 0.5, 2.0, 3.0):           # a denormal / tiny / huge: direction not normalised
        edge((0.1, 0.2, -3), (0, 0, sc)); edge((0.1, 0.2, -3), (0.01 * sc, 0, sc))
    for oy, dy in ((5, -1), (-5, 1), (0, 1), (0, -1)):              # gn.y = +-1 (asin edge), gn.x = gn.z = 0: atan2(+-0, +-0)
        for dx, dz in ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)):
            edge((0, oy, 0), (dx, dy, dz))
    for o, d in (((5, 0, 0), (-1, 0, 0)), ((-5, 0, 0), (1, 0, 0)), ((-5, 0, 0), (1, 0, -0.0)), ((0, 0, 5), (0, 0, -1)), ((0, 0, -5), (0, 0, 1))):
        edge(o, d)                                                  # atan2 on the axes: phi = 0, +-pi, +-pi/2
    n_hand = len(E)
    # grazing rays at the inflated spheres: the discriminant near 0 with both signs; roots pinned to range_t
    n_graze = 64 * 24
    k = np.arange(n_graze) % 64
    c = np.stack([s["center"]["x"][k], s["center"]["y"][k], s["center"]["z"][k]], -1)
    tang = unit(rs.normal(size=(n_graze, 3)))
    away = unit(np.cross(tang, rs.normal(size=(n_graze, 3))))
    o = (c + away * (s["radius"][k] * (1 + rs.choice([-1, 1], n_graze) * pow10(rs, -8, -5, n_graze)).astype(F32))[:, None]
         - tang * rs.uniform(1, 50, n_graze).astype(F32)[:, None]).astype(F32)
    graze = po.pin_rays(o, tang, FLT_MIN, FLT_MAX)
    n_pin = 64 * 32
    k = np.arange(n_pin) % 64
    c = np.stack([s["center"]["x"][k], s["center"]["y"][k], s["center"]["z"][k]], -1)
    d = unit(rs.normal(size=(n_pin, 3)))
    o = (c - d * (s["radius"][k] * rs.uniform(0.0, 4, n_pin).astype(F32))[:, None] + rs.normal(0, 0.3, (n_pin, 3)) * s["radius"][k][:, None]).astype(F32)
    near, far = _sphere_near_root(s, k, o, d)
    which = np.arange(n_pin) // 64 % 8
    lo = np.full(n_pin, FLT_MIN, F32); hi = np.full(n_pin, FLT_MAX, F32)
    with np.errstate(invalid="ignore"):
        hi = np.where(which == 0, near, hi); hi = np.where(which == 1, ulps(near, 1), hi); hi = np.where(which == 2, far, hi)
        hi = np.where(which == 3, ulps(far, 1), hi)
        lo = np.where(which == 4, near, lo); lo = np.where(which == 5, ulps(near, -1), lo); lo = np.where(which == 6, far, lo)
        lo = np.where(which == 7, ulps(far, -1), lo)
    lo = np.where(np.isnan(lo), FLT_MIN, lo).astype(F32); hi = np.where(np.isnan(hi), FLT_MAX, hi).astype(F32)
    pinned = po.pin_rays(o, d, lo, hi)
    hand = po.pin_rays(np.zeros((64 * n_hand, 3), F32), np.tile(np.array([[0, 0, 1]], F32), (64 * n_hand, 1)), FLT_MIN, FLT_MAX)
    hand["origin"][:, 0] = 1e6                                      # filler between hand-made rays: misses
    for i, (kk, o_, d_, lo_, hi_) in enumerate(E):
        j = 64 * i + kk
        hand["origin"][j], hand["direction"][j], hand["range"][j] = o_, d_, (lo_, hi_)
    # --- seeded
    n = N_SEEDED
    k = np.arange(len(hand) + len(graze) + len(pinned), len(hand) + len(graze) + len(pinned) + n) % 64
    c = np.stack([s["center"]["x"][k], s["center"]["y"][k], s["center"]["z"][k]], -1)
    r = s["radius"][k]
    o = (c + unit(rs.normal(size=(n, 3))) * (r * rs.uniform(0.0, 5, n).astype(F32))[:, None]).astype(F32)
    aim = c + rs.normal(0, 0.7, (n, 3)) * r[:, None]
    d = unit(aim - o) * np.where(rs.rand(n) < 0.3, pow10(rs, -3, 3, n), 1.0).astype(F32)[:, None]
    hi = np.where(rs.rand(n) < 0.5, FLT_MAX, (r * rs.uniform(0, 8, n)).astype(F32)).astype(F32)
    lo = np.where(rs.rand(n) < 0.8, FLT_MIN, (r * rs.uniform(0, 3, n)).astype(F32)).astype(F32)
    seeded = po.pin_rays(o, d.astype(F32), lo, hi)
    return carray(abi.Sphere, s), cat_rays(hand, graze, pinned, seeded), len(hand) + len(graze) + len(pinned), [64 * i + e[0] for i, e in enumerate(E)]


# ---------------------------------------------------------------------------------------------------------------- square
AXES = [(1, 2, 0), (0, 2, 1), (0, 1, 2)]      # (axis_i, axis_j, axis_k) as MakeSquare orders them


def _squares():
    rs = np.random.RandomState(201)
    q = np.zeros(48, dtype=np.dtype(abi.Square))
    for n in range(48):
        ai, aj, ak = AXES[n % 3]
        q["axis_i"][n], q["axis_j"][n], q["axis_k"][n] = ai, aj, ak
        if n < 3:                                                    # squares 0..2: [0, 4] x [-2, 2] at k = 1, one per axis: exact arithmetic
            q["range_i"][n] = (0.0, 4.0); q["range_j"][n] = (-2.0, 2.0); q["value_k"][n] = 1.0
        else:
            lo = rs.uniform(-300, 300, 2).astype(F32); ext = rs.uniform(0.5, 300, 2).astype(F32)
            q["range_i"][n] = (lo[0], lo[0] + ext[0]); q["range_j"][n] = (lo[1], lo[1] + ext[1])
            q["value_k"][n] = F32(rs.uniform(-300, 300))
        q["material"][n] = n % 24
    return q


def _square_inputs():
    q = _squares()
    rs = np.random.RandomState(202)
    E = []

    def edge(ax, o_ijk, d_ijk, lo=FLT_MIN, hi=FLT_MAX):
        """ray given in the square's own (i, j, k) order, for square `ax` of the three exact ones"""
        ai, aj, ak = AXES[ax]
        o, d = np.zeros(3, F32), np.zeros(3, F32)
        o[ai], o[aj], o[ak] = o_ijk
        d[ai], d[aj], d[ak] = d_ijk
        E.append((ax, o, d, lo, hi))
    for ax in range(3):
        for dk in (0.0, -0.0, DENORM, -DENORM, F32(1e-38), F32(-3e-39)):           # direction[k] = +-0 (t inf or NaN), denormal
            for ok in (1.0, 3.0, -2.0):                                            # ... with the origin ON the plane: 0 / 0
                edge(ax, (1, 0, ok), (0.3, 0.1, dk))
        for ok, dk in ((3.0, -1.0), (-1.0, 1.0), (3.0, -0.5), (-1.0, 4.0)):        # both faces; t = 2, 2, 4, 0.5 exactly
            t = F32((1.0 - ok) / dk)
            for lo, hi in ((FLT_MIN, FLT_MAX), (t, FLT_MAX), (ulps(t, 1), FLT_MAX), (ulps(t, -1), FLT_MAX), (FLT_MIN, t), (FLT_MIN, ulps(t, -1)),
                           (FLT_MIN, ulps(t, 1)), (t, t)):
                edge(ax, (1, 0, ok), (0, 0, dk), lo, hi)
            # a, b exactly on each of the four edges and 1 ulp outside / inside (d_i = d_j = 0: a = o_i, b = o_j exactly)
            for kk in (-1, 0, 1):
                edge(ax, (ulps(F32(0.0), kk) if kk else 0.0, 0, ok), (0, 0, dk)); edge(ax, (ulps(F32(4.0), kk), 0, ok), (0, 0, dk))
                edge(ax, (1, ulps(F32(-2.0), kk), ok), (0, 0, dk)); edge(ax, (1, ulps(F32(2.0), kk), ok), (0, 0, dk))
            edge(ax, (-0.0, 0, ok), (0, 0, dk)); edge(ax, (0.0, -0.0, ok), (-0.0, -0.0, dk))     # signed zeros into p and uv
            edge(ax, (0, -2, ok), (0, 0, dk)); edge(ax, (4, 2, ok), (0, 0, dk))                  # the corners
        for ok in (1.0,):                                                          # origin on the plane: t = 0, below FLT_MIN ...
            edge(ax, (1, 0, ok), (0, 0, 1)); edge(ax, (1, 0, ok), (0, 0, -1))
            edge(ax, (1, 0, ok), (0, 0, 1), 0.0, FLT_MAX); edge(ax, (1, 0, ok), (0, 0, -1), -1.0, 0.0)   # ... unless range_t admits it
            edge(ax, (1, 0, ok), (0, 0, 1), -0.0, 0.0)
        edge(ax, (1, 0, 3), (0, 0, 1)); edge(ax, (1, 0, 3), (0, 0, 1), -FLT_MAX, FLT_MAX)         # behind the origin: t < 0
    n_hand = len(E)
    hand = po.pin_rays(np.full((48 * n_hand, 3), 1e6, F32), np.tile(np.array([[1, 1, 1]], F32), (48 * n_hand, 1)), FLT_MIN, FLT_MAX)
    for i, (ax, o, d, lo, hi) in enumerate(E):
        j = 48 * i + ax
        hand["origin"][j], hand["direction"][j], hand["range"][j] = o, d, (lo, hi)

    def aimed(n, first, dyadic):
        k = np.arange(first, first + n) % 48
        ai, aj, ak = q["axis_i"][k].astype(int), q["axis_j"][k].astype(int), q["axis_k"][k].astype(int)
        ri, rj, vk = q["range_i"][k], q["range_j"][k], q["value_k"][k]
        idx = np.arange(n)
        o, d = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        if dyadic:       # origins and directions on a dyadic grid around the exact squares: a, b, t land ON the bounds again and again
            ok = rs.choice([-1.0, 0.0, 3.0, 5.0], n).astype(F32)
            dk = rs.choice([-2.0, -1.0, 1.0, 2.0, 0.5], n).astype(F32)
            o[idx, ai], o[idx, aj], o[idx, ak] = rs.randint(-4, 21, n) * 0.25, rs.randint(-12, 13, n) * 0.25, ok
            d[idx, ai], d[idx, aj], d[idx, ak] = rs.randint(-4, 5, n) * 0.25, rs.randint(-4, 5, n) * 0.25, dk
            lo = rs.choice([FLT_MIN, 0.5, 1.0, 2.0], n).astype(F32); hi = rs.choice([FLT_MAX, 4.0, 2.0, 1.0], n).astype(F32)
            return po.pin_rays(o, d, lo, hi)
        a = ri["x"] + (ri["y"] - ri["x"]) * rs.uniform(-0.3, 1.3, n).astype(F32)
        b = rj["x"] + (rj["y"] - rj["x"]) * rs.uniform(-0.3, 1.3, n).astype(F32)
        target = np.zeros((n, 3), F32); target[idx, ai], target[idx, aj], target[idx, ak] = a, b, vk
        o = (target + rs.normal(0, 200, (n, 3))).astype(F32)
        d = unit(target - o) * np.where(rs.rand(n) < 0.3, pow10(rs, -3, 3, n), 1.0).astype(F32)[:, None]
        d = np.where(rs.rand(n, 1) < 0.1, -d, d)
        dist = np.linalg.norm(target - o, axis=1)
        hi = np.where(rs.rand(n) < 0.5, FLT_MAX, dist * rs.uniform(0.5, 1.5, n)).astype(F32)
        lo = np.where(rs.rand(n) < 0.8, FLT_MIN, dist * rs.uniform(0.0, 1.2, n)).astype(F32)
        return po.pin_rays(o, d.astype(F32), lo, hi)
    # the dyadic class runs on the three exact squares only: a batch whose item i uses square i % 48 with i % 48 < 3
    n_dy = 48 * 3000
    dy = aimed(n_dy, len(hand), True)
    keep = (np.arange(len(hand), len(hand) + n_dy) % 48) < 3
    dy["origin"][~keep] = 1e6
    seeded = aimed(N_SEEDED, len(hand) + n_dy, False)
    return carray(abi.Square, q), cat_rays(hand, dy, seeded), len(hand) + n_dy, [48 * i + e[0] for i, e in enumerate(E)]


# ---------------------------------------------------------------------------------------------------------------- triangle
def _triangles():
    rs = np.random.RandomState(301)
    n_tri = 96
    tv = np.zeros(3 * n_tri, dtype=np.dtype(abi.TriangleVertex))
    # triangle 0: the unit right triangle in z = 0, exact arithmetic; 1: the same, wound the other way; 2: a big dyadic one
    tv["v"][0:3] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    tv["v"][3:6] = [(0, 0, 0), (0, 1, 0), (1, 0, 0)]
    tv["v"][6:9] = [(-2, -2, 1), (6, -2, 1), (-2, 6, 1)]
    tv["v"][9:12] = [(0, 0, 0), (1, 1, 1), (2, 2, 2)]                              # 3: zero area (collinear)
    tv["v"][12:15] = [(1, 2, 3), (1, 2, 3), (4, 5, 6)]                             # 4: zero area (two vertices equal)
    tv["v"][15:18] = [(0, 0, 0), (1000, 0, 0), (500, 1e-4, 0)]                     # 5: a sliver
    tv["v"][18:21] = [(0, 0, 0), (1e-3, 0, 0), (0, 1e-3, 0)]                       # 6: tiny: det near FLT_EPSILON for unit directions
    for t in range(7, n_tri):
        base = rs.uniform(-300, 300, 3)
        ext = pow10(rs, -2, 2.3)
        tv["v"][3 * t:3 * t + 3] = (base + rs.normal(0, ext, (3, 3))).astype(F32)
    tv["n"] = (rs.normal(size=(3 * n_tri, 3)) * pow10(rs, -1, 1, (3 * n_tri, 1))).astype(F32)    # vertex normals not normalised
    tv["n"][0:3] = [(0, 0, 1), (0, 0, 2), (0, 0, 0.5)]
    tv["uv"] = rs.uniform(-1, 2, (3 * n_tri, 2)).astype(F32)
    tv["uv"][0:3] = [(0, 0), (1, 0), (0, 1)]
    return tv, n_tri


def _triangle_inputs():
    tv, n_tri = _triangles()
    rs = np.random.RandomState(302)
    E = []

    def edge(k, o, d, lo=FLT_MIN, hi=FLT_MAX):
        E.append((k, o, d, lo, hi))
    for kk in range(-2, 3):                                         # fabs(det) exactly FLT_EPSILON and 1, 2 ulp either side (det = -d.z)
        s = ulps(F32(FLT_EPS), kk)
        for tri in (0, 1):
            edge(tri, (0.25, 0.25, 1), (0, 0, -s)); edge(tri, (0.25, 0.25, -1), (0, 0, s))
            edge(tri, (0.25, 0.25, FLT_EPS), (0, 0, -s), FLT_MIN, FLT_MAX)
    for tri in (0, 1):
        for z, dz in ((1.0, -1.0), (-1.0, 1.0), (2.0, -0.5)):        # front, back-facing, not normalised; t = 1, 1, 4
            for kk in (-1, 0, 1):                                   # u == 0, v == 0, u == 1, v == 1, u + v == 1 and 1 ulp beyond each
                z0 = ulps(F32(0.0), kk) if kk else F32(0.0)
                edge(tri, (z0, 0.3, z), (0, 0, dz)); edge(tri, (0.3, z0, z), (0, 0, dz)); edge(tri, (z0, z0, z), (0, 0, dz))
                edge(tri, (ulps(F32(1.0), kk), 0, z), (0, 0, dz)); edge(tri, (0, ulps(F32(1.0), kk), z), (0, 0, dz))
                edge(tri, (ulps(F32(0.5), kk), 0.5, z), (0, 0, dz)); edge(tri, (0.25, ulps(F32(0.75), kk), z), (0, 0, dz))
                edge(tri, (ulps(F32(1.0), kk), -0.0, z), (0, 0, dz))
            t = F32(-z / dz)
            for lo, hi in ((t, FLT_MAX), (ulps(t, 1), FLT_MAX), (ulps(t, -1), FLT_MAX), (FLT_MIN, t), (FLT_MIN, ulps(t, -1)), (FLT_MIN, ulps(t, 1)), (t, t)):
                edge(tri, (0.25, 0.25, z), (0, 0, dz), lo, hi)       # t == range.x, t == range.y
    for tri in (3, 4):                                              # degenerate: det == 0
        for d in ((0, 0, -1), (1, -1, 0), (0.3, 0.2, -0.9)):
            edge(tri, (1, 1, 5), d)
    for x in (1.0, 250.0, 500.0, 999.0):                            # the sliver, straight on and grazing
        edge(5, (x, 5e-5, 1), (0, 0, -1)); edge(5, (x, 2e-5, 1), (0, 0, -1)); edge(5, (x, -50, 1e-3), (0, 1, 0))
    for d in ((0, 0, -1), (0, 0, 1), (0.6, 0, -0.8), (0, 1e-3, -1)):
        edge(6, (2e-4, 3e-4, 1), d); edge(6, (2e-4, 3e-4, -1), d)
    n_hand = len(E)
    hand = po.pin_rays(np.full((n_tri * n_hand, 3), 1e6, F32), np.tile(np.array([[1, 1, 1]], F32), (n_tri * n_hand, 1)), FLT_MIN, FLT_MAX)
    for i, (k, o, d, lo, hi) in enumerate(E):
        j = n_tri * i + k
        hand["origin"][j], hand["direction"][j], hand["range"][j] = o, d, (lo, hi)
    # dyadic grid over triangles 0..2: u, v, u + v, t exactly on their bounds again and again
    n_dy = n_tri * 3000
    first = len(hand)
    k = np.arange(first, first + n_dy) % n_tri
    o = np.stack([rs.randint(-8, 25, n_dy) * 0.25, rs.randint(-8, 25, n_dy) * 0.25, rs.choice([-1.0, 2.0, 3.0], n_dy)], 1).astype(F32)
    d = np.stack([rs.choice([0, 0, 0, 0.25, -0.5], n_dy), rs.choice([0, 0, 0, -0.25, 0.5], n_dy), rs.choice([-1.0, 1.0, -0.5, 2.0], n_dy)], 1).astype(F32)
    dy = po.pin_rays(o, d, rs.choice([FLT_MIN, 1.0, 2.0], n_dy).astype(F32), rs.choice([FLT_MAX, 4.0, 2.0, 1.0], n_dy).astype(F32))
    dy["origin"][k > 2] = 1e6
    # seeded: aimed at points of the triangle's plane around the triangle
    n = N_SEEDED
    first += n_dy
    k = np.arange(first, first + n) % n_tri
    V = tv["v"].reshape(n_tri, 3, 3)[k].astype(np.float64)
    bu, bv = rs.uniform(-0.3, 1.3, n), rs.uniform(-0.3, 1.3, n)
    target = V[:, 0] + bu[:, None] * (V[:, 1] - V[:, 0]) + bv[:, None] * (V[:, 2] - V[:, 0])
    size = np.linalg.norm(V[:, 1] - V[:, 0], axis=1) + np.linalg.norm(V[:, 2] - V[:, 0], axis=1) + 1e-3
    o = (target + unit(rs.normal(size=(n, 3))) * (size * rs.uniform(0.01, 5, n))[:, None]).astype(F32)
    d = unit(target - o) * np.where(rs.rand(n) < 0.3, pow10(rs, -3, 3, n), 1.0).astype(F32)[:, None]
    d = np.where(rs.rand(n, 1) < 0.1, -d, d)
    graze = rs.rand(n) < 0.1                                         # in the triangle's plane, nearly: det near 0
    d = np.where(graze[:, None], unit((V[:, 1] - V[:, 0]) * rs.uniform(-1, 1, (n, 1)) + (V[:, 2] - V[:, 0]) * rs.uniform(-1, 1, (n, 1))
                                      + rs.normal(0, 1e-6, (n, 3)) * size[:, None]), d)
    dist = np.linalg.norm(target - o, axis=1)
    hi = np.where(rs.rand(n) < 0.5, FLT_MAX, dist * rs.uniform(0.5, 1.5, n)).astype(F32)
    lo = np.where(rs.rand(n) < 0.8, FLT_MIN, dist * rs.uniform(0.0, 1.2, n)).astype(F32)
    seeded = po.pin_rays(o, d.astype(F32), lo, hi)
    return carray(abi.TriangleVertex, tv), cat_rays(hand, dy, seeded), len(hand) + n_dy, [n_tri * i + e[0] for i, e in enumerate(E)]


# ---------------------------------------------------------------------------------------------------------------- cube, AABB
def _matrix(m4, M):
    for col in range(4):
        for row in range(4):
            m4["columns"][col]["xyzw"[row]] = F32(M[row][col])


def _cubes():
    """unit boxes under model matrices as host.build_node(..., model=M) makes them for the Cornell blocks: scale, rotate about y,
    translate; inverse and inverse-transpose in float64, rounded once.  Cube 0 is the identity, cube 1 a dyadic scale + shift."""
    rs = np.random.RandomState(401)
    n = 32
    c = np.zeros(n, dtype=np.dtype(abi.Cube))
    for i in range(n):
        if i == 0:
            M = np.eye(4)
        elif i == 1:
            M = np.diag([2.0, 4.0, 0.5, 1.0]); M[:3, 3] = (-1.0, 8.0, 0.25)
        else:
            ang = rs.uniform(-np.pi, np.pi)
            ca, sa = math.cos(ang), math.sin(ang)
            R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
            if i % 4 == 3:                                           # some about a general axis
                ax = unit(rs.normal(size=3)).astype(np.float64); K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
                R = np.eye(3) + sa * K + (1 - ca) * (K[:, :, None] * K[None, :, :]).sum(1)
            sc = pow10(rs, -1, 2.5, 3)
            M = np.eye(4); M[:3, :3] = R * sc[None, :]; M[:3, 3] = rs.uniform(-300, 300, 3)
        # the inverse of (rotation x scale, translation) in closed form, elementwise: S^-1 R^T and -(S^-1 R^T) t
        L = M[:3, :3]
        s2 = (L * L).sum(0)
        Mi = np.eye(4); Mi[:3, :3] = L.T / s2[:, None]; Mi[:3, 3] = -(Mi[:3, :3] * M[:3, 3][None, :]).sum(1)
        _matrix(c["model_matrix"][i:i + 1][0], M); _matrix(c["inverse_matrix"][i:i + 1][0], Mi); _matrix(c["normal_matrix"][i:i + 1][0], Mi.T)
        c["box"]["maxi"]["x"][i] = c["box"]["maxi"]["y"][i] = c["box"]["maxi"]["z"][i] = 1.0
        c["material"][i] = i % 24
    return c


def _cube_models(c):
    M = np.zeros((len(c), 4, 4))
    for col in range(4):
        for row, nm in enumerate("xyzw"):
            M[:, row, col] = c["model_matrix"]["columns"][:, col][nm]
    return M


def _cube_inputs():
    c = _cubes()
    n_c = len(c)
    rs = np.random.RandomState(402)
    E = []

    def edge(k, o, d, lo=FLT_MIN, hi=FLT_MAX):
        E.append((k, o, d, lo, hi))
    g3 = F32(1) + F32(2) * ((F32(3) * FLT_EPS * F32(0.5)) / (F32(1) - F32(3) * FLT_EPS * F32(0.5)))        # 1 + 2 * gamma(3)
    for o in ((0.5, 0.5, 0.5), (0.25, 0.5, 0.75), (0.999, 0.001, 0.5)):                                   # origin inside
        for d in ((0, 0, 1), (0, -1, 0), (1, 1, 0), (1, 1, 1), (-0.0, 0.0, 1), (DENORM, -DENORM, 1), (0.6, 0, -0.8), (0, 0, 3)):
            edge(0, o, d)
            te = F32(F32(0.5) * g3)
            for hi in (te, ulps(te, 1), ulps(te, -1), F32(0.5), F32(0.25)):                                # te crosses tmax (inside: te < tmax picks the axis)
                edge(0, o, d, FLT_MIN, hi)
    for face in range(3):                                                                                 # origin exactly ON a face: all(ddd > 0) with one 0
        for v in (0.0, 1.0, -0.0):
            o = np.array([0.5, 0.25, 0.75], F32); o[face] = v
            for s in (1.0, -1.0):
                d = np.array([0.1, 0.2, 0.3], F32); d[face] = s
                edge(0, o, d); dd = np.zeros(3, F32); dd[face] = s; edge(0, o, dd)
                dd2 = np.array([0.0, -0.0, 0.0], F32); dd2[(face + 1) % 3] = 1.0; edge(0, o, dd2)         # sliding in the face plane
    for o, d in (((0.5, 0.5, -2), (0, 0, 1)), ((0.5, 0.5, 3), (0, 0, -1)), ((-2, 0.5, 0.5), (1, 0, 0)), ((0.5, 4, 0.5), (0, -2, 0))):
        t = F32(np.abs(np.array(o, F32) - np.clip(np.array(o, F32), 0, 1)).sum())                          # axis-aligned: distance is exact
        for hi in (FLT_MAX, t, ulps(t, 1), ulps(t, -1), F32(t * g3)):                                      # _record.t >= range_t.y with equality
            edge(0, o, d, FLT_MIN, hi)
        for dz in (0.0, -0.0, DENORM, -DENORM):                                                           # direction components +-0, denormal
            dd = np.array(d, F32); dd[dd == 0] = dz; edge(0, o, dd)
    for o, d in (((-1, -1, 0.5), (1, 1, 0)), ((-1, -1, -1), (1, 1, 1)), ((2, 2, 0.5), (-1, -1, 0)), ((2, 2, 2), (-1, -1, -1)), ((-1, 0.5, -1), (1, 0, 1)),
                 ((-0.5, -1, 0.5), (0.5, 1, 0)), ((0.5, 0.5, 0.5), (1, 1, 1)), ((0.5, 0.5, 0.5), (-1, -1, 0))):
        edge(0, o, d)                                                                                      # ties in axisPick: through an edge / a corner
    for o, d in (((0, 9, 0.5), (0, 1, 0)), ((0, 30, 0.5), (0, -1, 0)), ((-3, 10, 0.5), (1, 0, 0)), ((0, 10, 0.5), (0.0, 1, 0)), ((-1, 8, 0.25), (1, 1, 0.125))):
        edge(1, o, d)                                                                                      # the dyadic cube: exact object-space arithmetic
    n_hand = len(E)
    hand = po.pin_rays(np.full((n_c * n_hand, 3), 1e6, F32), np.tile(np.array([[1, 1, 1]], F32), (n_c * n_hand, 1)), FLT_MIN, FLT_MAX)
    for i, (k, o, d, lo, hi) in enumerate(E):
        j = n_c * i + k
        hand["origin"][j], hand["direction"][j], hand["range"][j] = o, d, (lo, hi)
    # dyadic grid around cubes 0 and 1
    n_dy = n_c * 4000
    first = len(hand)
    k = np.arange(first, first + n_dy) % n_c
    o = (rs.randint(-8, 13, (n_dy, 3)) * 0.25).astype(F32)
    o[k == 1] = o[k == 1] * F32(4.0) + np.array([0, 8, 0], F32)
    d = rs.choice([0.0, 0.0, 1.0, -1.0, 0.5, -2.0], (n_dy, 3)).astype(F32)
    d[(d == 0).all(1)] = (0, 0, 1)
    dy = po.pin_rays(o, d, FLT_MIN, rs.choice([FLT_MAX, 0.5, 1.0, 2.0, 4.0], n_dy).astype(F32))
    dy["origin"][k > 1] = 1e6
    # seeded: world-space rays at the posed cubes, origins outside and inside
    n = N_SEEDED
    first += n_dy
    k = np.arange(first, first + n) % n_c
    M = _cube_models(c)[k]
    local = rs.uniform(-0.3, 1.3, (n, 3))
    target = mat3_vec(M[:, :3, :3], local) + M[:, :3, 3]
    size = np.linalg.norm(M[:, :3, :3], axis=(1, 2))
    inside = rs.rand(n) < 0.35
    lo_in = rs.uniform(0.001, 0.999, (n, 3))
    o_in = mat3_vec(M[:, :3, :3], lo_in) + M[:, :3, 3]
    o_out = target + unit(rs.normal(size=(n, 3))) * (size * rs.uniform(0.05, 4, n))[:, None]
    o = np.where(inside[:, None], o_in, o_out).astype(F32)
    d = np.where(inside[:, None], unit(rs.normal(size=(n, 3))), unit(target - o))
    d = (d * np.where(rs.rand(n) < 0.3, pow10(rs, -3, 3, n), 1.0)[:, None]).astype(F32)
    zero = rs.rand(n) < 0.05
    d[zero, rs.randint(0, 3, zero.sum())] = rs.choice([0.0, -0.0, float(DENORM)], zero.sum())
    dist = np.linalg.norm(target - o, axis=1)
    hi = np.where(rs.rand(n) < 0.5, FLT_MAX, dist * rs.uniform(0.2, 1.5, n)).astype(F32)
    seeded = po.pin_rays(o, d, FLT_MIN, hi)
    return carray(abi.Cube, c), cat_rays(hand, dy, seeded), len(hand) + n_dy, [n_c * i + e[0] for i, e in enumerate(E)]


def _aabb_inputs():
    rs = np.random.RandomState(501)
    n_b = 40
    b = np.zeros(n_b, dtype=np.dtype(abi.AABB))
    lo = rs.uniform(-300, 300, (n_b, 3)).astype(F32); ext = (pow10(rs, -2, 2.5, (n_b, 3))).astype(F32)
    lo[0], ext[0] = (0, 0, 0), (1, 1, 1)                             # box 0: the unit box; 1: zero thickness in y; 2: a point; 3: dyadic
    lo[1], ext[1] = (0, 2, 0), (4, 0, 4)
    lo[2], ext[2] = (1, 1, 1), (0, 0, 0)
    lo[3], ext[3] = (-2, -4, 8), (4, 2, 1)
    for i, nm in enumerate("xyz"):
        b["mini"][nm], b["maxi"][nm] = lo[:, i], lo[:, i] + ext[:, i]
    E = []

    def edge(k, o, d, lo_=FLT_MIN, hi_=FLT_MAX):
        E.append((k, o, d, lo_, hi_))
    for o, d in (((0.5, 0.5, 3), (0, 0, 1)), ((0.5, 0.5, 3), (0.01, 0, 1)), ((4, 4, 4), (1, 1, 1))):          # tmax < 0: the box lies behind
        edge(0, o, d); edge(0, o, d, -FLT_MAX, FLT_MAX)
    for d in ((0, 0, 1), (1, 1, 1), (-1, 0.5, 0.25), (0, -0.0, 1), (DENORM, 0, -1)):                            # tmin < 0 <= tmax: origin inside
        edge(0, (0.5, 0.5, 0.5), d); edge(0, (0.5, 0.5, 0.5), d, FLT_MIN, 0.25); edge(0, (0.5, 0.5, 0.5), d, 0.75, FLT_MAX)
    for o, d in (((2, 5, 2), (0, -1, 0)), ((2, 5, 2), (0.1, -1, 0.1)), ((2, 2, -3), (0, 0, 1)), ((2, 2, -3), (0, 0.0, 1)), ((-1, 2, 2), (1, -0.0, 0)),
                 ((2, ulps(F32(2.0), 1), -3), (0, 0, 1)), ((2, 2, 2), (0, 1, 0)), ((2, 2, 2), (0, 0, 1))):
        edge(1, o, d)                                                                                          # zero-thickness box, and a ray IN its plane
    for o, d in (((1, 1, -1), (0, 0, 1)), ((0, 0, 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 1)), ((1, 1, 1), (0, 0, 0))):
        edge(2, o, d)                                                                                          # the point box
    for face in range(3):                                                                                     # ray in a face plane: 0 * inf = NaN through fmin / fmax
        for v in (0.0, 1.0):
            for zero in (0.0, -0.0):
                o = np.array([0.5, 0.5, 0.5], F32); o[face] = v; o[(face + 1) % 3] = -2.0
                d = np.array([zero, zero, zero], F32); d[(face + 1) % 3] = 1.0
                edge(0, o, d); edge(0, o, -d)
                d2 = d.copy(); d2[(face + 2) % 3] = 0.5; edge(0, o, d2)
    for o, d in (((0, -3, 8.5), (0, 1, 0)), ((0, -3, 8.5), (0, 2, 0)), ((-6, -3, 8.5), (2, 0, 0)), ((0, -3, 7), (0, 0, 1)), ((0, -3, 10), (0, 0, -1))):
        for hi_ in (FLT_MAX, 1.0, 2.0, 0.5, ulps(F32(1.0), -1)):                                               # entry t exactly range_t.y, range_t.x
            edge(3, o, d, FLT_MIN, hi_); edge(3, o, d, hi_ if hi_ != FLT_MAX else FLT_MIN, FLT_MAX)
    n_hand = len(E)
    hand = po.pin_rays(np.full((n_b * n_hand, 3), 1e6, F32), np.tile(np.array([[1, 1, 1]], F32), (n_b * n_hand, 1)), FLT_MIN, FLT_MAX)
    for i, (k, o, d, lo_, hi_) in enumerate(E):
        j = n_b * i + k
        hand["origin"][j], hand["direction"][j], hand["range"][j] = o, d, (lo_, hi_)
    n_dy = n_b * 3000
    first = len(hand)
    k = np.arange(first, first + n_dy) % n_b
    o = (rs.randint(-8, 13, (n_dy, 3)) * 0.25).astype(F32)
    o[k == 3] = o[k == 3] * F32(4) + np.array([0, 0, 8], F32)
    d = rs.choice([0.0, -0.0, 1.0, -1.0, 0.5, -2.0], (n_dy, 3)).astype(F32)
    dy = po.pin_rays(o, d, rs.choice([FLT_MIN, 0.5, 1.0], n_dy).astype(F32), rs.choice([FLT_MAX, 0.5, 1.0, 2.0, 4.0], n_dy).astype(F32))
    dy["origin"][(k != 0) & (k != 3) & (k != 1)] = 1e6
    n = N_SEEDED
    first += n_dy
    k = np.arange(first, first + n) % n_b
    target = lo[k] + ext[k] * rs.uniform(-0.3, 1.3, (n, 3))
    size = np.linalg.norm(ext[k], axis=1) + 1e-2
    inside = rs.rand(n) < 0.3
    o = np.where(inside[:, None], lo[k] + ext[k] * rs.uniform(0, 1, (n, 3)), target + unit(rs.normal(size=(n, 3))) * (size * rs.uniform(0.05, 4, n))[:, None]).astype(F32)
    d = np.where(inside[:, None], unit(rs.normal(size=(n, 3))), unit(target - o))
    d = (d * np.where(rs.rand(n) < 0.3, pow10(rs, -3, 3, n), 1.0)[:, None]).astype(F32)
    d = np.where(rs.rand(n, 1) < 0.15, -d, d)
    zero = rs.rand(n) < 0.05
    d[zero, rs.randint(0, 3, zero.sum())] = rs.choice([0.0, -0.0, float(DENORM)], zero.sum())
    dist = np.linalg.norm(target - o, axis=1)
    hi = np.where(rs.rand(n) < 0.5, FLT_MAX, dist * rs.uniform(0.2, 1.5, n)).astype(F32)
    seeded = po.pin_rays(o, d, FLT_MIN, hi)                          # range_t.x = FLT_MIN, as the walk passes it
    return carray(abi.AABB, b), cat_rays(hand, dy, seeded), len(hand) + n_dy, [n_b * i + e[0] for i, e in enumerate(E)]


# ---------------------------------------------------------------------------------------------------------------- lights, math, sampling
def _edge_u():
    vals = [0.0, 1.0, float(ONE_BELOW), 0.5, 0.25, float(ulps(F32(0.5), -1)), float(ulps(F32(0.5), 1)), float(ulps(F32(0.25), -1)), 1e-7, 1e-6, 0.75]
    return np.array([(a, b) for a in vals for b in vals], F32)


def _uu(rs, n):
    return np.concatenate([_edge_u(), rs.uniform(0, 1, (n, 2)).astype(F32)]), len(_edge_u())


def _dirs_edge():
    """direction pairs (wo, wi / wh) for the lobes: z = +-0, grazing 1e-4, equal, opposite, wrong hemisphere, along the axes"""
    g = F32(1e-4)
    base = [(0, 0, 1), (0, 0, -1), (1, 0, 0.0), (1, 0, -0.0), (0, 1, 0.0), (0.6, 0, 0.8), (0.6, 0, -0.8), (0, -0.8, 0.6)]
    base += [tuple(unit((1, 0, s * g))) for s in (1, -1)] + [tuple(unit((0.3, -0.4, s * g))) for s in (1, -1)]
    base += [tuple(unit(v)) for v in ((1, 1, 1), (-1, 2, 0.5), (0.1, 0.1, -1), (0.01, 0, 1), (1e-4, 0, 1))]
    base += [(0.3, 0.4, 0.5), (0, 0, 2), (0, 0, 0)]                               # not unit, and null
    wo, wi = [], []
    for a in base:
        for b in base:
            wo.append(a); wi.append(b)
        wo.append(a); wi.append(tuple(-np.array(a, F32)))                        # wo == -wi
        wo.append(a); wi.append((-a[0], -a[1], a[2]))                             # the mirror direction
    return np.array(wo, F32), np.array(wi, F32)


def _material(mtype, tex=abi.TEX_CONSTANT):
    m = abi.Material()
    m.type, m.eta, m.roughness = mtype, 1.5, 0.5
    m.textureInfo.type = tex
    m.textureInfo.albedo.x, m.textureInfo.albedo.y, m.textureInfo.albedo.z = 0.73, 0.4, 0.2
    return m


MATERIALS = OrderedDict([("lambert", (abi.MAT_LAMBERT, abi.TEX_CONSTANT)), ("metal", (abi.MAT_METAL, abi.TEX_CONSTANT)),
                         ("plastic", (abi.MAT_PLASTIC, abi.TEX_CONSTANT)), ("glass", (abi.MAT_GLASS, abi.TEX_CONSTANT)),
                         ("lambert_checker", (abi.MAT_LAMBERT, abi.TEX_CHECKER)), ("glass_checker", (abi.MAT_GLASS, abi.TEX_CHECKER)),
                         ("diffuse", (abi.MAT_DIFFUSE, abi.TEX_CONSTANT)), ("nil", (abi.MAT_NIL, abi.TEX_CONSTANT))])


def _lobe_inputs(seed):
    rs = np.random.RandomState(seed)
    wo_e, wi_e = _dirs_edge()
    uu_e = _edge_u()
    # edges: every direction pair with a handful of uu, and every uu pair with a handful of directions
    pick_u = uu_e[rs.randint(0, len(uu_e), (len(wo_e), 2))]
    wo1, wi1, uu1 = np.repeat(wo_e, 2, 0), np.repeat(wi_e, 2, 0), pick_u.reshape(-1, 2)
    pick_d = rs.randint(0, len(wo_e), (len(uu_e), 3))
    wo2, wi2, uu2 = wo_e[pick_d].reshape(-1, 3), wi_e[pick_d].reshape(-1, 3), np.repeat(uu_e, 3, 0)
    n_edge = len(wo1) + len(wo2)
    n = N_SEEDED
    wo = unit(rs.normal(size=(n, 3)))
    wi = unit(rs.normal(size=(n, 3)))
    k = rs.rand(n)
    wi = np.where((k < 0.25)[:, None], wo * np.array([-1, -1, 1], F32) + rs.normal(0, 0.02, (n, 3)).astype(F32), wi)     # near the mirror direction
    wi = np.where(((k >= 0.25) & (k < 0.4))[:, None], unit(-wo.astype(np.float64) / 1.5 + rs.normal(0, 0.05, (n, 3))), wi)  # near a refraction
    graz = rs.rand(n) < 0.1
    wo[graz, 2] = (rs.choice([-1, 1], graz.sum()) * pow10(rs, -6, -2, graz.sum())).astype(F32)
    uu = rs.uniform(0, 1, (n, 2)).astype(F32)
    uv = rs.uniform(-0.5, 1.5, (n_edge + n, 2)).astype(F32)
    return (np.concatenate([wo1, wo2, wo]).astype(F32), np.concatenate([wi1, wi2, wi.astype(F32)]).astype(F32), uv,
            np.concatenate([uu1, uu2, uu]).astype(F32), n_edge)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _hit_case(kind, make, excluded):
    def run(pin):
        prims, rays = cached(kind, make)[:2]
        return rec_fields(pin.hit(kind, prims, rays))
    n_edge, hand = cached(kind, make)[2:]
    # the hand-made rays stand between fillers (item i uses primitive i % n_prim): keep those, not the fillers
    return Case(n_edge, run, excluded, np.concatenate([hand, np.arange(n_edge, n_edge + N_STORED)]).astype(np.int64))


def _scene_views():
    """name -> (scene view, keep-alive, rays): the three scenes of the GPU traversal test and the adversarial seeds 1-6"""
    def make():
        from conftest import random_rays, camera_rays
        from tracer_amd import host
        import test_gpu_traversal as tg
        out = OrderedDict()
        for name, hs in (("cornell_spheres", host.HostScene(abi.SCENE_CORNELL_SPHERES)),
                         ("ball_mesh_scene", host.HostScene(abi.SCENE_CORNELL_MESH, host.Mesh.ball(50, 50, 0.08)))):
            rays = np.concatenate([random_rays(3072, 31), random_rays(3072, 32, inside_only=True),
                                   camera_rays(host.prepare_camera(64, 32), 64, 32)])
            assert len(rays) == N_SCENE_RAYS
            out[name] = (hs.view, hs, rays)
        for seed in range(1, 7):
            rs = np.random.RandomState(7000 + seed)
            sv, keep, targets = tg.adversarial_scene(rs)
            rays = tg.adversarial_rays(rs, targets)
            rays = np.ascontiguousarray(rays[np.random.RandomState(seed).permutation(len(rays))[:N_SCENE_RAYS]])
            out[f"adversarial_{seed}"] = (sv, keep, rays)
        return out
    return cached("scenes", make)


SCENE_NAMES = ["cornell_spheres", "ball_mesh_scene"] + [f"adversarial_{s}" for s in range(1, 7)]
GPU_SCENES = ["cornell_spheres", "ball_mesh_scene", "adversarial_1"]


def shadow_rays(name, rays, closest_t, closest_accepted):
    """any-hit rays of a scene: tmax == t of the closest hit for every other ray that hit (Square / Triangle::hit_test accept
    t == range_t.y and Scene::hit still answers range_t.y < test_t = false), 1 ulp short of and beyond it for some, seeded else"""
    rs = np.random.RandomState(sum(map(ord, name)))
    s = rays.copy()
    s["tmax"] = rs.uniform(1.0, 900.0 if not name.startswith("adv") else 160.0, len(rays)).astype(F32)
    i = np.arange(len(rays))
    hit = closest_accepted != 0
    s["tmax"] = np.where(hit & (i % 2 == 0), closest_t, s["tmax"])
    s["tmax"] = np.where(hit & (i % 8 == 1), ulps(closest_t, 1), s["tmax"])
    s["tmax"] = np.where(hit & (i % 8 == 3), ulps(closest_t, -1), s["tmax"])
    return s


def _scene_case(name, any_hit):
    def run(pin):
        sv, _, rays = _scene_views()[name]
        closest = pin.scene_hit(sv, rays)
        if not any_hit:
            return rec_fields(closest)
        # the closest t is this family's own: where the two families differ there, the closest case fails first
        return rec_fields(pin.scene_hit(sv, shadow_rays(name, rays, closest["t"], closest["accepted"]), any_hit=True))
    # whole outputs are kept for the scenes the GPU test uploads; the other adversarial seeds are held by their CRC alone (file size)
    return Case(0, run, SCENE_EXCLUDED, None if name in GPU_SCENES else np.arange(0))


TRC_VIEW_OF_SCENE_BITS = slice(0, 14)      # canonical(scene case): accepted t p[3] gn[3] sn[3] uv[2] material | f


def trc_view(accepted, rec):
    """a record as trc_hit reports it (oracle.cpp fill_hit, trc_trace_rays): the answer, and the record only where the answer is yes"""
    hit = np.asarray(accepted) != 0
    out = OrderedDict([("hit", hit.astype(np.int32))])
    for f in ("t", "p", "gn", "sn", "uv", "material"):
        a = np.ascontiguousarray(rec[f])
        out[f] = np.where(hit.reshape((-1,) + (1,) * (a.ndim - 1)), a, np.zeros((), a.dtype))
    return out


# Fields a hit_test leaves unwritten, by primitive type: the table of tests/test_reference_pin.py (reasons and line numbers there)
EXCLUDED = {"sphere": {"PDF"}, "square": set(), "cube": {"PDF"}, "triangle": {"PDF"}, "aabb_record": {"sn", "f", "material", "PDF"}}
SCENE_EXCLUDED = {"PDF", "range_y"}


def build_cases():
    cases = OrderedDict()
    cases["sphere"] = _hit_case("sphere", _sphere_inputs, EXCLUDED["sphere"])
    cases["square"] = _hit_case("square", _square_inputs, EXCLUDED["square"])
    cases["triangle"] = _hit_case("triangle", _triangle_inputs, EXCLUDED["triangle"])
    cases["cube"] = _hit_case("cube", _cube_inputs, EXCLUDED["cube"])
    cases["aabb_record"] = _hit_case("aabb_record", _aabb_inputs, EXCLUDED["aabb_record"])
    n_aabb = cached("aabb_record", _aabb_inputs)[2]

    def aabb(pin):
        boxes, rays = cached("aabb_record", _aabb_inputs)[:2]
        h, t = pin.aabb_hit_t(boxes, rays)
        return {"hit": pin.aabb_hit(boxes, rays), "hit_t": h, "t": t}
    cases["aabb"] = Case(n_aabb, aabb, stored=cases["aabb_record"].stored)
    for name in SCENE_NAMES:
        cases[f"scene_{name}"] = _scene_case(name, False)
        cases[f"scene_any_{name}"] = _scene_case(name, True)

    # --- light samplers
    def sq_sample_in():
        rs = np.random.RandomState(601)
        q = _squares()
        u, n_e = _uu(rs, N_SEEDED)
        n_e *= 3
        u = np.concatenate([np.repeat(_edge_u(), 3, 0), u[len(_edge_u()):]])
        pos = rs.uniform(-400, 400, (len(u), 3)).astype(F32)
        k = np.arange(len(u)) % 48
        onplane = np.arange(len(u)) % 5 == 0                        # pos ON the square's plane: dot(w, n) = +-0 into copysign
        pos[onplane, q["axis_k"][k][onplane].astype(int)] = q["value_k"][k][onplane]
        return carray(abi.Square, q), u, pos, n_e
    n_e = cached("sq_sample", sq_sample_in)[3]
    cases["square_sample"] = Case(n_e, lambda pin: {"out": pin.square_sample(*cached("sq_sample", sq_sample_in)[:3])})

    def tri_sample_in():
        rs = np.random.RandomState(602)
        tv, n_tri = _triangles()
        u = np.concatenate([np.repeat(_edge_u(), 3, 0), rs.uniform(0, 1, (N_SEEDED, 2)).astype(F32)])
        return carray(abi.TriangleVertex, tv), u, 3 * len(_edge_u())
    cases["triangle_sample"] = Case(cached("tri_sample", tri_sample_in)[2], lambda pin: {"out": pin.triangle_sample(*cached("tri_sample", tri_sample_in)[:2])})

    def tri_area_in():
        rs = np.random.RandomState(603)
        tv, n_tri = _triangles()
        n = N_SEEDED
        big = np.zeros(3 * (n_tri + n), dtype=tv.dtype)
        big[:3 * n_tri] = tv
        base = rs.uniform(-300, 300, (n, 1, 3)); ext = pow10(rs, -4, 2.5, (n, 1, 1))
        big["v"][3 * n_tri:] = (base + rs.normal(0, 1, (n, 3, 3)) * ext).astype(F32).reshape(-1, 3)
        return carray(abi.TriangleVertex, big), n_tri
    cases["triangle_area"] = Case(cached("tri_area", tri_area_in)[1], lambda pin: {"out": pin.triangle_area(cached("tri_area", tri_area_in)[0])})

    # --- Math.hh
    def offset_in():
        rs = np.random.RandomState(701)
        b = F32(1 / 32)
        vals = [0.0, -0.0, float(b), -float(b), float(ulps(b, -1)), float(ulps(b, 1)), -float(ulps(b, -1)), -float(ulps(b, 1)), 1e-3, -1e-3,
                float(DENORM), -float(DENORM), 1.0, -1.0, 555.0, -555.0, 1e-30, float(FLT_MAX) / 4]
        pe = np.array([(a, b_, c) for a in vals for b_ in vals[:8] for c in vals[8:12]], F32)
        ne = np.tile(np.array([(0, 0, 1), (0, -1, 0), (1, 0, 0), (-0.6, 0, 0.8), (0.577, 0.577, -0.577), (0, 0, -1)], F32), (len(pe) // 6 + 1, 1))[:len(pe)]
        n = N_SEEDED
        p = (rs.choice([-1, 1], (n, 3)) * pow10(rs, -4, 3, (n, 3))).astype(F32)
        near = rs.rand(n, 3) < 0.15
        p = np.where(near, ulps(np.where(rs.rand(n, 3) < 0.5, b, -b).astype(F32), rs.randint(-3, 4, (n, 3))), p).astype(F32)
        nn = unit(rs.normal(size=(n, 3)))
        axis = rs.rand(n) < 0.3
        nn[axis] = np.eye(3, dtype=F32)[rs.randint(0, 3, axis.sum())] * rs.choice([-1, 1], (axis.sum(), 1)).astype(F32)
        return np.concatenate([pe, p]), np.concatenate([ne, nn]), len(pe)
    cases["offset_ray"] = Case(cached("offset", offset_in)[2], lambda pin: {"out": pin.map("offset_ray_n", 3, *cached("offset", offset_in)[:2])})

    def scalar_in():
        rs = np.random.RandomState(702)
        inf = np.inf
        e = [0.0, -0.0, inf, -inf, float(DENORM), -float(DENORM), 1e-45, -1e-45, float(FLT_MIN), -float(FLT_MIN), float(FLT_MAX), -float(FLT_MAX), 1.0, -1.0,
             float(ulps(F32(1.0), -1)), np.nan, 0.99999, -0.99999, float(ulps(F32(0.99999), 1)), float(ulps(F32(0.99999), -1)), 1.5, -1.5, 0.5, -0.5]
        x5 = F32(math.sqrt(1 - math.exp(-5.0)))                         # ErfInv's w == 5: -log((1 - x)(1 + x)) = 5
        e += [float(ulps(x5, k)) for k in range(-200, 201)] + [-float(ulps(x5, k)) for k in range(-200, 201, 7)]
        e = np.array(e, F32)
        n = N_SEEDED
        x = np.concatenate([rs.uniform(-1, 1, n // 2), rs.normal(0, 3, n // 4), rs.choice([-1, 1], n // 4) * pow10(rs, -44, 38, n // 4)]).astype(F32)
        return np.concatenate([e, x]), len(e)
    n_e = cached("scalar", scalar_in)[1]
    for fn in ("next_float_up", "next_float_down", "erf_n", "erfinv_n"):
        cases[fn.replace("_n", "")] = Case(n_e, lambda pin, fn=fn: {"out": pin.map(fn, 1, cached("scalar", scalar_in)[0])})
    cases["gamma"] = Case(8, lambda pin: {"out": np.array([pin.gamma(n) for n in range(1, 9)], F32)})

    # --- Sampling.hh, HitRecord.hh
    def u_in():
        return _uu(np.random.RandomState(801), N_SEEDED)
    n_e = cached("u", u_in)[1]
    for fn, w in (("cosine_sample_hemisphere_n", 3), ("concentric_sample_disk", 2), ("uniform_sample_triangle", 2)):
        cases[fn.replace("_n", "")] = Case(n_e, lambda pin, fn=fn, w=w: {"out": pin.map(fn, w, cached("u", u_in)[0])})

    def pdf_in():
        rs = np.random.RandomState(802)
        vals = np.array([0.0, -0.0, 1.0, 1e-30, 1e30, np.inf, 1e-20, 0.5, 3e38, np.nan], F32)
        e = np.array([(a, b) for a in vals for b in vals], F32)
        x = (pow10(rs, -25, 25, (N_SEEDED, 2))).astype(F32)
        z = rs.rand(N_SEEDED, 2) < 0.05
        x[z] = 0
        return np.concatenate([e, x]), len(e)
    cases["power_heuristic"] = Case(cached("pdf", pdf_in)[1], lambda pin: {"out": np.concatenate(
        [pin.power_heuristic(nf, cached("pdf", pdf_in)[0][:, 0], ng, cached("pdf", pdf_in)[0][:, 1]) for nf, ng in ((1, 1), (2, 1), (1, 4))], 1)})

    def vec_in():
        rs = np.random.RandomState(803)
        e, _ = _dirs_edge()
        e = np.concatenate([e[::len(e) // 60], np.array([(1, 1, 0), (1, -1, 0), (-0.0, 0.0, 1), (0, 0, 0), (1e-30, 1e-30, 0), (3, 4, 0)], F32)])
        v = unit(rs.normal(size=(N_SEEDED, 3)))
        tie = rs.rand(N_SEEDED) < 0.05
        v[tie, 1] = v[tie, 0] * rs.choice([-1, 1], tie.sum()).astype(F32)          # abs(a.x) == abs(a.y)
        return np.concatenate([e, v]).astype(F32), len(e)
    cases["coordinate_system"] = Case(cached("vec", vec_in)[1], lambda pin: {"out": pin.map("coordinate_system", 6, cached("vec", vec_in)[0])})

    def sph_in():
        rs = np.random.RandomState(804)
        n = N_SEEDED + 64
        ct = rs.uniform(-1, 1, n).astype(F32)
        ct[:64] = np.resize(np.array([1, -1, 0, -0.0, 0.5, float(ONE_BELOW)], F32), 64)
        st = np.sqrt(np.maximum(F32(0), F32(1) - ct * ct)).astype(F32)
        phi = rs.uniform(0, 2 * np.pi, n).astype(F32)
        phi[:64] = np.resize(np.array([0, np.pi, 2 * np.pi, np.pi / 2, -0.0, 1e-30, 6.2831855], F32), 64)
        xyz = np.concatenate([unit(rs.normal(size=(n, 3))), unit(rs.normal(size=(n, 3))), unit(rs.normal(size=(n, 3)))], 1).astype(F32)
        return np.stack([st, ct, phi], 1), xyz, 64
    cases["spherical_direction"] = Case(64, lambda pin: {"out": pin.map("spherical_direction", 3, *cached("sph", sph_in)[:2])})

    def hg_in():
        rs = np.random.RandomState(805)
        ge = np.array([0.0, -0.0, 1e-3, -1e-3, float(ulps(F32(1e-3), -1)), float(ulps(F32(1e-3), 1)), 0.5, -0.5, 0.999, -0.999, 1.0, -1.0, 0.877], F32)
        ue = _edge_u()
        g = np.concatenate([np.repeat(ge, len(ue)), rs.uniform(-0.99, 0.99, N_SEEDED).astype(F32)])
        small = rs.rand(len(g)) < 0.05
        g = np.where(small & (np.arange(len(g)) >= len(ge) * len(ue)), (rs.uniform(-2e-3, 2e-3, len(g))).astype(F32), g).astype(F32)
        uu = np.concatenate([np.tile(ue, (len(ge), 1)), rs.uniform(0, 1, (N_SEEDED, 2)).astype(F32)])
        wo = unit(rs.normal(size=(len(g), 3)))
        wo[:len(ge) * len(ue):3] = (0, 0, 1); wo[1:len(ge) * len(ue):3] = (1, 0, 0)
        ct = np.concatenate([np.resize(np.array([1, -1, 0, 0.5, -0.5, float(ONE_BELOW)], F32), len(ge) * len(ue)), rs.uniform(-1, 1, N_SEEDED).astype(F32)])
        return g, wo, uu, ct, len(ge) * len(ue)
    n_e = cached("hg", hg_in)[4]
    cases["phase_hg"] = Case(n_e, lambda pin: {"out": pin.map("phase_hg_n", 1, cached("hg", hg_in)[3], cached("hg", hg_in)[0])})
    cases["hg_sample"] = Case(n_e, lambda pin: {"out": pin.map("hg_sample_n", 4, *cached("hg", hg_in)[:3])})

    # --- Fresnel, Reflect, Refract
    def fr_in():
        rs = np.random.RandomState(901)
        crit = F32(np.sqrt(1 - 1 / 1.5 ** 2))                        # cos of the critical angle leaving eta = 1.5
        ce = [0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e-4, -1e-4, 1e-20, 0.5, -0.5] + [float(ulps(crit, k)) for k in range(-40, 41)] + [-float(ulps(crit, k)) for k in range(-40, 41)]
        ee = [1.0, 1.5, 1 / 1.5, 1.33, 2.4, 1e-3, 1e3, float(ulps(F32(1.0), 1)), float(ulps(F32(1.0), -1))]
        e = np.array([(c, et) for c in ce for et in ee], F32)
        n = N_SEEDED
        c = rs.uniform(-1, 1, n).astype(F32)
        et = np.where(rs.rand(n) < 0.5, 1.5, rs.uniform(0.3, 3, n)).astype(F32)
        near = rs.rand(n) < 0.2
        with np.errstate(invalid="ignore"):
            cc = np.sqrt(np.maximum(0, 1 - 1 / et.astype(np.float64) ** 2))
        c = np.where(near, -ulps(cc.astype(F32), rs.randint(-50, 51, n)), c).astype(F32)
        return np.concatenate([e[:, 0], c]), np.concatenate([e[:, 1], et]), len(e)
    n_e = cached("fr", fr_in)[2]
    cases["fr_dielectric"] = Case(n_e, lambda pin: {"out": pin.map("fr_dielectric_n", 1, *cached("fr", fr_in)[:2])})

    def frc_in():
        rs = np.random.RandomState(902)
        n = N_SEEDED + 32
        c = rs.uniform(0, 1, n).astype(F32)
        c[:32] = np.resize(np.array([0, 1, 1e-4, 0.5, -0.5, 1e-20, -0.0, 2.0], F32), 32)
        eta = rs.uniform(0.05, 4, (n, 3)).astype(F32); k = rs.uniform(0, 8, (n, 3)).astype(F32)
        eta[:32:2] = (0.18, 0.15, 0.81); k[:32:2] = (1, 1, 1)       # createMetalMaterial's
        k[1:32:4] = 0
        return c, eta, k, 32
    cases["fr_conductor"] = Case(32, lambda pin: {"out": pin.map("fr_conductor_n", 3, *cached("frc", frc_in)[:3])})

    def refl_in():
        rs = np.random.RandomState(903)
        wo_e, wi_e = _dirs_edge()
        crit = np.sqrt(1 - 1 / 1.5 ** 2)
        n = N_SEEDED
        wo = unit(rs.normal(size=(n, 3))); nn = unit(rs.normal(size=(n, 3)))
        nn = np.where((rs.rand(n) < 0.5)[:, None], unit(wo + rs.normal(0, 0.3, (n, 3))), nn)
        eta = np.where(rs.rand(n) < 0.5, rs.choice([1.5, 1 / 1.5]), rs.uniform(0.3, 3, n)).astype(F32)
        near = rs.rand(n) < 0.2                                      # total internal reflection exactly at and around the critical angle
        z = ulps(np.full(n, crit, F32), rs.randint(-50, 51, n))
        xy = unit(np.concatenate([rs.normal(size=(n, 2)), np.zeros((n, 1))], 1)) * np.sqrt(np.maximum(0, 1 - z.astype(np.float64) ** 2))[:, None]
        wo = np.where(near[:, None], xy.astype(F32) + np.stack([0 * z, 0 * z, z * rs.choice([-1, 1], n)], 1), wo).astype(F32)
        eta = np.where(near, 1.5, eta).astype(F32)
        ee = np.resize(np.array([1.0, 1.5, 1 / 1.5, 0.0, 1e3], F32), len(wo_e))
        return np.concatenate([wo_e, wo]), np.concatenate([wi_e, nn]).astype(F32), np.concatenate([ee, eta]), len(wo_e)
    n_e = cached("refl", refl_in)[3]
    cases["reflect"] = Case(n_e, lambda pin: {"out": pin.map("reflect", 3, *cached("refl", refl_in)[:2])})
    cases["refract"] = Case(n_e, lambda pin: {"out": pin.map("refract", 4, *cached("refl", refl_in)[:3])})

    # --- lobes
    for i, (name, (mt, tex)) in enumerate(MATERIALS.items()):
        def lobes(i=i):
            return _lobe_inputs(1000 + i)
        n_e = cached(("lobe", i), lobes)[4]
        m = _material(mt, tex)
        # whole outputs are kept for the four lobes over a constant texture; the checker / no-lobe variants are held by their CRC alone (file size)
        st = None if i < 4 else np.arange(0)
        cases[f"material_f_{name}"] = Case(n_e, lambda pin, i=i, m=m, lobes=lobes: {"out": pin.material("f", m, *cached(("lobe", i), lobes)[:4])}, stored=st)
        cases[f"material_pdf_{name}"] = Case(n_e, lambda pin, i=i, m=m, lobes=lobes: {
            "out": pin.material("pdf", m, cached(("lobe", i), lobes)[0], cached(("lobe", i), lobes)[1], cached(("lobe", i), lobes)[3])}, stored=st)
        cases[f"material_s_f_{name}"] = Case(n_e, lambda pin, i=i, m=m, lobes=lobes: {
            "out": pin.material("s_f", m, cached(("lobe", i), lobes)[0], cached(("lobe", i), lobes)[2], cached(("lobe", i), lobes)[3])}, stored=st)
    # Beckmann / TrowbridgeReitz at both ends of the roughness range, at EffectivelySmooth's 1e-3 (below it alpha is clamped) and the materials' own
    ALPHAS = [(0.001, 0.001), (0.0005, 2e-4), (float(ulps(F32(0.001), 1)), 0.001), (0.01, 0.02), (0.01, 0.1), (0.01, 0.01), (0.3, 0.3), (1.0, 1.0), (1.0, 0.001)]
    for dist, dname in ((0, "beckmann"), (1, "trowbridge_reitz")):
        def lobes():
            return _lobe_inputs(1100)
        n_e = cached(("lobe", "mf"), lobes)[4]

        def run(pin, dist=dist, lobes=lobes):
            wo, wh, _, uu, _ = cached(("lobe", "mf"), lobes)
            step = len(ALPHAS)
            return {"out": np.concatenate([pin.microfacet(dist, ax, ay, wo[j::step], wh[j::step], uu[j::step]) for j, (ax, ay) in enumerate(ALPHAS)])}
        cases[f"microfacet_{dname}"] = Case(0, run)
    return cases


def canonical(fields, excluded=()):
    """{field: array} -> (n, W) uint32: the bits of every compared field side by side, every NaN as 0x7FC00000"""
    cols = []
    for name, a in fields.items():
        if name in excluded:
            continue
        a = np.ascontiguousarray(a)
        a = a.reshape(len(a), -1)
        if a.dtype == np.float32:
            a = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
        cols.append(np.ascontiguousarray(a).view(np.uint32) if a.dtype != np.uint32 else a)
    return np.ascontiguousarray(np.concatenate(cols, 1))
