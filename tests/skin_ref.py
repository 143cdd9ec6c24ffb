"""The definition of trc_skin_vertices (include/tracer_abi.h) restated in numpy, for tests/test_skin_cpu.py and
tests/test_gpu_skin_vertices.py.  Everything is a float32 array and every line is ONE operation, so nothing is fused and the orders are
the header's:  B.e = ((w0*M[b0].e + w1*M[b1].e) + w2*M[b2].e) + w3*M[b3].e  for every matrix entry that is read, then
x' = ((B.c0.x*x + B.c1.x*y) + B.c2.x*z) + B.c3.x  as in tests/pose_ref.py.

A palette is a sequence of (model, normal): two (4, 4) matrices in the mathematical layout, m[r, c] = row r of column c.  A binding
is (first, bones_idx, weights): vertex first + i has the influences (bones_idx[i, k], weights[i, k]), k = 0..3.  Vertices are (n, 8)
float32 rows: position, normal, uv."""
import numpy as np

import pose_ref as pr

F = np.float32
MAX_BONES = 65536


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def stack(palette):
    """-> (model, normal): two (n_bones, 4, 4) float32 arrays"""
    return _f([p[0] for p in palette]).reshape(-1, 4, 4), _f([p[1] for p in palette]).reshape(-1, 4, 4)


def blend(mats, bones_idx, weights):
    """(n_bones, 4, 4), (n, 4), (n, 4) -> (n, 3, 4): rows 0..2 of every vertex's blended matrix, summed in the order k = 0, 1, 2, 3"""
    w = _f(weights)[:, :, None, None]
    m = mats[:, :3, :]
    p0 = w[:, 0] * m[bones_idx[:, 0]]
    p1 = w[:, 1] * m[bones_idx[:, 1]]
    p2 = w[:, 2] * m[bones_idx[:, 2]]
    p3 = w[:, 3] * m[bones_idx[:, 3]]
    s = p0 + p1
    s = s + p2
    s = s + p3
    assert s.dtype == F
    return s


def transform(b, x, y, z, translate):
    """rows 0..2 of the per-vertex matrices b (n, 3, 4) applied to (x, y, z): pose_ref.transform with one matrix per vertex"""
    out = []
    for r in range(3):
        t0 = b[:, r, 0] * x
        t1 = b[:, r, 1] * y
        t2 = b[:, r, 2] * z
        s = t0 + t1
        s = s + t2
        if translate:
            s = s + b[:, r, 3]
        assert s.dtype == F
        out.append(s)
    return out


def skin(rest, current, first, bones_idx, weights, palette):
    """rest, current: (n, 8) float32; -> the vertices after trc_skin_vertices(palette) under the binding (first, bones_idx, weights):
    the bound range from REST, the others as in current"""
    rest, out = _f(rest), _f(current).copy()
    bones_idx = np.asarray(bones_idx, dtype=np.int64).reshape(-1, 4)
    count = len(bones_idx)
    model, normal = stack(palette)
    bm, bn = blend(model, bones_idx, weights), blend(normal, bones_idx, weights)
    r = rest[first:first + count]
    x, y, z = transform(bm, r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), True)
    nx, ny, nz = transform(bn, r[:, 3].copy(), r[:, 4].copy(), r[:, 5].copy(), False)
    out[first:first + count] = np.stack([x, y, z, nx, ny, nz, r[:, 6], r[:, 7]], axis=1)
    return out


def valid_binding(first, bones_idx, weights, n_vertex):
    """what trc_skin_bind accepts (TRC_OK) on a scene with n_vertex > 0 vertices; a refusal is TRC_ERR_INVALID_ARG.  An empty table
    removes the binding, whatever `first`."""
    bones_idx = np.asarray(bones_idx, dtype=np.int64).reshape(-1, 4)
    if len(bones_idx) == 0:
        return True
    if first + len(bones_idx) > n_vertex:
        return False
    return bool(np.isfinite(_f(weights)).all() and (bones_idx >= 0).all() and (bones_idx < MAX_BONES).all())


def valid_palette(palette, max_bone):
    """what trc_skin_vertices accepts for a binding whose largest bone index is max_bone; an empty palette is TRC_OK and does nothing"""
    if len(palette) == 0:
        return True
    if len(palette) > MAX_BONES or len(palette) <= max_bone:
        return False
    model, normal = stack(palette)
    return bool(np.isfinite(model[:, :3, :4]).all() and np.isfinite(normal[:, :3, :3]).all())


# ---------------------------------------------------------------------------------------------------- data for the tests
def palette(n_bones, centre):
    """n_bones (model, normal) pairs from pose_ref.turn: every bone its own angle, non-uniform scale and shift, so that no product
    of a blend or of the transform is exact"""
    out = []
    for k in range(n_bones):
        angle = -1.45 + 2.9 * ((k * 0.6180339887) % 1.0)
        scale = (0.85 + 0.3 * ((k * 0.377) % 1.0), 0.9 + 0.2 * ((k * 0.713) % 1.0), 0.8 + 0.35 * ((k * 0.129) % 1.0))
        shift = (-17.0 + 34.0 * ((k * 0.271) % 1.0), -19.0 + 31.0 * ((k * 0.557) % 1.0), -13.0 + 29.0 * ((k * 0.839) % 1.0))
        out.append(pr.turn(centre, angle, scale, shift))
    return out


def identity_palette(n_bones):
    return [(pr.identity(), pr.identity())] * n_bones


def binding(count, n_bones, seed=11):
    """(bones_idx (count, 4) int64, weights (count, 4) float32) for `count` vertices over a palette of n_bones: weights that are inexact
    in float32 and sum to about 0.97, never exactly 1.  By i % 5: 0 and 3 have four non-zero influences, 1 has two weights of 0,
    2 names its first bone twice, 4 has one weight of 0; vertex 1 (if any) has a negative weight.  Every 7th vertex names bone 0
    and every 7th the last bone, so that both ends of a large palette are read."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, n_bones, size=(count, 4), dtype=np.int64)
    w = (rng.random((count, 4)) + 0.05).astype(F)
    total = w.sum(axis=1, dtype=F)[:, None]
    w = w / total
    w = w * F(0.97)
    i = np.arange(count)
    w[i % 5 == 1, 2:] = F(0)
    w[i % 5 == 4, 3] = F(0)
    b[i % 5 == 2, 1] = b[i % 5 == 2, 0]
    b[0::7, 0] = 0
    b[3::7, 1] = n_bones - 1
    if count > 1:
        w[1, 0] = F(-0.3)
    return b, _f(w)
