"""The motion texel of trc_denoise_track_motion (include/tracer_abi.h, "Motion tracking") restated in numpy, for
tests/test_svgf_motion_ref.py and tests/test_gpu_denoise_motion.py.  Everything is a float32 array and every line is ONE operation, so
nothing is fused and the order of every sum is the header's:  dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z.

Vertices are (n, 8) float32 rows (position, normal, uv), `indices` the scene's idxList; a vector is a tuple of three arrays."""
import numpy as np

F = np.float32
MOTION = np.dtype([("prev", np.float32, 3), ("moved", np.uint32)])


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def _sub(p, q):
    return p[0] - q[0], p[1] - q[1], p[2] - q[2]


def _dot(p, q):
    t0 = p[0] * q[0]
    t1 = p[1] * q[1]
    t2 = p[2] * q[2]
    s = t0 + t1
    s = s + t2
    assert s.dtype == F
    return s


def _cross(p, q):
    a0 = p[1] * q[2]
    b0 = p[2] * q[1]
    a1 = p[2] * q[0]
    b1 = p[0] * q[2]
    a2 = p[0] * q[1]
    b2 = p[1] * q[0]
    return a0 - b0, a1 - b1, a2 - b2


def gbuffer_rays(cam, W, H):
    """(o, d) of the header's G-buffer ray for every pixel, row by row: o = lookFrom (3 scalars), d (3 arrays of W*H) normalised"""
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs.astype(F) / F(W)).ravel()
    v = (ys.astype(F) / F(H)).ravel()
    vec = lambda a: (F(a.x), F(a.y), F(a.z))
    eye, hor, ver, cll = vec(cam.lookFrom), vec(cam.horizontal), vec(cam.vertical), vec(cam.cornerLowLeft)
    s = [None] * 3
    for k in range(3):
        t = hor[k] * u
        t = cll[k] + t
        w = ver[k] * v
        t = t + w
        s[k] = t - eye[k]
    n2 = _dot(s, s)
    r = np.sqrt(n2)
    inv = F(1) / r
    d = (s[0] * inv, s[1] * inv, s[2] * inv)
    return eye, d


def texels(o, d, triangle, current, snapshot, indices):
    """The motion texels of rays (o, d): `triangle` (n,) int64 is the triangle each ray's primary hit is, or -1 for every other texel
    (a miss, an analytic primitive).  current / snapshot: the vertices now and when the last trc_denoise ran.  -> (n,) MOTION"""
    current, snapshot = _f(current), _f(snapshot)
    indices = np.asarray(indices, dtype=np.int64)
    triangle = np.asarray(triangle, dtype=np.int64)
    out = np.zeros(len(triangle), MOTION)
    sel = np.nonzero(triangle >= 0)[0]
    if len(sel) == 0:
        return out
    t = triangle[sel]
    ia, ib, ic = indices[3 * t], indices[3 * t + 1], indices[3 * t + 2]
    col = lambda arr, idx: (arr[idx, 0].copy(), arr[idx, 1].copy(), arr[idx, 2].copy())
    a, b, c = col(current, ia), col(current, ib), col(current, ic)
    a_, b_, c_ = col(snapshot, ia), col(snapshot, ib), col(snapshot, ic)
    dd = (d[0][sel], d[1][sel], d[2][sel])
    oo = (np.full(len(sel), o[0], F), np.full(len(sel), o[1], F), np.full(len(sel), o[2], F))
    e1 = _sub(b, a)
    e2 = _sub(c, a)
    pvec = _cross(dd, e2)
    det = _dot(e1, pvec)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1) / det
    tvec = _sub(oo, a)
    u = _dot(tvec, pvec)
    u = u * inv
    qvec = _cross(tvec, e1)
    v = _dot(dd, qvec)
    v = v * inv
    w = F(1) - u
    w = w - v
    prev = np.empty((len(sel), 3), F)
    for k in range(3):
        t0 = u * b_[k]
        t1 = v * c_[k]
        s = t0 + t1
        t2 = w * a_[k]
        s = s + t2
        assert s.dtype == F
        prev[:, k] = s
    moved = np.zeros(len(sel), bool)
    for now, then in ((a, a_), (b, b_), (c, c_)):
        for k in range(3):
            moved |= now[k] != then[k]
    out["prev"][sel] = prev
    out["moved"][sel] = moved
    return out
