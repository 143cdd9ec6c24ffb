"""What the fast-math build (libtracer_amd_fast.so) is held to, for tests/test_fast_ref_cpu.py and the tests/test_gpu_fast_*.py modules.

1. Float64 restatements of include/tracer_abi.h's definitions (pose, skin, morph, fused morph + skin, recomputed normals) on the same
   binary32 inputs.  Every value travels with a first-order running error bound (class T below):
     - every product and sum of the definition adds u = 2^-24 times the absolute value of its float64 result, and the bounds of its
       operands are propagated through absolute values;
     - contraction (an fma in place of a product and a sum) only removes a rounding, so it needs no term of its own;
     - a division or square root adds DIV_SQRT_ULP units in the last place.  The compiler documentation shipped with the toolchain
       names no figure for -fno-hip-fp32-correctly-rounded-divide-sqrt (its option help only says that, without the flag, divide and
       sqrt need not be correctly rounded), so the issue's fallback of 4 ulp is used;
     - every operation adds 2^-126 absolute for a flushed denormal;
     - the total is doubled for the second-order terms (bound()).
   No other tolerance constant belongs in the geometry tests.
2. validate_tree: what makes trc_download_bvh's records a tree over a given leaf list.
3. robust_rays: the camera rays whose first hit does not depend on the last bits of the arithmetic, by the CPU oracle."""
import numpy as np

import normals_ref as nr
import skin_ref as sr
from tracer_amd import abi
from tracer_amd.dtypes import make_rays

F = np.float32
D = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
DIV_SQRT_ULP = 4.0
PARENT, LEFT, RIGHT, AXIS, PTYPE, PINDEX = range(6)
MINI, MAXI = slice(8, 11), slice(12, 15)
PRIM_BVH = np.uint32(abi.PRIM_BVH & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------- values with a running bound
class T:
    """v: the float64 value of an expression of the definition; e: first-order bound on |binary32 evaluation - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=D)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=D), self.v.shape).copy()

    def __getitem__(self, k):
        return T(self.v[k], self.e[k])

    def __neg__(self):
        return T(-self.v, self.e)


def given(x):
    """a binary32 input: exact"""
    a = np.asarray(x)
    assert a.dtype == F, a.dtype
    return T(a.astype(D))


def mul(a, b):
    v = a.v * b.v
    return T(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + U * np.abs(v) + TINY)


def add(a, b):
    v = a.v + b.v
    return T(v, a.e + b.e + U * np.abs(v) + TINY)


def sub(a, b):
    return add(a, -b)


def div(a, b):
    with np.errstate(all="ignore"):
        v = a.v / b.v
        return T(v, a.e / np.abs(b.v) + np.abs(v) * b.e / np.abs(b.v) + DIV_SQRT_ULP * 2.0 * U * np.abs(v) + TINY)


def sqrt(a):
    with np.errstate(all="ignore"):
        v = np.sqrt(a.v)
        return T(v, a.e / (2.0 * v) + DIV_SQRT_ULP * 2.0 * U * np.abs(v) + TINY)


def where(m, a, b):
    return T(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def stack(ts, axis):
    return T(np.stack([t.v for t in ts], axis), np.stack([t.e for t in ts], axis))


def bound(t):
    """the tolerance of a comparison: the first-order total, doubled"""
    return 2.0 * t.e


def within(got, t):
    """component by component: |got - value| <= bound; -> boolean array"""
    return np.abs(np.asarray(got, dtype=D) - t.v) <= bound(t)


def free_of_denormals(*arrays):
    """no binary32 input is a denormal (zeros are fine)"""
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=F))
        if ((a > 0) & (a < F(2.0 ** -126))).any():
            return False
    return True


# ---------------------------------------------------------------------------------------------------- pose, skin, morph
def _transform(m, x, y, z, translate):
    """rows 0..2 of m (T of shape (..., 3, 4), broadcast against x) applied to (x, y, z): the header's ((m0 x + m1 y) + m2 z) [+ m3]"""
    out = []
    for r in range(3):
        s = add(mul(m[..., r, 0], x), mul(m[..., r, 1], y))
        s = add(s, mul(m[..., r, 2], z))
        if translate:
            s = add(s, m[..., r, 3])
        out.append(s)
    return out


def _rows(values6, model, normal):
    """T (count, 6) -> T (count, 6): positions under `model`, normals under `normal` (T of (3, 4) or (count, 3, 4))"""
    p = _transform(model, values6[:, 0], values6[:, 1], values6[:, 2], True)
    n = _transform(normal, values6[:, 3], values6[:, 4], values6[:, 5], False)
    return stack(p + n, 1)


def _result(current):
    cur = np.ascontiguousarray(current, dtype=F)
    return T(cur.astype(D))


def _put(out, first, count, t6, uv):
    out.v[first:first + count, :6] = t6.v; out.e[first:first + count, :6] = t6.e
    out.v[first:first + count, 6:] = uv; out.e[first:first + count, 6:] = 0.0


def pose(rest, current, poses):
    """pose_ref.pose in float64 -> T of (n, 8): every range from REST (uv copied, bound 0), the others as in current (bound 0)"""
    rest = np.ascontiguousarray(rest, dtype=F)
    out = _result(current)
    for first, count, model, normal in poses:
        r = rest[first:first + count]
        m, nm = given(np.ascontiguousarray(model, dtype=F)[:3, :4]), given(np.ascontiguousarray(normal, dtype=F)[:3, :4])
        _put(out, first, count, _rows(given(r[:, :6]), m, nm), r[:, 6:])
    return out


def blend(mats, bones_idx, weights, order=(0, 1, 2, 3)):
    """skin_ref.blend in float64 -> T of (n, 3, 4); `order`: the influences summed (the definition's is 0, 1, 2, 3)"""
    w = given(np.ascontiguousarray(weights, dtype=F))
    m = np.ascontiguousarray(mats, dtype=F)[:, :3, :]
    term = lambda k: mul(T(w.v[:, k, None, None]), given(m[bones_idx[:, k]]))
    s = term(order[0])
    for k in order[1:]:
        s = add(s, term(k))
    return s


def _skin_rows(values6, bones_idx, weights, palette, order=(0, 1, 2, 3)):
    model, normal = sr.stack(palette)
    return _rows(values6, blend(model, bones_idx, weights, order), blend(normal, bones_idx, weights, order))


def skin(rest, current, first, bones_idx, weights, palette, order=(0, 1, 2, 3)):
    """skin_ref.skin in float64 -> T of (n, 8)"""
    rest = np.ascontiguousarray(rest, dtype=F)
    bones_idx = np.asarray(bones_idx, dtype=np.int64).reshape(-1, 4)
    count = len(bones_idx)
    out = _result(current)
    r = rest[first:first + count]
    _put(out, first, count, _skin_rows(given(r[:, :6]), bones_idx, weights, palette, order), r[:, 6:])
    return out


def morphed_values(rest, first, deltas, weights, skip=()):
    """morph_ref.morphed_values in float64 -> T of (n, 8): `rest` with rows [first, first + count) morphed; `skip`: targets left out"""
    import morph_ref as mr
    rest = np.ascontiguousarray(rest, dtype=F)
    deltas = np.ascontiguousarray(deltas, dtype=F)
    count = deltas.shape[1]
    out = _result(rest)
    acc = given(rest[first:first + count, :6])
    for k, w in mr.active(weights):
        if k in skip:
            continue
        acc = add(acc, mul(given(np.full((1, 1), w, F)), given(deltas[k])))
    _put(out, first, count, acc, rest[first:first + count, 6:])
    return out


def morph(rest, current, first, deltas, weights, skip=()):
    """morph_ref.morph in float64 -> T of (n, 8)"""
    count = np.asarray(deltas).shape[1]
    staged = morphed_values(rest, first, deltas, weights, skip)
    out = _result(current)
    out.v[first:first + count] = staged.v[first:first + count]; out.e[first:first + count] = staged.e[first:first + count]
    return out


def morph_skin(rest, current, first, deltas, weights, skin_first, bones_idx, skin_weights, palette):
    """morph_ref.morph_skin in float64 -> T of (n, 8): the skin's operands are the morphed values, bounds and all"""
    staged = morphed_values(rest, first, deltas, weights)
    out = morph(rest, current, first, deltas, weights)
    bones_idx = np.asarray(bones_idx, dtype=np.int64).reshape(-1, 4)
    count = len(bones_idx)
    s = staged[skin_first:skin_first + count]
    _put(out, skin_first, count, _skin_rows(s[:, :6], bones_idx, skin_weights, palette), s.v[:, 6:])
    return out


# ---------------------------------------------------------------------------------------------------- recomputed normals
def normals(vertices, indices, first=0, count=None, normalise=True):
    """normals_ref.recompute in float64 -> (T of (n, 3): the new normals, T of (n,): their length, decided (n,) bool).
    `decided`: the vertices of the range whose branch the bounds settle -- the sign of the side rule's dot product and a length that
    is above its own bound; the others (and the vertices normals_ref.kept names) are judged by neither the values nor the bound.
    normalise=False leaves the sums undivided (the wrong variant of tests/test_fast_ref_cpu.py)."""
    v = np.ascontiguousarray(vertices, dtype=F)
    n = len(v)
    count = n - first if count is None else count
    tri = np.asarray(indices, dtype=np.uint32).reshape(-1, 3)
    p = given(v[:, :3])
    e1, e2 = sub(p[tri[:, 1]], p[tri[:, 0]]), sub(p[tri[:, 2]], p[tri[:, 0]])
    cr = lambda a, b: sub(mul(e1[:, a], e2[:, b]), mul(e1[:, b], e2[:, a]))
    c = stack([cr(1, 2), cr(2, 0), cr(0, 1)], 1)
    offsets, corners = nr.adjacency(indices, n)
    val = (offsets[1:] - offsets[:-1]).astype(np.int64)
    s = T(np.zeros((n, 3)))
    for j in range(int(val.max()) if n else 0):
        m = np.nonzero(val > j)[0]
        t = add(s[m], c[corners[offsets[m] + j] // 3])
        s.v[m] = t.v; s.e[m] = t.e
    nc = given(v[:, 3:6])
    d = add(add(mul(s[:, 0], nc[:, 0]), mul(s[:, 1], nc[:, 1])), mul(s[:, 2], nc[:, 2]))
    s = where((d.v < 0)[:, None], -s, s)
    q = add(add(mul(s[:, 0], s[:, 0]), mul(s[:, 1], s[:, 1])), mul(s[:, 2], s[:, 2]))
    l = sqrt(q)
    with np.errstate(all="ignore"):
        new = div(s, T(l.v[:, None], l.e[:, None])) if normalise else s
        length = sqrt(add(add(mul(new[:, 0], new[:, 0]), mul(new[:, 1], new[:, 1])), mul(new[:, 2], new[:, 2])))
        decided = nr.in_range(n, first, count) & (np.abs(d.v) > bound(d)) & (q.v > bound(q)) & np.isfinite(l.v)
    return new, length, decided


# ---------------------------------------------------------------------------------------------------- trees
def raw(nodes):
    """(n, 16) uint32 copy of a ctypes array of abi.BVH (or of an array that already is one)"""
    if isinstance(nodes, np.ndarray):
        return nodes.astype(np.uint32, copy=True).reshape(-1, 16)
    return np.frombuffer(bytes(memoryview(nodes)), dtype=np.uint32).reshape(-1, 16).copy()


def leaves_of(records):
    """sorted [(pType, pIndex)] of the leaf records"""
    a = raw(records)
    leaf = a[a[:, PTYPE] != PRIM_BVH]
    return sorted((int(t), int(i)) for t, i in leaf[:, [PTYPE, PINDEX]])


def validate_tree(records, expected_leaves, max_depth=abi.TRC_MAX_BVH_DEPTH):
    """'' when `records` (trc_download_bvh, root at 0) is a binary tree over exactly `expected_leaves` [(pType, pIndex)], else what is
    wrong: 2n - 1 records and one root; every expected leaf exactly once; parent, left and right agree; every interior box equals, as
    values, the component-wise min / max of its children's; depth <= max_depth.  -> (message, depth of the deepest leaf)"""
    a = raw(records)
    box = a.view(F)
    n = len(expected_leaves)
    if len(a) != 2 * n - 1:
        return f"{len(a)} records for {n} leaves, not {2 * n - 1}", -1
    interior = a[:, PTYPE] == PRIM_BVH
    if n > 1 and not interior[0]:
        return "record 0 is not an interior record", -1
    if a[0, PARENT] != 0:
        return f"the root names parent {a[0, PARENT]}", -1
    got = sorted((int(t), int(i)) for t, i in a[~interior][:, [PTYPE, PINDEX]])
    want = sorted((int(t), int(i)) for t, i in expected_leaves)
    if got != want:
        twice = sorted({g for k, g in enumerate(got[1:]) if g == got[k]})
        missing = sorted(set(want) - set(got)); extra = sorted(set(got) - set(want))
        return f"leaves: twice {twice[:3]}, missing {missing[:3]}, unexpected {extra[:3]}", -1
    seen = np.zeros(len(a), bool)
    depth = np.zeros(len(a), np.int64)
    seen[0] = True
    order = [0]
    for i in order:
        if not interior[i]:
            continue
        l, r = int(a[i, LEFT]), int(a[i, RIGHT])
        for c in (l, r):
            if c >= len(a) or c == 0:
                return f"record {i} names child {c}: dangling", -1
            if seen[c]:
                return f"record {c} is the child of two records (second: {i})", -1
            if a[c, PARENT] != i:
                return f"record {c} names parent {a[c, PARENT]}, its parent is {i}", -1
            seen[c] = True; depth[c] = depth[i] + 1
            order.append(c)
        if l == r:
            return f"record {i} names child {l} twice", -1
    if not seen.all():
        return f"{(~seen).sum()} records are not reached from the root, first {np.nonzero(~seen)[0][0]}", -1
    for i in reversed(order):
        if interior[i]:
            l, r = int(a[i, LEFT]), int(a[i, RIGHT])
            lo, hi = np.minimum(box[l, MINI], box[r, MINI]), np.maximum(box[l, MAXI], box[r, MAXI])
            if not (np.array_equal(box[i, MINI], lo) and np.array_equal(box[i, MAXI], hi)):
                return f"box of record {i} is [{box[i, MINI]}, {box[i, MAXI]}], its children's union is [{lo}, {hi}]", -1
    deepest = int(depth[~interior].max()) if n > 1 else 0
    if deepest > max_depth:
        return f"depth {deepest} > {max_depth}", deepest
    return "", deepest


def leaf_boxes(records):
    """{(pType, pIndex): 6 uint32 box words} of the leaf records"""
    a = raw(records)
    return {(int(r[PTYPE]), int(r[PINDEX])): tuple(int(x) for x in np.concatenate([r[MINI], r[MAXI]])) for r in a[a[:, PTYPE] != PRIM_BVH]}


# ---------------------------------------------------------------------------------------------------- robust rays
TILT = 1e-4            # radians
MAX_NON_ROBUST = 0.10


def _tilted(d, axis, angle):
    """(n, 3) float64 directions turned by `angle` about coordinate axis `axis`"""
    c, s = np.cos(angle), np.sin(angle)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    out = d.copy()
    out[:, i] = c * d[:, i] - s * d[:, j]
    out[:, j] = s * d[:, i] + c * d[:, j]
    return out


def robust_rays(view, rays):
    """boolean (n,): the CPU oracle reports the same (hit, pType, pIndex) for the ray and for four copies whose direction is tilted by
    +-TILT about the x and the y axis (a camera ray here looks along z, so both tilts move it across the picture)"""
    from oracle import pyoracle
    base = pyoracle.trace_rays(view, rays)
    o = np.ascontiguousarray(rays["origin"], dtype=F)
    d = np.asarray(rays["direction"], dtype=D)
    ok = np.ones(len(rays), bool)
    for axis in (0, 1):
        for angle in (TILT, -TILT):
            got = pyoracle.trace_rays(view, make_rays(o, _tilted(d, axis, angle).astype(F)))
            ok &= (got["hit"] == base["hit"]) & (got["pType"] == base["pType"]) & (got["pIndex"] == base["pIndex"])
    return ok


# ---------------------------------------------------------------------------------------------------- analytic primitives
def primitive_leaf_box(mini, maxi, cols):
    """primitives_ref.leaf_box in float64 -> (lo, hi): T of (3,) each.  A min / max of eight values moves by no more than the
    largest move of one of them, so the corner bounds' maximum is the box's."""
    ele = (np.asarray(mini, dtype=F), np.asarray(maxi, dtype=F))
    c = given(np.asarray(cols, dtype=F))                               # [column][row]
    one = given(np.asarray(1.0, dtype=F))
    ws = []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                x, y, z = given(ele[i][0]), given(ele[j][1]), given(ele[k][2])
                row = []
                for q in range(3):
                    s = add(mul(c[0, q], x), mul(c[1, q], y))
                    s = add(s, mul(c[2, q], z))
                    row.append(add(s, mul(c[3, q], one)))
                ws.append(stack(row, 0))
    w = stack(ws, 0)                                                    # (8, 3)
    e = w.e.max(axis=0)
    return T(w.v.min(axis=0), e), T(w.v.max(axis=0), e)


def square_pdf(range_i, range_j):
    """primitives_ref.pack_square's 1 / (2 di dj) in float64 -> T scalar"""
    i, j = given(np.asarray(range_i, dtype=F)), given(np.asarray(range_j, dtype=F))
    di, dj = sub(i[1], i[0]), sub(j[1], j[0])
    area = mul(mul(given(np.asarray(2.0, dtype=F)), di), dj)
    return div(given(np.asarray(1.0, dtype=F)), area)


# ---------------------------------------------------------------------------------------------------- the per-tile error estimate
EPS = np.asarray(1e-4, dtype=F)       # TRC_ADAPTIVE_EPS
CAP = 65535.0


def pixel_scaled(I, A):
    """adaptive_ref.pixel_q before the truncation, in float64: T of the pixels' e * 65536.  max(s, eps) and min(e, cap) move by no more
    than their operand; a pixel that takes the eps or the cap because of a NaN, an infinity or a sign takes it exactly (bound 0).  Planes
    whose finite sums overflow binary32 are outside this restatement."""
    I, A = np.asarray(I, dtype=F), np.asarray(A, dtype=F)
    i, a = given(np.ascontiguousarray(I[..., :3])), given(np.ascontiguousarray(A[..., :3]))
    with np.errstate(all="ignore"):
        ab = lambda t: T(np.abs(t.v), t.e)
        d = add(add(ab(sub(i[..., 0], a[..., 0])), ab(sub(i[..., 1], a[..., 1]))), ab(sub(i[..., 2], a[..., 2])))
        s = add(add(i[..., 0], i[..., 1]), i[..., 2])
        eps = T(np.full(s.v.shape, float(EPS)))
        s1 = where(s.v > float(EPS), s, eps)                            # a NaN s takes the eps
        e = div(d, sqrt(s1))
        cap = T(np.full(s.v.shape, CAP))
        e1 = where(e.v < CAP, e, cap)                                   # NaN and inf take the cap
        e1 = T(e1.v, np.where(np.isfinite(e1.e), e1.e, 0.0))
        return mul(e1, given(np.asarray(65536.0, dtype=F)))


def tile_errors(I, A):
    """adaptive_ref.tile_errors (every tile) in float64 -> T of (n tiles,): E_t's bound is the sum over the tile of the pixels' bounds
    plus 1 for each truncation, divided by N_t * 65536, plus the rounding of E_t itself."""
    import adaptive_ref as ar
    H, W = np.asarray(I).shape[:2]
    sc = pixel_scaled(I, A)
    th, tw = ar.tile_grid(W, H)
    v, e = np.zeros(th * tw), np.zeros(th * tw)
    for t, rows, cols in ar.tile_slices(W, H):
        n = sc.v[rows, cols].size
        v[t] = np.floor(sc.v[rows, cols]).sum() / (n * 65536.0)
        e[t] = (bound(sc)[rows, cols] + 1.0).sum() / (n * 65536.0) / 2.0 + U * v[t]      # (bound() doubles e again)
    return T(v, e)


# ---------------------------------------------------------------------------------------------------- frames: two renders of one picture
RMSE_FACTOR, BLOCK_FACTOR, MEAN_REL, RAYS_REL = 1.15, 1.2, 0.01, 0.01      # tests/test_gpu_fast_math.py's thresholds
LUM_CLIP = 4.0                                                              # fireflies of single pixels would dominate an RMSE


def luminance(frame):
    f = np.asarray(frame, dtype=D)
    return f[..., 0] * 0.2126 + f[..., 1] * 0.7152 + f[..., 2] * 0.0722


def frame_figures(candidate, exact_a, exact_b):
    """luminance frames -> dict: the candidate's distance from exact_a in units of the seed noise (exact_a against exact_b, another seed
    of the same build), per pixel (clipped-luminance RMSE) and per 8 x 8 block mean, and the relative difference of the clipped means"""
    H, W = exact_a.shape
    clip = lambda x: np.minimum(x, LUM_CLIP)
    blk = lambda x: clip(x)[: H // 8 * 8, : W // 8 * 8].reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))
    rms = lambda x: float(np.sqrt(np.mean(x ** 2)))
    noise, block_noise = rms(clip(exact_a) - clip(exact_b)), rms(blk(exact_a) - blk(exact_b))
    return dict(rmse=rms(clip(candidate) - clip(exact_a)) / noise, blocks=rms(blk(candidate) - blk(exact_a)) / block_noise,
                mean=abs(clip(candidate).mean() - clip(exact_a).mean()) / clip(exact_a).mean(), noise=noise, block_noise=block_noise,
                finite=bool(np.isfinite(candidate).all()))


def frames_disagree(fig, rays=None, margin=1.0):
    """[] when the figures say "indistinguishable from a re-seeded exact render", else the criteria missed.  margin 0.5: every threshold
    with half its margin (1.075, 1.10, 0.5 %), what further exact seeds must meet for a frame size to be usable.  rays: (candidate's
    ray count, exact_a's)."""
    out = []
    if not fig["finite"]:
        out.append("not finite")
    if not fig["rmse"] < 1.0 + (RMSE_FACTOR - 1.0) * margin:
        out.append(f"rmse {fig['rmse']:.4f} x seed noise")
    if not fig["blocks"] < 1.0 + (BLOCK_FACTOR - 1.0) * margin:
        out.append(f"8x8 block means {fig['blocks']:.4f} x seed noise")
    if not fig["mean"] < MEAN_REL * margin:
        out.append(f"mean off by {fig['mean']:.5f}")
    if rays is not None and not abs(rays[0] - rays[1]) < RAYS_REL * rays[1]:
        out.append(f"rays {rays[0]} against {rays[1]}")
    return out
