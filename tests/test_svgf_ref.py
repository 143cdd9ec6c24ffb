"""The CPU restatement of the SVGF stage (tests/svgf_ref/svgf_ref.cpp, include/tracer_abi.h "SVGF denoiser") on synthetic
G-buffers: the properties the statement promises, and agreement with an independent float64 numpy version of the same
statement (which catches a formula the kernel and the restatement could both get wrong)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_ref"))
import svgf_loader as sl  # noqa: E402

from tracer_amd import host  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sl.build(tmp_path_factory.mktemp("svgf_ref"))


def rotated(cam, degrees):
    """cam turned about its vertical axis through lookFrom (the camera vectors rotated; lens and film unchanged)"""
    import copy
    a = np.radians(degrees)
    v = np.array([cam.v.x, cam.v.y, cam.v.z], np.float64)
    v /= np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    out = copy.deepcopy(cam)
    eye = np.array([cam.lookFrom.x, cam.lookFrom.y, cam.lookFrom.z], np.float64)
    for name, is_point in (("lookAt", True), ("u", False), ("v", False), ("w", False), ("vertical", False), ("horizontal", False),
                           ("cornerLowLeft", True)):
        f = getattr(cam, name)
        x = np.array([f.x, f.y, f.z], np.float64)
        y = R @ (x - eye) + eye if is_point else R @ x
        g = getattr(out, name)
        g.x, g.y, g.z = (float(np.float32(t)) for t in y)
    return out


def plane_gbuffer(cam, W, H, tilt=0.3, dist=600.0, step=None):
    """G-buffer of a tilted plane in front of the Cornell camera (a fixed plane in the world, whatever the camera);
    step = (x0, dist2): pixels x >= x0 (of the unrotated view) see a second plane at dist2 instead; material 0 / 1"""
    base = host.prepare_camera(W, H)
    f = lambda a: np.array([a.x, a.y, a.z], np.float64)
    nrm = f(base.w) + tilt * f(base.u)
    nrm /= np.linalg.norm(nrm)
    P0 = f(base.lookFrom) - dist * f(base.w)
    ys, xs = np.mgrid[0:H, 0:W]
    u, v = xs / W, ys / H
    eye = f(cam.lookFrom)
    d = f(cam.cornerLowLeft)[None, None] + f(cam.horizontal)[None, None] * u[..., None] + f(cam.vertical)[None, None] * v[..., None] - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = ((P0 - eye) @ nrm) / (d @ nrm)
    g = np.zeros((H, W), sl.GBUF)
    g["depth"] = t
    g["normal"] = nrm
    g["albedo"] = 0.5 + 0.25 * np.sin(xs * 0.3)[..., None] * np.array([1.0, 0.5, 0.25])
    g["id"] = 0
    if step is not None:
        far = xs >= step[0]
        g["depth"][far] = np.float32(step[1])
        g["id"][far] = 1
    return g


def noisy(H, W, seed, base=0.4):
    rng = np.random.default_rng(seed)
    a = np.empty((H, W, 4), np.float32)
    a[..., :3] = base * (0.5 + rng.random((H, W, 3)))
    a[..., 3] = 1.0
    return a


def ulp_diff(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


def test_constant_image_comes_back_within_2_ulp(ref):
    W, H = 48, 32
    cam = host.prepare_camera(W, H)
    g = plane_gbuffer(cam, W, H)
    g["albedo"] = 0.5                 # demodulation keeps the image constant
    for value in (0.3, 0.5, 1.7):
        for demod in (False, True):
            ref.reset()
            a = np.full((H, W, 4), value, np.float32)
            a[..., 3] = 1.0
            for _ in range(3):
                integ, hc, hm, out = ref.frame(sl.params(demodulate=demod), sl.cam_vectors(cam), g, a)
            assert ulp_diff(out[..., :3], a[..., :3]).max() <= 2, (value, demod)
            assert np.array_equal(out[..., 3], a[..., 3])


def test_unchanged_camera_is_the_exact_identity(ref):
    """A still camera takes the one tap at the same pixel with weight 1: colour = prev (1 - a) + c a with prev the history
    texel itself, bit for bit, and the history length counts frames exactly"""
    W, H = 40, 24
    cam = host.prepare_camera(W, H)
    g = plane_gbuffer(cam, W, H)
    ref.reset()
    p = sl.params(iterations=1)
    frames = [noisy(H, W, s) for s in range(6)]
    _, hc, hm, _ = ref.frame(p, sl.cam_vectors(cam), g, frames[0])
    for k, a in enumerate(frames[1:], start=2):
        prev_c, prev_m = hc.copy(), hm.copy()
        integ, hc, hm, _ = ref.frame(p, sl.cam_vectors(cam), g, a)
        assert np.all(hm[..., 2] == np.float32(k))
        n = np.float32(k)
        alpha = max(np.float32(1) / n, np.float32(0.1))
        expect = prev_c[..., :3] + (a[..., :3] - prev_c[..., :3]) * alpha
        assert np.array_equal(integ[..., :3].view(np.uint32), expect.astype(np.float32).view(np.uint32))
        am = max(np.float32(1) / n, np.float32(0.2))
        L = (np.float32(0.2126) * a[..., 0] + np.float32(0.7152) * a[..., 1]) + np.float32(0.0722) * a[..., 2]
        assert np.array_equal(hm[..., 0], prev_m[..., 0] + (L - prev_m[..., 0]) * am)


def test_no_weight_crosses_a_depth_step_or_a_miss_boundary(ref):
    W, H = 64, 32
    cam = host.prepare_camera(W, H)
    g = plane_gbuffer(cam, W, H, tilt=0.0, step=(40, 2000.0))
    g["depth"][:, 20:40] = np.float32(1000.0)         # a third, flat region: two steps
    g["albedo"] = 0.5
    miss = np.zeros((H, W), bool)
    miss[8:16, 10:30] = True
    g["depth"][miss] = np.inf
    g["normal"][miss] = 0
    g["albedo"][miss] = 1
    g["id"][miss] = sl.MISS
    a = np.zeros((H, W, 4), np.float32)
    a[..., 3] = 1
    a[:, :20, :3] = 0.25
    a[:, 20:40, :3] = 2.0
    a[:, 40:, :3] = 8.0
    a[miss, :3] = 1000.0
    for demod in (False, True):
        ref.reset()
        for _ in range(2):
            _, _, _, out = ref.frame(sl.params(demodulate=demod), sl.cam_vectors(cam), g, a)
        assert np.array_equal(out[miss], a[miss])                  # misses pass through
        for sl_x in (slice(0, 20), slice(20, 40), slice(40, W)):
            region = ~miss[:, sl_x]
            assert ulp_diff(out[:, sl_x][region][:, :3], a[:, sl_x][region][:, :3]).max() <= 2


def test_normal_weight_is_seven_squarings_bitwise(ref):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.random(20000).astype(np.float32), np.float32([0.0, 1.0, 0.9, 0.999, -0.5])])
    expect = np.maximum(x, np.float32(0))
    for _ in range(7):
        expect = expect * expect
    got = np.array([ref.L.svgf_ref_normal_weight(float(v), 128) for v in x], np.float32)
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32))
    # ... and that is x**128 up to the rounding of seven squarings
    pos = x > 0.5
    np.testing.assert_allclose(got[pos], (x[pos].astype(np.float64)) ** 128, rtol=128 * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------------------
# the same statement in float64 numpy, written independently of svgf_ref.cpp
def _shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx] where that is inside, `fill` elsewhere; and the inside mask"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
        inside[ys:ye, xs:xe] = True
    return out, inside


def _lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def np_svgf(p, cam, prev_cam, g, gp, accum, hist_col, hist_mom):
    H, W = g.shape
    demod = bool(p.flags & 1)
    z = g["depth"].astype(np.float64)
    n = g["normal"].astype(np.float64)
    alb = np.maximum(g["albedo"].astype(np.float64), 1e-3)
    hit = g["id"] != sl.MISS
    c = accum[..., :3].astype(np.float64)
    if demod:
        c = c / alb
    L = _lum(c)
    e = int(np.log2(p.normal_exponent))
    zs = np.where(hit, z, np.inf)

    def grad():
        gs = []
        for (ax, ay), (bx, by) in (((1, 0), (-1, 0)), ((0, 1), (0, -1))):
            za, ia = _shift(zs, ax, ay, np.inf)
            zb, ib = _shift(zs, bx, by, np.inf)
            da = np.where(ia & np.isfinite(za), np.abs(za - z), np.inf)
            db = np.where(ib & np.isfinite(zb), np.abs(zb - z), np.inf)
            m = np.minimum(da, db)
            gs.append(np.where(np.isfinite(m), m, 0.0))
        return gs

    gx, gy = grad()
    # temporal
    sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sm = np.zeros((H, W, 3))
    if prev_cam is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        if np.array_equal(cam, prev_cam):
            taps = [(xs, ys, np.ones((H, W)))]
            zq = z
            ok = np.ones((H, W), bool)
        else:
            c64 = cam.astype(np.float64); p64 = prev_cam.astype(np.float64)
            eye, hor, ver, cll = c64[0:3], c64[3:6], c64[6:9], c64[9:12]
            d = cll + hor * (xs / W)[..., None] + ver * (ys / H)[..., None] - eye
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            P = eye + d * np.where(hit, z, 0)[..., None]
            pe, ph, pv, pc = p64[0:3], p64[3:6], p64[6:9], p64[9:12]
            q = P - pe
            a = pc - pe
            m = np.cross(ph, pv)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = (a @ m) / (q @ m)
            px = ((q @ ph) * s - a @ ph) / (ph @ ph) * W
            py = ((q @ pv) * s - a @ pv) / (pv @ pv) * H
            zq = np.linalg.norm(q, axis=-1)
            ok = (s > 0) & np.isfinite(s) & (px > -1) & (px < W) & (py > -1) & (py < H)
            x0, y0 = np.floor(np.where(ok, px, 0)), np.floor(np.where(ok, py, 0))
            fx, fy = np.where(ok, px, 0) - x0, np.where(ok, py, 0) - y0
            taps = [(x0.astype(int) + dx, y0.astype(int) + dy, (fx if dx else 1 - fx) * (fy if dy else 1 - fy))
                    for dy in (0, 1) for dx in (0, 1)]
        for tx, ty, tw in taps:
            inb = ok & hit & (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
            cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            o = gp[cy, cx]
            cons = inb & (o["id"] == g["id"]) & (np.abs(o["depth"].astype(np.float64) - zq) <= 0.1 * zq)
            cons &= np.einsum("ijk,ijk->ij", n, o["normal"].astype(np.float64)) >= 0.9
            w = np.where(cons, tw, 0.0)
            sw += w
            sc += w[..., None] * hist_col[cy, cx, :3]
            sm += w[..., None] * hist_mom[cy, cx, :3]
    valid = sw >= 0.01
    swv = np.where(valid, sw, 1.0)
    hl = np.where(valid, np.minimum(sm[..., 2] / swv + 1, 64), 1.0)
    ac = np.where(valid, np.maximum(1 / hl, p.alpha_color), 1.0)
    am = np.where(valid, np.maximum(1 / hl, p.alpha_moments), 1.0)
    col = (sc / swv[..., None]) * (1 - ac[..., None]) + c * ac[..., None]
    mu1 = (sm[..., 0] / swv) * (1 - am) + L * am
    mu2 = (sm[..., 1] / swv) * (1 - am) + L * L * am
    var = np.maximum(mu2 - mu1 * mu1, 0)
    # 7x7 estimate
    ws = np.zeros((H, W)); s1 = np.zeros((H, W)); s2 = np.zeros((H, W))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            zq_, inb = _shift(zs, dx, dy, np.inf)
            nq, _ = _shift(n, dx, dy, 0.0)
            Lq, _ = _shift(L, dx, dy, 0.0)
            use = inb & np.isfinite(zq_) & hit
            D = p.sigma_z * (gx * abs(dx) + gy * abs(dy)) + 1e-3 * z
            with np.errstate(invalid="ignore", over="ignore"):
                w = np.exp(-np.abs(z - zq_) / D) * np.maximum(np.einsum("ijk,ijk->ij", n, nq), 0) ** (2 ** e)
            w = np.where(use, w, 0.0)
            ws += w; s1 += w * Lq; s2 += w * Lq * Lq
    wsv = np.where(ws > 0, ws, 1.0)
    var_sp = np.where(ws > 0, np.maximum(s2 / wsv - (s1 / wsv) ** 2, 0), 0)
    var = np.where(hl >= p.min_history, var, var_sp)
    col = np.where(hit[..., None], col, accum[..., :3])
    var = np.where(hit, var, 0.0)
    cur = np.concatenate([col, var[..., None]], axis=-1)
    integ = cur.copy()
    hk = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    gk = [0.25, 0.5, 0.25]
    hist_out = cur.copy()
    for it in range(p.iterations):
        step = 1 << it
        sg = np.zeros((H, W)); sv = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                zq_, inb = _shift(zs, dx, dy, np.inf)
                vq, _ = _shift(cur[..., 3], dx, dy, 0.0)
                w = np.where(inb & np.isfinite(zq_), gk[dy + 1] * gk[dx + 1], 0.0)
                sg += w; sv += w * vq
        phi = p.sigma_l * np.sqrt(np.maximum(sv / np.where(sg > 0, sg, 1), 0)) + 1e-10
        Lc = _lum(cur)
        ws = np.zeros((H, W)); C = np.zeros((H, W, 3)); V = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                zq_, inb = _shift(zs, dx * step, dy * step, np.inf)
                nq, _ = _shift(n, dx * step, dy * step, 0.0)
                cq, _ = _shift(cur, dx * step, dy * step, 0.0)
                D = p.sigma_z * (gx * abs(dx * step) + gy * abs(dy * step)) + 1e-3 * z
                with np.errstate(invalid="ignore", over="ignore"):
                    w = (hk[dx + 2] * hk[dy + 2] * np.maximum(np.einsum("ijk,ijk->ij", n, nq), 0) ** (2 ** e) *
                         np.exp(-(np.abs(z - zq_) / D + np.abs(Lc - _lum(cq)) / phi)))
                w = np.where(inb & np.isfinite(zq_) & hit, w, 0.0)
                ws += w; C += w[..., None] * cq[..., :3]; V += w * w * cq[..., 3]
        wsv = np.where(ws > 0, ws, 1.0)
        nxt = np.concatenate([C / wsv[..., None], (V / (wsv * wsv))[..., None]], axis=-1)
        cur = np.where((hit & (ws > 0))[..., None], nxt, cur)
        if it == 0:
            hist_out = cur.copy()
    out = accum.astype(np.float64).copy()
    rgb = cur[..., :3] * (alb if demod else 1.0)
    out[..., :3] = np.where(hit[..., None], rgb, accum[..., :3])
    return integ, hist_out, np.stack([mu1, mu2, hl], -1), out


@pytest.mark.parametrize("demod", [False, True])
def test_restatement_agrees_with_float64_numpy(ref, demod):
    W, H = 64, 40
    base = host.prepare_camera(W, H)
    views = [0.0, 0.0, 0.5, 1.0, 1.5, 1.5, 1.5, 4.0]          # still, stepping 0.5 degrees, still again, a jump
    p = sl.params(demodulate=demod, iterations=5)
    ref.reset()
    prev = None
    for k, deg in enumerate(views):
        cam = rotated(base, deg)
        g = plane_gbuffer(cam, W, H)
        a = noisy(H, W, 100 + k)
        cv = sl.cam_vectors(cam)
        hist = (ref.hist_col, ref.hist_mom, ref.prev_cam, ref.prev_g)
        integ, hc, hm, out = ref.frame(p, cv, g, a)
        if prev is None:
            e_integ, e_hc, e_hm, e_out = np_svgf(p, cv, None, g, None, a, None, None)
        else:
            e_integ, e_hc, e_hm, e_out = np_svgf(p, cv, hist[2], g, hist[3], a, hist[0].astype(np.float64), hist[1].astype(np.float64))
        prev = True
        # away from the border: a pixel whose reprojection leaves the frame by a fraction of a pixel may keep or lose its
        # history at W = 0.01 in one precision and not the other (a decision, not arithmetic)
        # A moved camera's reprojection (s, then dot(q, h') s - dot(a, h')) cancels: its float32 tap position carries ~1e-4 px of
        # error into a noisy history, so frames after a move agree to 1e-4; still frames to 1e-5.  The a-trous output after a
        # move to 2e-3: the luminance edge-stop exp(-|L - L'| / phi) turns those differences into differences of weights.
        b = 8
        rtol = 1e-5 if k == 0 or deg == views[k - 1] else 1e-4
        for got, exp, what in ((integ, e_integ, "integrated"), (hm[..., :3], e_hm, "moments"), (hc, e_hc, "history"), (out, e_out, "out")):
            got, exp = got[b:-b, b:-b], exp[b:-b, b:-b]
            r = rtol if what in ("integrated", "moments") or rtol == 1e-5 else 2e-3
            np.testing.assert_allclose(got[..., :3], exp[..., :3], rtol=r, atol=r * float(np.abs(exp[..., :3]).max()),
                                       err_msg=f"frame {k} ({deg} deg): {what}")
            if what != "moments" and what != "out":     # variance = a difference of moments: measured against their scale
                np.testing.assert_allclose(got[..., 3], exp[..., 3], rtol=r, atol=r * float(e_hm[..., 1].max()),
                                           err_msg=f"frame {k} ({deg} deg): {what} variance")
        if k >= 2 and deg != views[k - 1]:
            assert (hm[..., 2] > 1).mean() > 0.8           # a small step reprojects most pixels
